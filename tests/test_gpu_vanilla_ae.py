"""The vanilla squared-error autoencoder on the layer-stack engine (VAEB_AE_SE output,
VAEB_AE_LATENT_ACT latent, vaeb_ae_sq_error: vaeb_amd/csrc/ae_mlp.hpp PAeFwdT<true>, engine_ae.inc)
against the float64 oracle tests/vanilla_ae_oracle.py.

1. Per-block gradient parity of one train step from a ZERO accumulator (recovery, error measure and
   the 16 x float32-restatement bound of tests/ae_grad_cases.py; cases and inputs in
   tests/vanilla_ae_cases.py); the step's value se / M within VALUE_RTOL = 2e-5.
   tests/test_vanilla_ae_host.py shows that six kinds of wrong gradient miss these bounds and that
   every bound is <= 1e-4.  No bound comes from the device.
2. Stale rows: a 33-row step, then a 5-row step on the same context.
3. reconstruct / encode (the activated code) / decode: absolute <= 2e-5 at x 30 weights.
4. sq_error: rows and sum within VALUE_RTOL on four kinds of context, rows bitwise independent of
   max_batch, no state changed.
5. Two epochs with a partial last batch track the oracle per step within 1e-4.
6. Argument errors.  7. ConstructVanillaAE.  8. The vanilla_ae driver on a toy.

Measured on an MI355X (every step test prints its line; -s shows them).  Per case the block nearest
to its bound: device error / restatement error / bound, and the value's relative error.

  case                                 block    device  / restate / bound      value
  edge_bin_tanh-act-se-theta0          bdec1    6.1e-07 / 4.8e-07 / 7.7e-06   4.2e-09
  edge_bin_tanh-act-se-x30             bout     1.3e-07 / 6.7e-08 / 1.1e-06   6.6e-09
  edge_cont_sigmoid-act-se-theta0      Wout     4.5e-07 / 4.4e-07 / 7.0e-06   3.0e-08
  edge_cont_sigmoid-act-se-x30         benc0    7.0e-08 / 3.2e-08 / 5.1e-07   2.5e-08
  edge_relu_b1-act-se-theta0           bdec0    8.0e-08 / 6.4e-08 / 1.0e-06   4.3e-08
  edge_relu_b1-act-se-x30              benc0    5.0e-08 / 2.8e-08 / 4.4e-07   9.5e-08
  k512_513-act-se-theta0               bout     3.9e-07 / 1.6e-07 / 2.6e-06   8.3e-10
  k512_513-act-se-x30                  bdec0    1.4e-07 / 1.4e-07 / 2.2e-06   1.8e-08
  batch_512-act-se-theta0              Wout     1.0e-06 / 7.0e-07 / 1.1e-05   4.4e-08
  batch_512-act-se-x30                 benc0    7.0e-08 / 2.5e-07 / 4.0e-06   9.1e-09
  batch_513-act-se-theta0              Wout     1.5e-06 / 9.0e-07 / 1.4e-05   4.0e-08
  batch_513-act-se-x30                 bz       9.4e-08 / 9.4e-08 / 1.5e-06   4.8e-08
  edge_bin_tanh-act-binary-theta0      Wdec1    8.6e-08 / 6.7e-08 / 1.1e-06   5.1e-08
  edge_bin_tanh-act-binary-x30         bz       1.1e-07 / 1.8e-08 / 2.9e-07   3.2e-08
  edge_cont_sigmoid-act-cont-theta0    bdec0    1.3e-07 / 4.8e-08 / 7.7e-07   2.9e-08
  edge_cont_sigmoid-act-cont-x30       bmu      1.4e-07 / 6.4e-08 / 1.0e-06   1.9e-08
  edge_bin_tanh-point-se-theta0        bdec1    6.1e-07 / 4.4e-07 / 7.1e-06   4.2e-09
  edge_bin_tanh-point-se-x30           Wdec0    1.5e-07 / 9.0e-08 / 1.4e-06   3.6e-08
  stale-act-se 33 rows                 bdec0    1.4e-07 / 1.4e-07 / 2.2e-06   1.8e-08
  stale-act-se then 5 rows             Wdec0    8.9e-08 / 8.9e-08 / 1.4e-06   6.8e-08

The device is at most 6.1 x the restatement, 0.38 of its bound (bz of edge_bin_tanh-act-binary-x30,
Dz = 1: one column sum of 17 terms), and on the batch_512 / batch_513 x30 rows below it, as in
tests/test_gpu_ae_grads.py.  sq_error: rows within 1.4e-07 and the sum within 2.6e-08 of float64 on
all four kinds of context (bound 2e-5).  Nothing failed on the first run and no kernel changed after it.
"""
import os

import numpy as np
import pytest

from oracle import ae_oracle as A
from tests import ae_grad_cases as G
from tests import vae_stack_oracle as V
from tests import vanilla_ae_cases as C
from tests import vanilla_ae_oracle as VA

pytestmark = pytest.mark.gpu


def make_ctx(cfg, max_batch, latent, **kw):
    from vaeb_amd import _lib
    return _lib.AEContext(cfg.Dobs, cfg.Denc, cfg.Dz, cfg.Ddec, otype=cfg.otype, act=cfg.act, s2=cfg.s2,
                          eta=cfg.eta, max_batch=max_batch, latent=latent, **kw)


def zero_acc_step(ctx, st):
    ctx.set_params(st.theta())
    ctx.set_adagrad_state(np.zeros(ctx.P, np.float32))
    v = ctx.train(st.idx)
    return v, ctx.get_params(), ctx.get_adagrad_state()


def assert_step(label, st, v, th1, ac1):
    err = st.device_errors(th1, ac1)
    vrel = abs(v - st.value64) / abs(st.value64)
    print(G.table_line(label, err, st.bound, st.restate) + f"   value {vrel:.1e}")
    bad = G.rejected(err, st.bound)
    assert not bad, {n: (err[n], st.restate[n], st.bound[n]) for n in bad}
    assert vrel <= G.VALUE_RTOL, (v, st.value64)


# ------------------------------------------------------------------ 1. gradient per block
@pytest.mark.parametrize("name,latent,otype,scaled", C.CASES, ids=C.CASE_IDS)
def test_step_gradient_per_block(name, latent, otype, scaled):
    st = C.case(name, latent, otype, scaled)
    ctx = make_ctx(st.cfg, len(st.idx), latent)
    try:
        assert ctx.P == sum(int(np.prod(s)) for _, s in st.shapes)
        ctx.set_data(st.Xtr)
        v, th1, ac1 = zero_acc_step(ctx, st)
    finally:
        ctx.close()
    if otype == "se":
        assert v > 0                                   # se / M, not -se / M
    assert_step(f"{name}-{latent}-{otype}-{'x30' if scaled else 'theta0'}", st, v, th1, ac1)


# ------------------------------------------------------------------ 2. stale rows
def test_small_batch_after_a_large_one():
    big = C.case("k512_513", "act", "se", True)
    assert len(big.idx) == 33
    idx5 = np.random.default_rng(7).choice(big.Xtr.shape[0], size=5, replace=False).astype(np.int32)
    small = C.make_step(big.cfg, "act", big.params, big.Xtr, idx5)
    assert max(small.bound.values()) <= G.GRAD_CAP
    ctx = make_ctx(big.cfg, 33, "act")
    try:
        ctx.set_data(big.Xtr)
        first = zero_acc_step(ctx, big)
        second = zero_acc_step(ctx, small)
    finally:
        ctx.close()
    assert_step("stale-act-se 33 rows", big, *first)
    assert_step("stale-act-se then 5 rows", small, *second)


# ------------------------------------------------------------------ 3. predictions
PREDICT = [
    ("deep_odd_tanh", dict(Dobs=37, Denc=(29, 17), Dz=5, Ddec=(13, 21), otype="se", s2=2.0), 23),
    ("deep_sigmoid", dict(Dobs=48, Denc=(20,), Dz=4, Ddec=(18, 11), otype="se", act="sigmoid"), 30),
    ("relu", dict(Dobs=64, Denc=(32,), Dz=8, Ddec=(32,), otype="se", act="relu"), 32),
]


@pytest.mark.parametrize("name,kw,B", PREDICT, ids=[c[0] for c in PREDICT])
def test_predict_parity(name, kw, B):
    cfg = A.AEConfig(**kw)
    X = C.data_for(cfg, 3 * B, 4)
    params = [(p * 30).astype(np.float32) for p in VA.init_params(cfg, seed=7)]
    out = VA.forward_backward([p.astype(np.float64) for p in params], X.astype(np.float64), cfg, "act", need_grad=False)
    Z, Xpr = out["Z"], out["Xpr"]
    if cfg.act == "tanh":
        assert np.abs(Z).max() > 0.9                   # f matters in encode
    ztol = 2e-5 * max(1.0, np.abs(Z).max())
    ctx = make_ctx(cfg, B, "act")
    try:
        ctx.set_params(A.flatten(params))
        for n in (3 * B, 2 * B + 7):
            assert np.abs(ctx.reconstruct(X[:n]) - Xpr[:n]).max() <= 2e-5
            assert np.abs(ctx.encode(X[:n]) - Z[:n]).max() <= ztol
            assert np.abs(ctx.decode(Z[:n].astype(np.float32)) - Xpr[:n]).max() <= 2e-5
    finally:
        ctx.close()


# ------------------------------------------------------------------ 4. sq_error
def sq_reference(cfg, latent, params, X):
    """Row values sum_d (x - Xpr)^2 of the float64 deterministic forward (gauss: z = mu; cont: the mean)."""
    p64, X64 = [p.astype(np.float64) for p in params], X.astype(np.float64)
    if latent == "gauss":
        out = V.forward_backward(p64, X64, np.zeros((X.shape[0], cfg.Dz)), cfg, need_grad=False)
    else:
        out = VA.forward_backward(p64, X64, cfg, latent, need_grad=False)
    return ((X64 - out["Xpr"]) ** 2).sum(1)


SQ = [("act", "se"), ("point", "binary"), ("point", "cont"), ("gauss", "cont")]


@pytest.mark.parametrize("latent,otype", SQ, ids=["-".join(c) for c in SQ])
def test_sq_error(latent, otype):
    from vaeb_amd import _lib
    cfg = A.AEConfig(Dobs=37, Denc=(17,), Dz=5, Ddec=(15,), otype=otype, act="tanh")
    B = 7
    n = 2 * B + 7
    X = C.data_for(cfg, n, 5)
    if latent == "gauss":
        params = [(p * 30).astype(np.float32) for p in V.init_params(cfg, seed=7)]
    else:
        params = [(p * 30).astype(np.float32) for p in VA.init_params(cfg, seed=7)]
    ref = sq_reference(cfg, latent, params, X)
    rows = {}
    for mb in (B, 64):
        ctx = make_ctx(cfg, mb, latent)
        try:
            ctx.set_params(A.flatten(params))
            acc = np.random.default_rng(1).random(ctx.P).astype(np.float32)
            ctx.set_adagrad_state(acc)
            if latent == "gauss":
                ctx.set_eps_mode(_lib.EPS_PHILOX, 3)
                ctx.set_step(11)
            total, r = ctx.sq_error(X, rows=True)
            only = ctx.sq_error(X)
            assert np.array_equal(ctx.get_params(), A.flatten(params))
            assert np.array_equal(ctx.get_adagrad_state(), acc)
            if latent == "gauss":
                assert ctx.get_step() == 11
            if mb == B:
                # Xpr is what reconstruct returns
                rec = ctx.reconstruct(X).astype(np.float64)
                assert np.abs(((X - rec) ** 2).sum(1) - r).max() <= G.VALUE_RTOL * ref.max()
        finally:
            ctx.close()
        print(f"sq_error {latent}-{otype} max_batch {mb}: rows {np.abs(r - ref).max() / ref.max():.1e} "
              f"(worst row {(np.abs(r - ref) / ref).max():.1e}), sum {abs(total - ref.sum()) / ref.sum():.1e}")
        assert r.dtype == np.float32 and r.shape == (n,)
        assert (np.abs(r - ref) <= G.VALUE_RTOL * ref).all()
        assert abs(total - ref.sum()) <= G.VALUE_RTOL * ref.sum()
        assert abs(only - total) <= 1e-12 * total          # rows=False: the same sum
        assert abs(total - float(r.astype(np.float64).sum())) <= 1e-12 * total   # the fp64 sum of the float rows
        rows[mb] = r
    assert np.array_equal(rows[B], rows[64])               # a row's value does not depend on max_batch


# ------------------------------------------------------------------ 5. an epoch
def test_epoch_with_partial_batch_tracks_oracle():
    cfg = A.AEConfig(Dobs=96, Denc=(40,), Dz=6, Ddec=(40,), otype="se")
    Ntr, B = 350, 100
    X = C.data_for(cfg, Ntr, 9)
    params = VA.init_params(cfg)
    rs = np.random.RandomState(15485863)
    batches = VA.epoch_batches(Ntr, B, rs) + VA.epoch_batches(Ntr, B, rs)
    assert [len(b) for b in batches[:4]] == [100, 100, 100, 50]
    ctx = make_ctx(cfg, B, "act")
    try:
        ctx.set_data(X)
        ctx.set_params(A.flatten(params))
        got = list(ctx.train_many(np.concatenate(batches[:4]), B)) + list(ctx.train_many(np.concatenate(batches[4:]), B))
        theta = ctx.get_params()
    finally:
        ctx.close()
    p = [q.astype(np.float64) for q in params]
    a = [np.zeros_like(q) for q in p]
    ref = []
    for b in batches:
        v, p, a, _ = VA.train_step(p, a, X.astype(np.float64), b, cfg, "act")
        ref.append(v)
    assert len(got) == 8
    for g, r in zip(got, ref):
        assert abs(g - r) <= 1e-4 * abs(r), (g, r)
    d = np.abs(theta - A.flatten(p))
    assert float((d > 1e-2 * cfg.eta).mean()) <= 1e-3


# ------------------------------------------------------------------ 6. errors
def test_argument_errors():
    from vaeb_amd import _lib
    cfg = A.AEConfig(Dobs=20, Denc=(9,), Dz=3, Ddec=(8,), otype="se")
    with pytest.raises(_lib.VaebError, match=r"error -1\b"):
        make_ctx(cfg, 8, "gauss")                       # -se is no log-likelihood
    with pytest.raises(_lib.VaebError, match=r"error -1\b"):
        make_ctx(cfg, 8, "act", iw_samples=2)
    ctx = make_ctx(cfg, 8, "act")
    try:
        x = C.data_for(cfg, 4, 0)
        for call in (lambda: ctx.elbo(x), lambda: ctx.set_eps_mode(_lib.EPS_PHILOX, 1), lambda: ctx.marginal_ll(x, 3),
                     lambda: ctx.sq_error(x[:0])):
            with pytest.raises(_lib.VaebError, match=r"error -1\b"):
                call()
        assert ctx.sq_error(x) > 0                      # the context still works
    finally:
        ctx.close()


# ------------------------------------------------------------------ 7. ConstructVanillaAE
def test_construct_vanilla_ae():
    from vaeb_amd import ae
    cfg_binary = A.AEConfig(Dobs=784, Denc=(64,), Dz=5, Ddec=(64,), otype="binary")
    # pixels with their own means (iid Beta(2, 2) rows have nothing to learn: 1/2 is already their mean)
    from vaeb_amd import synthetic
    X = synthetic.mnist_like(1000)
    np.random.seed(15485863)
    train, reconstruct, encode, decode, theta = ae.ConstructVanillaAE(X, Denc=[64], Dz=5, Ddec=[64])
    try:
        ref0 = A.init_params(cfg_binary, seed=15485863)
        assert len(theta) == len(ref0) and all(np.array_equal(t.get_value(), r) for t, r in zip(theta, ref0))
        se = []
        for _ in range(3):
            idx = np.random.permutation(1000).astype(np.int32)
            se.extend(train.ctx.train_many(idx, 100).tolist())
        assert len(se) == 30 and np.isfinite(se).all() and 0 < se[-1] < se[0]
        one = train(np.arange(50))
        assert np.isfinite(one) and one > 0
        host = ae.mse(X, reconstruct(X))
        assert abs(train.mse(X) - host) <= 1e-5 * host
        z = encode(X[:7])
        assert z.shape == (7, 5) and (np.abs(z) < 1).all()
        assert decode(z).shape == (7, 784)
    finally:
        train.ctx.close()
    with pytest.raises(ValueError):
        ae.ConstructAE(X, otype="se")                   # ConstructAE keeps to binary | cont


# ------------------------------------------------------------------ 8. the driver
def test_driver_writes_the_result_table(tmp_path, capsys):
    from vaeb_amd import synthetic, vanilla_ae
    frey, mnist = synthetic.frey_like(340), synthetic.mnist_like(340)
    data = {"continuous": (frey[:300], frey[300:]), "discrete": (mnist[:300], mnist[300:])}
    res = vanilla_ae.main(["--out", str(tmp_path), "--epochs", "2", "--dz", "2", "--hidden", "16"], data=data)
    lines = open(os.path.join(tmp_path, "AE_MSE.res")).read().split("\n")
    assert lines[0] == "data_type,latent_size,MSE" and lines[3:] == [""]
    for line, kind in zip(lines[1:3], ("continuous", "discrete")):
        a, b, c = line.split(",")
        assert (a, b) == (kind, "2") and np.isfinite(float(c)) and float(c) > 0
        assert float(c) == res[(kind, 2)]
    for kind in ("continuous", "discrete"):
        for t in range(8):
            for what in ("orig", "recon"):
                assert os.path.getsize(os.path.join(tmp_path, f"AE_{kind}_2_{what}_{t}.jpg")) > 0
    out = capsys.readouterr().out.split("\n")
    assert out.count("Training the autoencoder.") == 2
    for i in (0, 1):
        assert sum(l.startswith(f"Epoch {i}. mse = ") for l in out) == 2
    assert sum(l.startswith("training rmse = ") for l in out) == 2
    assert sum(l.startswith("testing rmse = ") for l in out) == 2
