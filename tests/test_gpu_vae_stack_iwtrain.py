"""The layer-stack engine's training step on the K-sample importance-weighted bound
(vaeb_ae_config.iw_samples >= 2: vaeb_amd/csrc/engine_ae.inc ae_step / ae_iw_forward, ae_iwae.hpp
ae_iw_weight_kernel / ae_iw_plane_sum_kernel, ae_mlp.hpp B_LATENT_IW) against the float64 oracle
(tests/vae_stack_iwtrain_oracle.py) on identical theta / rows / eps.

Gradients are recovered per element from a step off a ZERO AdaGrad accumulator and judged per
parameter block at 16 x the float32 restatement's error, the value at VALUE_RTOL = 2e-5
(tests/ae_grad_cases.py); the cases, the IW-scaled weights and the bounds are built and checked in
tests/test_vae_stack_iwtrain_host.py, which also shows that eleven kinds of wrong gradient miss
these bounds.  The Philox step and the epoch trajectory use the tolerances of
tests/test_gpu_vae_stack.py.  No bound comes from the device.  Every test prints its
`device / restatement / bound` line (-s shows them).

Measured on an MI355X.  Per case the block nearest to its bound: device error / restatement
error / bound, and the value's relative error.

  case                           block    device  / restate / bound      value
  bin-theta0                     bzlv     3.8e-06 / 7.6e-07 / 1.2e-05   3.1e-08
  bin-iwscale                    bzlv     1.5e-06 / 4.8e-07 / 7.6e-06   5.6e-08
  cont-theta0                    bmu      1.5e-07 / 1.7e-07 / 2.7e-06   2.4e-08
  cont-iwscale                   bdec0    9.4e-08 / 7.4e-08 / 1.2e-06   2.3e-08
  relu-theta0                    benc0    3.4e-07 / 4.3e-07 / 6.9e-06   6.7e-08
  relu-iwscale                   Wout     4.4e-07 / 2.0e-07 / 3.2e-06   5.3e-08
  deep-theta0                    Wzmu     6.1e-07 / 4.6e-07 / 7.4e-06   5.2e-08
  deep-iwscale                   Wdec0    3.5e-07 / 3.3e-07 / 5.3e-06   2.2e-08
  full-theta0                    bmu      2.1e-07 / 1.6e-07 / 2.6e-06   4.1e-09
  full-iwscale                   bmu      1.6e-07 / 1.6e-07 / 2.5e-06   4.0e-08
  stale 11 rows-theta0           bmu      1.5e-07 / 8.1e-08 / 1.3e-06   1.6e-08
  stale then 5 rows-theta0       Wzlv     2.3e-06 / 1.4e-06 / 2.3e-05   4.7e-09
  stale 11 rows-iwscale          bmu      1.1e-07 / 9.5e-08 / 1.5e-06   7.3e-08
  stale then 5 rows-iwscale      bzlv     6.8e-07 / 5.1e-07 / 8.2e-06   1.4e-08

The device is at most 5.0 x the restatement, 0.32 of its bound (bzlv of bin-theta0, the block and
the reason of tests/test_gpu_ae_grads.py's worst row).  Philox step: value 3.2e-08 from the oracle;
epochs: worst value 1.2e-07, no theta element off; train's value x M against marginal_ll: 4.7e-08
(bin), 2.8e-08 (cont), cap 1e-5.  Nothing failed on the first run and no tolerance was widened.
"""
import numpy as np
import pytest

from oracle import ae_oracle as A
from tests import ae_grad_cases as G
from tests import test_vae_stack_iwtrain_host as C
from tests import vae_stack_iwtrain_oracle as T
from tests import vae_stack_oracle as V
from tests.test_gpu_vae_stack import assert_step as assert_step_caps
from tests.test_vae_stack_host import SEED, STEP

pytestmark = pytest.mark.gpu


def make_ctx(cfg, max_batch, iw_samples=None, latent="gauss"):
    from vaeb_amd import _lib
    kw = {} if iw_samples is None else {"iw_samples": iw_samples}
    return _lib.AEContext(cfg.Dobs, cfg.Denc, cfg.Dz, cfg.Ddec, otype=cfg.otype, act=cfg.act, s2=cfg.s2,
                          eta=cfg.eta, max_batch=max_batch, latent=latent, **kw)


def stacked(eps):
    """[K, n, Dz] -> the push [K n, Dz]: sample k of list position i at row k n + i."""
    return np.ascontiguousarray(eps, np.float32).reshape(-1, eps.shape[-1])


def zero_acc_step(ctx, st):
    """theta, a zero accumulator and the host eps of st loaded, one train(idx): (value, theta', acc')."""
    from vaeb_amd import _lib
    ctx.set_params(st.theta())
    ctx.set_adagrad_state(np.zeros(ctx.P, np.float32))
    ctx.set_eps_mode(_lib.EPS_HOST)
    ctx.push_eps(stacked(st.eps))
    v = ctx.train(st.idx)
    return v, ctx.get_params(), ctx.get_adagrad_state()


def assert_step(label, st, v, th1, ac1):
    err = st.device_errors(th1, ac1)
    vrel = abs(v - st.value64) / abs(st.value64)
    print(G.table_line(label, err, st.bound, st.restate) + f"   value {vrel:.1e}")
    bad = G.rejected(err, st.bound)
    assert not bad, {n: (err[n], st.restate[n], st.bound[n]) for n in bad}
    assert vrel <= G.VALUE_RTOL, (v, st.value64)


# ------------------------------------------------------------------ 1. per-block gradients and value
@pytest.mark.parametrize("name,scaled", C.GPU_CASES, ids=C.GPU_IDS)
def test_iw_step_gradient_per_block(name, scaled):
    st, _ = C.case(name, scaled)
    K, M = st.eps.shape[0], len(st.idx)
    ctx = make_ctx(st.cfg, K * M, K)
    try:
        assert ctx.iw_samples == K
        ctx.set_data(st.Xtr)
        v, th1, ac1 = zero_acc_step(ctx, st)
    finally:
        ctx.close()
    assert_step(f"{name}-{'iwscale' if scaled else 'theta0'}", st, v, th1, ac1)


# ------------------------------------------------------------------ 2. stale rows
@pytest.mark.parametrize("scaled", [False, True], ids=["theta0", "iwscale"])
def test_small_step_after_a_large_one(scaled):
    """K = 3, max_batch 33: a step of M = 11 (33 stacked rows), then theta and a zero accumulator
    again and a step of M = 5 on other rows, whose planes then sit at another stride among the first
    step's rows."""
    big, _ = C.case("stale11", scaled)
    small = C.stale_small(scaled)
    ctx = make_ctx(big.cfg, 33, 3)
    try:
        ctx.set_data(big.Xtr)
        first = zero_acc_step(ctx, big)
        second = zero_acc_step(ctx, small)
    finally:
        ctx.close()
    assert_step(f"stale 11 rows-{'iwscale' if scaled else 'theta0'}", big, *first)
    assert_step(f"stale then 5 rows-{'iwscale' if scaled else 'theta0'}", small, *second)


# ------------------------------------------------------------------ 3. Philox
def test_iw_philox_train_step():
    from vaeb_amd import _lib
    cfg, X, params, acc, idx = C.philox_setup()
    K = C.PHILOX_K
    ctx = make_ctx(cfg, K * len(idx), K)
    try:
        ctx.set_data(X)
        ctx.set_params(A.flatten(params))
        ctx.set_adagrad_state(A.flatten(acc))
        ctx.set_eps_mode(_lib.EPS_PHILOX, SEED)
        ctx.set_step(STEP)
        got = ctx.train(idx)
        ref, ref_p, ref_a, _ = C.step64(cfg, X, params, acc, idx, T.train_eps(SEED, idx, cfg.Dz, STEP, K))
        print(f"philox step: value device {got:.7f} oracle {ref:.7f} rel {abs(got - ref) / abs(ref):.1e}")
        assert_step_caps(ctx, got, ref, ref_p, ref_a, cfg.eta)
        assert ctx.get_step() == STEP + 1
    finally:
        ctx.close()


# ------------------------------------------------------------------ 4. epoch trajectory
def test_iw_epochs_with_partial_batch_track_oracle():
    from vaeb_amd import _lib
    cfg, X, params, epochs, eps = C.epoch_setup()
    ctx = make_ctx(cfg, C.EPOCH_K * C.EPOCH_B, C.EPOCH_K)
    try:
        ctx.set_data(X)
        ctx.set_params(A.flatten(params))
        ctx.set_eps_mode(_lib.EPS_HOST)
        ctx.set_step(STEP)
        got = []
        for batches, e in zip(epochs, eps):
            ctx.push_eps(stacked(e))
            got += list(ctx.train_many(np.concatenate(batches), C.EPOCH_B))
        assert ctx.get_step() == STEP + 8
        theta = ctx.get_params()
    finally:
        ctx.close()
    ref, ref_theta = C.epoch_trajectory(cfg, X, params, epochs, eps, np.float64)
    d = np.abs(theta - ref_theta)
    print(f"epochs: worst value rel {max(abs(g - r) / abs(r) for g, r in zip(got, ref)):.1e}; "
          f"theta share off {float((d > 1e-2 * cfg.eta).mean()):.1e}")
    C.assert_epoch_close(got, theta, ref, ref_theta, cfg.eta)


# ------------------------------------------------------------------ 5. value against marginal_ll
@pytest.mark.parametrize("name", ["bin", "cont"])
def test_iw_value_is_marginal_ll_of_the_same_eps(name):
    from vaeb_amd import _lib
    st, _ = C.case(name, True)
    K, M = st.eps.shape[0], len(st.idx)
    ctx = make_ctx(st.cfg, K * M, K)
    try:
        ctx.set_data(st.Xtr)
        ctx.set_params(st.theta())
        ctx.set_eps_mode(_lib.EPS_HOST)
        ctx.push_eps(stacked(st.eps))
        ml = ctx.marginal_ll(st.Xtr[st.idx], K)
        v = ctx.train(st.idx)
    finally:
        ctx.close()
    print(f"{name}: train value x M {v * M:.6f}, marginal_ll {ml:.6f}, rel {abs(v * M - ml) / abs(ml):.1e}")
    assert abs(v * M - ml) <= 1e-5 * abs(ml), (v * M, ml)


# ------------------------------------------------------------------ 6. evaluation on an IW context
def test_evaluation_calls_are_bitwise_those_of_an_elbo_context():
    from vaeb_amd import _lib
    st, _ = C.case("cont", True)
    X = st.Xtr
    res = []
    for K in (3, 1):
        ctx = make_ctx(st.cfg, 16, K)
        try:
            ctx.set_data(X)
            ctx.set_params(st.theta())
            ctx.set_eps_mode(_lib.EPS_PHILOX, SEED)
            ctx.set_step(STEP)
            res.append((ctx.elbo(X), ctx.marginal_ll(X, 4, rows=True), ctx.encode(X), ctx.reconstruct(X),
                        ctx.get_step()))
        finally:
            ctx.close()
    (e3, (m3, r3), z3, x3, s3), (e1, (m1, r1), z1, x1, s1) = res
    assert X.shape[0] > 16 and np.isfinite(e3) and np.isfinite(m3)
    assert e3 == e1 and m3 == m1 and s3 == s1 == STEP
    assert np.array_equal(r3, r1) and np.array_equal(z3, z1) and np.array_equal(x3, x1)


# ------------------------------------------------------------------ 7. the ELBO path is unchanged
def test_iw_samples_0_and_1_are_the_elbo_step():
    from vaeb_amd import _lib
    st, _ = C.case("cont", True)
    idx = np.concatenate([st.idx, st.idx[::-1]])[:25].astype(np.int32)
    res = []
    for K in (None, 0, 1):
        ctx = make_ctx(st.cfg, 10, K)
        try:
            ctx.set_data(st.Xtr)
            ctx.set_params(st.theta())
            ctx.set_eps_mode(_lib.EPS_PHILOX, SEED)
            ctx.set_step(STEP)
            vals = ctx.train_many(idx, 10)
            res.append((vals, ctx.get_params(), ctx.get_adagrad_state(), ctx.get_step()))
        finally:
            ctx.close()
    assert len(res[0][0]) == 3 and np.isfinite(res[0][0]).all() and res[0][3] == STEP + 3
    for other in res[1:]:
        assert np.array_equal(res[0][0], other[0]) and np.array_equal(res[0][1], other[1])
        assert np.array_equal(res[0][2], other[2]) and res[0][3] == other[3]
    # and it is the one-sample ELBO step of the oracle, not an importance-weighted one
    p = [q.astype(np.float64) for q in st.params]
    v, _, _, _ = V.train_step(p, [np.zeros_like(q) for q in p], st.Xtr.astype(np.float64), idx[:10],
                              V.train_eps(SEED, idx[:10], st.cfg.Dz, STEP), st.cfg)
    assert abs(res[0][0][0] - v) <= G.VALUE_RTOL * abs(v)


# ------------------------------------------------------------------ 8. errors
def test_iw_errors():
    from vaeb_amd import _lib
    cfg = A.AEConfig(Dobs=24, Denc=(12,), Dz=3, Ddec=(12,), otype="binary")
    X = G.data_for(cfg, 20, 0)
    for kw in (dict(iw_samples=2, latent="point"), dict(iw_samples=-1), dict(iw_samples=(1 << 20) + 1)):
        with pytest.raises(_lib.VaebError, match=r"error -1\b"):
            make_ctx(cfg, 8, **kw)
    ctx = make_ctx(cfg, 9, 2)
    try:
        ctx.set_data(X)
        ctx.set_params(A.flatten(V.init_params(cfg)))
        ctx.set_adagrad_state(np.full(ctx.P, 1e-4, np.float32))
        ctx.set_eps_mode(_lib.EPS_PHILOX, SEED)
        ctx.set_step(7)
        before = (ctx.get_params(), ctx.get_adagrad_state(), ctx.get_step())
        with pytest.raises(_lib.VaebError, match=r"error -1\b"):      # K M = 10 = max_batch + 1
            ctx.train(np.arange(5, dtype=np.int32))
        after = (ctx.get_params(), ctx.get_adagrad_state(), ctx.get_step())
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2]
        ctx.set_eps_mode(_lib.EPS_HOST)
        ctx.push_eps(np.zeros((4, 3), np.float32))                    # M rows, not K M
        with pytest.raises(_lib.VaebError, match=r"error -3\b"):
            ctx.train(np.arange(4, dtype=np.int32))
        ctx.push_eps(np.zeros((8, 3), np.float32))
        assert np.isfinite(ctx.train(np.arange(4, dtype=np.int32)))
        assert ctx.get_step() == 8
    finally:
        ctx.close()


# ------------------------------------------------------------------ 9. ConstructVAE
def test_construct_vae_iw_samples():
    from vaeb_amd import ae
    cfg = A.AEConfig(Dobs=64, Denc=(16,), Dz=4, Ddec=(16,), otype="binary")
    X = G.data_for(cfg, 250, 3)
    np.random.seed(15485863)
    train, reconstruct, encode, decode, theta = ae.ConstructVAE(X, Denc=[16], Dz=4, Ddec=[16], iw_samples=3)
    assert train.iw_samples == 3 and train.ctx.cfg.max_batch == 300
    b0 = train.marginal_ll(X, 3)
    vals = ae.train_epochs(train, X.shape[0], 2, batch_size=100, verbose=False)
    assert len(vals) == 6 and np.isfinite(vals).all() and vals[-1] > vals[0]
    assert train.ctx.get_step() == 6 and train.marginal_ll(X, 3) > b0
    train2 = ae.ConstructVAE(X, Denc=[16], Dz=4, Ddec=[16])[0]
    assert train2.iw_samples == 1 and train2.ctx.cfg.max_batch == 250
