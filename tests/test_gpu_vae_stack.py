"""Parity of the layer-stack engine's Gaussian latent (vaeb_ae_* with VAEB_AE_LATENT_GAUSS,
vaeb_amd/csrc/ae_mlp.hpp F_LATENT / B_LATENT) against the float64 NumPy oracle
(tests/vae_stack_oracle.py) on identical theta / acc / rows / eps.

Tolerances are those of tests/test_gpu_ae.py (fp32 MFMA, ~1-ulp hardware transcendentals):
  * train's value ((loglik - KL) / n): relative <= 2e-5
  * theta' after AdaGrad: check_theta; accumulator norm relative <= 1e-4
  * encode_dist mu / lv: absolute <= 2e-5 * max(1, |.|max)
  * 8-step epoch and elbo(X): relative <= 1e-4
  * device noise: EPS_ATOL = 2.3e-6, the bound tests/test_gpu_philox.py measured for the same
    device function
The inputs are shared with tests/test_vae_stack_host.py, which shows that they sit inside these
caps in float32 and tell a mis-keyed noise site apart.
"""
import numpy as np
import pytest

from oracle import ae_oracle as A
from oracle import philox
from tests import vae_stack_oracle as V
from tests.test_gpu_ae import check_theta, data_for
from tests.test_vae_stack_host import (ACC_RTOL, PHILOX_B, SEED, STEP, STEP_CASES, STEP_IDS, VALUE_RTOL, philox_setup,
                                       step64, step_setup)

pytestmark = pytest.mark.gpu

EPS_ATOL = 2.3e-6


def make_ctx(cfg, max_batch, latent="gauss"):
    from vaeb_amd import _lib
    return _lib.AEContext(cfg.Dobs, cfg.Denc, cfg.Dz, cfg.Ddec, otype=cfg.otype, act=cfg.act, s2=cfg.s2,
                          eta=cfg.eta, max_batch=max_batch, latent=latent)


def loaded(cfg, X, params, acc, max_batch, latent="gauss"):
    ctx = make_ctx(cfg, max_batch, latent)
    ctx.set_data(X)
    ctx.set_params(A.flatten(params))
    if acc is not None:
        ctx.set_adagrad_state(A.flatten(acc))
    return ctx


def assert_step(ctx, got, ref, ref_p, ref_a, eta):
    assert abs(got - ref) <= VALUE_RTOL * abs(ref), (got, ref)
    check_theta(ctx.get_params(), V.flatten(ref_p), eta)
    na, ra = ctx.get_adagrad_state(), V.flatten(ref_a)
    assert np.linalg.norm(na - ra) <= ACC_RTOL * np.linalg.norm(ra)


# ------------------------------------------------------------------ 1. single step, host eps
@pytest.mark.parametrize("name,kw,B,scale", STEP_CASES, ids=STEP_IDS)
def test_vae_stack_step_parity_host_eps(name, kw, B, scale):
    from vaeb_amd import _lib
    cfg, X, params, acc, idx, eps = step_setup(kw, B, scale)
    ctx = loaded(cfg, X, params, acc, B)
    assert ctx.P == sum(int(np.prod(s)) for _, s in V.param_shapes(cfg))
    ctx.set_eps_mode(_lib.EPS_HOST)
    ref, ref_p, ref_a, aux = step64(cfg, X, params, acc, idx, eps)
    # the encoder's distribution at the step's rows (before the step moves theta)
    ctx.push_eps(eps)
    mu, lv, z = ctx.encode_dist(X[idx])
    for got_a, want in ((mu, aux["mu"]), (lv, aux["lv"])):
        assert np.abs(got_a - want).max() <= 2e-5 * max(1.0, np.abs(want).max())
    got = ctx.train(idx)
    assert_step(ctx, got, ref, ref_p, ref_a, cfg.eta)
    ctx.close()


# ------------------------------------------------------------------ 2. device noise
def test_vae_stack_eval_noise_matches_host_philox():
    """Both latent heads zeroed: z = eps exactly.  Rows past the first max_batch chunk show the
    row key is the index in the call's x."""
    from vaeb_amd import _lib
    cfg = A.AEConfig(Dobs=24, Denc=(12,), Dz=20, Ddec=(12,), otype="binary")
    mb = 16
    n = 3 * mb + 7
    X = data_for(cfg, n, seed=1)
    params = V.init_params(cfg)
    for nm, p in zip(V.names(cfg), params):
        if nm in V.LATENT_NAMES:
            p[...] = 0
    ctx = loaded(cfg, X, params, None, mb)
    ctx.set_eps_mode(_lib.EPS_PHILOX, SEED)
    ctx.set_step(STEP)
    mu, lv, z = ctx.encode_dist(X)
    assert not mu.any() and not lv.any()
    want = philox.eval_eps(SEED, STEP, n, cfg.Dz, 0)
    assert np.abs(z - want).max() <= EPS_ATOL, np.abs(z - want).max()
    assert ctx.get_step() == STEP
    ctx.close()


# ------------------------------------------------------------------ 3. Philox-mode train step
def test_vae_stack_philox_train_step():
    from vaeb_amd import _lib
    cfg, X, params, acc, idx = philox_setup()
    ctx = loaded(cfg, X, params, acc, PHILOX_B)
    ctx.set_eps_mode(_lib.EPS_PHILOX, SEED)
    ctx.set_step(STEP)
    got = ctx.train(idx)
    eps = philox.latent_normal(SEED, idx.astype(np.int64)[:, None], np.arange(cfg.Dz, dtype=np.int64)[None, :], STEP, 0)
    ref, ref_p, ref_a, _ = step64(cfg, X, params, acc, idx, eps)
    assert_step(ctx, got, ref, ref_p, ref_a, cfg.eta)
    assert ctx.get_step() == STEP + 1
    ctx.close()


# ------------------------------------------------------------------ 4. two epochs, partial batch
def test_vae_stack_epochs_with_partial_batch_track_oracle():
    from vaeb_amd import _lib
    cfg = A.AEConfig(Dobs=96, Denc=(40,), Dz=6, Ddec=(40,), otype="binary")
    Ntr, B = 350, 100
    X = data_for(cfg, Ntr, seed=9)
    params = V.init_params(cfg)
    ctx = loaded(cfg, X, params, None, B)
    ctx.set_eps_mode(_lib.EPS_PHILOX, SEED)
    ctx.set_step(STEP)
    rs = np.random.RandomState(15485863)
    batches = A.epoch_batches(Ntr, B, rs) + A.epoch_batches(Ntr, B, rs)   # two epochs, 4 + 4 steps
    got = list(ctx.train_many(np.concatenate(batches[:4]), B)) + list(ctx.train_many(np.concatenate(batches[4:]), B))
    assert ctx.get_step() == STEP + 8
    p = [q.astype(np.float64) for q in params]
    a = [np.zeros_like(q) for q in p]
    ref = []
    for k, b in enumerate(batches):
        v, p, a, _ = V.train_step(p, a, X.astype(np.float64), b, V.train_eps(SEED, b, cfg.Dz, STEP + k), cfg)
        ref.append(v)
    assert [len(b) for b in batches[:4]] == [100, 100, 100, 50]
    for g, r in zip(got, ref):
        assert abs(g - r) <= 1e-4 * abs(r), (g, r)
    d = np.abs(ctx.get_params() - V.flatten(p))
    assert float((d > 1e-2 * cfg.eta).mean()) <= 1e-3
    ctx.close()


def test_vae_stack_host_eps_follows_the_rows_of_the_call():
    """Host eps past the first slice / chunk: train_many reads the eps rows of each slice of the
    idx list, encode_dist those of each max_batch chunk of x (Dz over two column tiles)."""
    from vaeb_amd import _lib
    name, kw, B, scale = STEP_CASES[1]
    cfg, X, params, _, _, _ = step_setup(kw, B, scale)
    rng = np.random.default_rng(8)
    n = B + 11
    idx = rng.choice(X.shape[0], size=n, replace=False).astype(np.int32)
    eps = rng.standard_normal((n, cfg.Dz)).astype(np.float32)
    ctx = loaded(cfg, X, params, None, B)
    ctx.set_eps_mode(_lib.EPS_HOST)
    ctx.push_eps(eps)
    p = [q.astype(np.float64) for q in params]
    want = V.forward_backward(p, X[idx].astype(np.float64), eps.astype(np.float64), cfg, need_grad=False)
    mu, lv, z = ctx.encode_dist(X[idx])
    for got_a, ref_a in ((mu, want["mu"]), (lv, want["lv"]), (z, want["z"])):
        assert np.abs(got_a - ref_a).max() <= 2e-5 * max(1.0, np.abs(ref_a).max())
    got = ctx.train_many(idx, B)
    a = [np.zeros_like(q) for q in p]
    for k, (lo, hi) in enumerate(((0, B), (B, n))):
        v, p, a, _ = V.train_step(p, a, X.astype(np.float64), idx[lo:hi], eps[lo:hi].astype(np.float64), cfg)
        assert abs(got[k] - v) <= 1e-4 * abs(v), (k, got[k], v)
    d = np.abs(ctx.get_params() - V.flatten(p))
    assert float((d > 1e-2 * cfg.eta).mean()) <= 1e-3
    ctx.close()


# ------------------------------------------------------------------ 5. elbo(X)
def test_vae_stack_elbo_is_forward_only():
    from vaeb_amd import _lib
    name, kw, B, scale = STEP_CASES[1]
    cfg, X, params, acc, idx, _ = step_setup(kw, B, scale)
    mb = 16
    n = X.shape[0]
    assert n > mb and n % mb
    ctx = loaded(cfg, X, params, acc, mb)
    ctx.set_eps_mode(_lib.EPS_PHILOX, SEED)
    ctx.set_step(STEP)
    before = (ctx.get_params(), ctx.get_adagrad_state(), ctx.get_step())
    got = ctx.elbo(X)
    again = ctx.elbo(X)
    after = (ctx.get_params(), ctx.get_adagrad_state(), ctx.get_step())
    eps = philox.eval_eps(SEED, STEP, n, cfg.Dz, 0)
    out = V.forward_backward([p.astype(np.float64) for p in params], X.astype(np.float64), eps, cfg, need_grad=False)
    assert abs(got - out["elbo"]) <= 1e-4 * abs(out["elbo"]), (got, out["elbo"])
    assert got == again
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2]
    ctx.close()


# ------------------------------------------------------------------ 6. degenerate identity
def test_vae_stack_zero_noise_zero_lv_head_trains_like_the_point_model():
    from vaeb_amd import _lib
    name, kw, B, _ = STEP_CASES[0]
    cfg = A.AEConfig(**kw)
    X = data_for(cfg, 4 * B)
    point = [(p * 30).astype(np.float32) for p in A.init_params(cfg, seed=3)]
    gauss = V.from_point(point, cfg)
    idx = np.random.default_rng(2).choice(X.shape[0], size=B, replace=False).astype(np.int32)
    acc_p = [np.full(p.shape, 1e-4, np.float32) for p in point]
    acc_g = [np.full(p.shape, 1e-4, np.float32) for p in gauss]
    pc = loaded(cfg, X, point, acc_p, B, latent="point")
    gc = loaded(cfg, X, gauss, acc_g, B)
    gc.set_eps_mode(_lib.EPS_HOST)
    gc.push_eps(np.zeros((B, cfg.Dz), np.float32))
    pc.train(idx)
    gc.train(idx)
    pt = dict(zip([n for n, _ in A.param_shapes(cfg)], A.unflatten(pc.get_params(), cfg)))
    for n, g in zip(V.names(cfg), V.unflatten(gc.get_params(), cfg)):
        if n in V.LV_NAMES:
            continue
        check_theta(g.ravel(), pt[{"Wzmu": "Wz", "bzmu": "bz"}.get(n, n)].ravel(), cfg.eta)
    pc.close()
    gc.close()


# ------------------------------------------------------------------ 7. errors
def test_vae_stack_calls_on_a_point_context_and_eps_row_mismatch():
    from vaeb_amd import _lib
    cfg = A.AEConfig(Dobs=24, Denc=(12,), Dz=3, Ddec=(12,), otype="binary")
    X = data_for(cfg, 20)
    pc = make_ctx(cfg, 8, latent="point")
    pc.set_data(X)
    calls = [lambda: pc.set_eps_mode(_lib.EPS_HOST), lambda: pc.push_eps(np.zeros((4, 3), np.float32)),
             lambda: pc.set_step(1), lambda: pc.get_step(), lambda: pc.encode_dist(X), lambda: pc.elbo(X)]
    for call in calls:
        with pytest.raises(_lib.VaebError, match=r"error -1\b"):
            call()
    pc.close()
    gc = make_ctx(cfg, 8)
    gc.set_data(X)
    gc.set_params(A.flatten(V.init_params(cfg)))
    gc.set_eps_mode(_lib.EPS_HOST)
    gc.push_eps(np.zeros((5, 3), np.float32))
    with pytest.raises(_lib.VaebError, match=r"error -3\b"):
        gc.train(np.arange(4, dtype=np.int32))
    assert np.isfinite(gc.train(np.arange(5, dtype=np.int32)))
    gc.close()


# ------------------------------------------------------------------ 8. ConstructVAE
def test_construct_vae_mirror_learns():
    from vaeb_amd import ae
    cfg = A.AEConfig(Dobs=784, Denc=(64,), Dz=8, Ddec=(64,), otype="binary", act="relu")
    X = data_for(cfg, 1000, seed=3)
    np.random.seed(15485863)
    train, reconstruct, encode, decode, theta = ae.ConstructVAE(X, Denc=[64], Dz=8, Ddec=[64], f="relu")
    ref0 = V.init_params(cfg, seed=15485863)
    assert [t.name for t in theta][2:6] == ["Wzmu", "Wzlv", "bzmu", "bzlv"]
    assert all(np.array_equal(t.get_value(), r) for t, r in zip(theta, ref0))
    e0 = train.elbo(X)
    vals = ae.train_epochs(train, X.shape[0], 3, verbose=False)
    assert len(vals) == 30 and np.isfinite(vals).all() and vals[-1] > vals[0]
    assert np.isfinite(e0) and train.elbo(X) > e0
    assert train.ctx.get_step() == 30
    z = encode(X[:7])
    assert z.shape == (7, 8) and decode(z).shape == (7, 784)
    assert reconstruct(X[:7]).shape == (7, 784)
