"""Parity of the layer-stack engine's denoising training (vaeb_ae_config.corruption,
vaeb_amd/csrc/ae_corrupt.hpp, engine_ae.inc ae_step) against the float64 oracle
(tests/denoise_oracle.py) on identical theta / acc / rows / draws.

Tolerances are the project's own:
  * a step's value: relative <= VALUE_RTOL = 2e-5; theta': check_theta; accumulator norm <= ACC_RTOL = 1e-4
  * multi-step runs: per-step value relative <= 1e-4, theta' off by > 1e-2 eta in <= 1e-3 of its elements
    (test_vae_stack_epochs_with_partial_batch_track_oracle)
  * the replacing kinds' xt: exact (the decisions compare exactly representable float32 values)
  * the additive kind's xt: |xt - ref| <= level * EPS_ATOL + 2.4e-7 * max(1, |xt|): EPS_ATOL = 2.3e-6 is the
    measured error of the device normal (tests/test_gpu_philox.py), 2.4e-7 = 2 * 2^-23 the two float32
    roundings of x + p n
The cases are defined in tests/test_denoise_host.py, which shows that they sit inside these caps in
float32, tell a mis-keyed draw apart and show a step scored on the corrupted rows or a first-layer
gradient taken from the clean ones.
"""
import numpy as np
import pytest

from oracle import ae_oracle as A
from tests import denoise_oracle as D
from tests.test_denoise_host import COR_SEED, DENOISE_IDS, SHAPES, denoise_case, oracle_step, philox_case
from tests.test_gpu_ae import check_theta, data_for
from tests.test_vae_stack_host import ACC_RTOL, SEED, STEP, VALUE_RTOL, step_setup

pytestmark = pytest.mark.gpu

EPS_ATOL = 2.3e-6
ROUND_RTOL = 2.4e-7


def make_ctx(cfg, max_batch, latent, corruption="none", iw_samples=1):
    from vaeb_amd import _lib
    return _lib.AEContext(cfg.Dobs, cfg.Denc, cfg.Dz, cfg.Ddec, otype=cfg.otype, act=cfg.act, s2=cfg.s2,
                          eta=cfg.eta, max_batch=max_batch, latent=latent, iw_samples=iw_samples,
                          corruption=corruption)


def loaded(cfg, X, params, acc, max_batch, latent, corruption="none", iw_samples=1):
    ctx = make_ctx(cfg, max_batch, latent, corruption, iw_samples)
    ctx.set_data(X)
    ctx.set_params(A.flatten(params))
    if acc is not None:
        ctx.set_adagrad_state(A.flatten(acc))
    return ctx


def state(ctx):
    return ctx.get_params(), ctx.get_adagrad_state()


def assert_step(ctx, got, ref, eta):
    rv, rp, ra = ref
    print(f"value {got!r} ref {rv!r} rel {abs(got - rv) / abs(rv):.2e}")
    assert abs(got - rv) <= VALUE_RTOL * abs(rv), (got, rv)
    check_theta(ctx.get_params(), A.flatten(rp), eta)
    na, fa = ctx.get_adagrad_state(), A.flatten(ra)
    assert np.linalg.norm(na - fa) <= ACC_RTOL * np.linalg.norm(fa)


def case_ctx(c, host=True):
    """The case's context, loaded, in host (pushed draws) or Philox noise mode."""
    from vaeb_amd import _lib
    B = len(c.idx)
    ctx = loaded(c.cfg, c.X, c.params, c.acc, max(c.K, 1) * B, c.latent, c.kind, c.K)
    ctx.set_corruption_level(c.level)
    if host:
        ctx.set_corruption_noise(_lib.EPS_HOST)
        ctx.push_corruption(c.draw)
        if c.latent == "gauss":
            ctx.set_eps_mode(_lib.EPS_HOST)
            ctx.push_eps(c.eps.reshape(-1, c.cfg.Dz))
    return ctx


# ------------------------------------------------------------------ 1. corrupt(idx) against the oracle
@pytest.mark.parametrize("kind,level", [("mask", 0.3), ("saltpepper", 0.3), ("gauss", 1.0)])
def test_corrupt_matches_the_host_draw(kind, level):
    from vaeb_amd import _lib
    _, kw, B, scale = SHAPES["A"]
    cfg, X, params, acc, _, _ = step_setup(kw, B, scale)
    params = D.init_params(cfg, "point")
    acc = [np.full(p.shape, 1e-4, np.float32) for p in params]
    rng = np.random.default_rng(21)
    idx = rng.choice(X.shape[0], size=2 * B + 7, replace=False).astype(np.int32)
    idx[-1] = idx[3]                                    # a repeated row: the same corruption
    ctx = loaded(cfg, X, params, acc, B, "point", kind)
    try:
        ctx.set_corruption_noise(_lib.EPS_PHILOX, COR_SEED)
        ctx.set_corruption_level(level)
        ctx.set_step(STEP)
        before = state(ctx)
        got = ctx.corrupt(idx)
        again = ctx.corrupt(idx)
        r, n = D.corruption_draws(COR_SEED, idx, cfg.Dobs, STEP)
        ref = D.corrupt(X[idx].astype(np.float64), kind, level, n if kind == "gauss" else r)
        assert got.shape == ref.shape == (len(idx), cfg.Dobs)
        if kind == "gauss":
            err = np.abs(got - ref)
            print(f"gauss xt: max |err| {err.max():.3e}")
            assert (err <= level * EPS_ATOL + ROUND_RTOL * np.maximum(1.0, np.abs(got))).all(), err.max()
        else:
            assert int((got != ref).sum()) == 0
            # the draw is at work.  Binary rows with 30 % ones at p = 0.3: a mask changes the ones it
            # hits, 0.3 * 0.3 = 0.09 of the 1961 elements; salt and pepper 0.3 * 0.15 + 0.7 * 0.15 = 0.15
            assert 0.05 < float((got != X[idx]).mean()) < 0.25
        assert np.array_equal(got, again) and np.array_equal(got[-1], got[3])
        after = state(ctx)
        assert ctx.get_step() == STEP and ctx.get_corruption_level() == np.float32(level)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    finally:
        ctx.close()


# ------------------------------------------------------------------ 2. single step, host-pushed draws
@pytest.mark.parametrize("name", DENOISE_IDS)
def test_denoise_step_parity_host_draws(name):
    c = denoise_case(name)
    ctx = case_ctx(c)
    try:
        xt = ctx.corrupt(c.idx)
        want = D.corrupt(c.X[c.idx], c.kind, c.level, c.draw)
        if c.kind == "gauss":
            assert np.abs(xt - want).max() <= ROUND_RTOL * max(1.0, np.abs(want).max())
        else:
            assert np.array_equal(xt, want)
        got = ctx.train(c.idx)
        assert_step(ctx, got, oracle_step(c, np.float64), c.cfg.eta)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 3. single step, Philox draws
def test_denoise_step_parity_philox_draws():
    from vaeb_amd import _lib
    c = philox_case()
    ctx = case_ctx(c, host=False)
    try:
        ctx.set_eps_mode(_lib.EPS_PHILOX, SEED)
        ctx.set_corruption_noise(_lib.EPS_PHILOX, COR_SEED)
        ctx.set_step(STEP)
        got = ctx.train(c.idx)
        assert_step(ctx, got, oracle_step(c, np.float64), c.cfg.eta)
        assert ctx.get_step() == STEP + 1                # the latent and the corruption share the step word
    finally:
        ctx.close()


def test_point_context_with_corruption_advances_the_step_once():
    from vaeb_amd import _lib
    c = denoise_case("B_point_cont_gauss")
    ctx = case_ctx(c, host=False)
    try:
        ctx.set_corruption_noise(_lib.EPS_PHILOX, COR_SEED)
        ctx.set_step(STEP)
        got = ctx.train(c.idx)
        _, n = D.corruption_draws(COR_SEED, c.idx, c.cfg.Dobs, STEP)
        c.draw = n
        assert_step(ctx, got, oracle_step(c, np.float64), c.cfg.eta)
        assert ctx.get_step() == STEP + 1
    finally:
        ctx.close()


# ------------------------------------------------------------------ 4. level 0 is the clean engine
@pytest.mark.parametrize("kind", D.KINDS)
@pytest.mark.parametrize("name", ["A_gauss_bin_mask", "C_act_se_saltpepper"])
def test_level_zero_is_the_clean_engine_bit_for_bit(name, kind):
    from vaeb_amd import _lib
    c = denoise_case(name)
    B = len(c.idx)
    outs = []
    for corruption in ("none", kind):
        ctx = loaded(c.cfg, c.X, c.params, c.acc, B, c.latent, corruption)
        try:
            if c.latent == "gauss":
                ctx.set_eps_mode(_lib.EPS_PHILOX, SEED)
                ctx.set_step(STEP)
            if corruption != "none":
                ctx.set_corruption_noise(_lib.EPS_PHILOX, COR_SEED)
                ctx.set_step(STEP)
                assert ctx.get_corruption_level() == 0.0
            outs.append((ctx.train(c.idx),) + state(ctx))
        finally:
            ctx.close()
    (v0, p0, a0), (v1, p1, a1) = outs
    assert v0 == v1 and np.array_equal(p0, p1) and np.array_equal(a0, a1)
    assert not np.array_equal(p0, A.flatten(c.params))


# ------------------------------------------------------------------ 5. an epoch, a partial slice, two levels
def test_denoise_epochs_follow_the_pushed_rows_and_the_level():
    from vaeb_amd import _lib
    cfg = A.AEConfig(Dobs=96, Denc=(40,), Dz=6, Ddec=(40,), otype="binary")
    Ntr, B = 350, 100
    X = data_for(cfg, Ntr, seed=9)
    params = A.init_params(cfg)
    rng = np.random.default_rng(12)
    draw = rng.random((Ntr, cfg.Dobs)).astype(np.float32)
    rs = np.random.RandomState(15485863)
    epochs = [np.concatenate(A.epoch_batches(Ntr, B, rs)) for _ in range(2)]
    levels = [0.4, 0.1]
    ctx = loaded(cfg, X, params, None, B, "point", "mask")
    try:
        ctx.set_corruption_noise(_lib.EPS_HOST)
        ctx.push_corruption(draw)                        # stays for both calls
        got = []
        for idx, level in zip(epochs, levels):
            ctx.set_corruption_level(level)
            got += list(ctx.train_many(idx, B))
        assert ctx.get_step() == 8
        p = [q.astype(np.float64) for q in params]
        a = [np.zeros_like(q) for q in p]
        ref, sizes = [], []
        X64 = X.astype(np.float64)
        for idx, level in zip(epochs, levels):
            for lo in range(0, Ntr, B):
                rows = idx[lo:lo + B]
                xt = D.corrupt(X64[rows], "mask", level, draw[lo:lo + B])   # the slice's own rows of the push
                v, p, a, _ = D.train_step(p, a, xt, X64[rows], cfg, "point")
                ref.append(v)
                sizes.append(len(rows))
        assert sizes == [100, 100, 100, 50] * 2
        for k, (g, r) in enumerate(zip(got, ref)):
            assert abs(g - r) <= 1e-4 * abs(r), (k, g, r)
        d = np.abs(ctx.get_params() - A.flatten(p))
        assert float((d > 1e-2 * cfg.eta).mean()) <= 1e-3
    finally:
        ctx.close()


# ------------------------------------------------------------------ 6. evaluation is untouched
def test_evaluation_calls_never_corrupt():
    from vaeb_amd import _lib
    c = denoise_case("A_gauss_bin_mask")
    B = len(c.idx)
    res = []
    for corruption in ("none", "mask"):
        ctx = loaded(c.cfg, c.X, c.params, c.acc, B, "gauss", corruption)
        try:
            ctx.set_eps_mode(_lib.EPS_PHILOX, SEED)
            ctx.set_step(STEP)
            if corruption != "none":
                ctx.set_corruption_noise(_lib.EPS_PHILOX, COR_SEED)
                ctx.set_corruption_level(0.5)
            before = state(ctx)
            x = c.X[:2 * B + 5]
            mu, lv, z = ctx.encode_dist(x)
            ll, ll_rows = ctx.marginal_ll(x, 3, rows=True)
            se, se_rows = ctx.sq_error(x, rows=True)
            res.append([ctx.reconstruct(x), ctx.encode(x), mu, lv, z, np.float64(ctx.elbo(x)), np.float64(ll), ll_rows,
                        np.float64(se), se_rows])
            after = state(ctx)
            assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
            assert ctx.get_step() == STEP
        finally:
            ctx.close()
    for k, (clean, cor) in enumerate(zip(*res)):
        assert np.array_equal(clean, cor), k


# ------------------------------------------------------------------ 7. errors
def test_denoise_argument_and_state_errors():
    from vaeb_amd import _lib
    cfg = A.AEConfig(Dobs=24, Denc=(12,), Dz=3, Ddec=(12,), otype="binary")
    X = data_for(cfg, 20)
    params = A.init_params(cfg)
    idx = np.arange(5, dtype=np.int32)
    nc = loaded(cfg, X, params, None, 8, "point")
    try:
        before = state(nc)
        calls = [lambda: nc.set_corruption_level(0.1), lambda: nc.get_corruption_level(),
                 lambda: nc.set_corruption_noise(_lib.EPS_HOST), lambda: nc.push_corruption(np.zeros((5, 24), np.float32)),
                 lambda: nc.corrupt(idx), lambda: nc.set_step(1), lambda: nc.get_step()]
        for call in calls:
            with pytest.raises(_lib.VaebError, match=r"error -1\b"):
                call()
        after = state(nc)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    finally:
        nc.close()
    cc = loaded(cfg, X, params, None, 8, "point", "mask")
    gc = loaded(cfg, X, params, None, 8, "point", "gauss")
    try:
        cc.set_corruption_level(0.25)
        for bad in (-0.1, 1.5, float("nan")):
            with pytest.raises(_lib.VaebError, match=r"error -1\b"):
                cc.set_corruption_level(bad)
            assert cc.get_corruption_level() == 0.25
        gc.set_corruption_level(1.5)                     # the additive kind: any finite level >= 0
        for bad in (-0.1, float("inf"), float("nan")):
            with pytest.raises(_lib.VaebError, match=r"error -1\b"):
                gc.set_corruption_level(bad)
            assert gc.get_corruption_level() == 1.5
        with pytest.raises(_lib.VaebError, match=r"error -1\b"):
            cc.set_corruption_noise(2)
        cc.set_step(7)
        assert cc.get_step() == 7
        cc.set_corruption_noise(_lib.EPS_HOST)
        cc.push_corruption(np.full((4, 24), 0.5, np.float32))
        before = state(cc)
        for call in (lambda: cc.train(idx), lambda: cc.corrupt(idx)):
            with pytest.raises(_lib.VaebError, match=r"error -3\b"):
                call()
        after = state(cc)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and cc.get_step() == 7
        cc.push_corruption(np.full((5, 24), 0.5, np.float32))
        assert np.isfinite(cc.train(idx)) and cc.get_step() == 8
        assert not np.array_equal(cc.get_params(), before[0])
    finally:
        cc.close()
        gc.close()


# ------------------------------------------------------------------ 8. the Python mirror
def test_construct_vanilla_ae_with_a_noise_schedule():
    from vaeb_amd import ae
    cfg = A.AEConfig(Dobs=784, Denc=(64,), Dz=8, Ddec=(64,), otype="binary")
    X = data_for(cfg, 1000, seed=3)
    np.random.seed(15485863)
    plain = ae.ConstructVanillaAE(X, Denc=[64], Dz=8, Ddec=[64], corruption=None)
    theta0 = [t.get_value() for t in plain[4]]
    plain[0].ctx.close()
    ref0 = A.init_params(cfg, seed=15485863)
    assert all(np.array_equal(t, r) for t, r in zip(theta0, ref0))
    np.random.seed(15485863)
    train, reconstruct, encode, decode, theta = ae.ConstructVanillaAE(X, Denc=[64], Dz=8, Ddec=[64],
                                                                     corruption=("mask", 0.3), corruption_seed=COR_SEED)
    try:
        assert all(np.array_equal(t.get_value(), r) for t, r in zip(theta, ref0))
        assert train.noise == np.float32(0.3)
        xt = train.corrupt(np.arange(10))
        assert xt.shape == (10, 784) and ((xt == 0) | (xt == X[:10])).all() and (xt != X[:10]).any()
        sched = ae.noise_schedule([0.3, 0.15, 0.0], 3)
        vals = ae.train_epochs(train, X.shape[0], 3, verbose=False, noise=sched)
        assert len(vals) == 30 and np.isfinite(vals).all()
        assert np.mean(vals[20:]) < np.mean(vals[:10])
        assert train.noise == 0.0
        assert np.isfinite(train.mse(X))
        assert np.isfinite(train(np.arange(50)))
        assert reconstruct(xt).shape == (10, 784)        # denoising: the corrupted rows go to reconstruct
    finally:
        train.ctx.close()


# ------------------------------------------------------------------ 9. the driver with --corruption
def test_driver_with_corruption_reports_the_clean_test_error(tmp_path):
    """AE_MSE.res of a denoising run is the clean test-set MSE of the model it trained, and the schedule's
    last stage is the level the run ends at."""
    import os
    from vaeb_amd import ae, synthetic, vanilla_ae
    frey, mnist = synthetic.frey_like(340), synthetic.mnist_like(340)
    data = {"continuous": (frey[:300], frey[300:]), "discrete": (mnist[:300], mnist[300:])}
    seen = {}
    report = vanilla_ae._report

    def spy(data_type, Dz, reconstruct, Xte, out_dir):
        seen[data_type] = (reconstruct.train.noise, ae.mse(Xte, reconstruct(Xte)))
        return report(data_type, Dz, reconstruct, Xte, out_dir)

    vanilla_ae._report = spy
    try:
        res = vanilla_ae.main(["--out", str(tmp_path), "--epochs", "4", "--dz", "2", "--hidden", "16",
                               "--corruption", "saltpepper", "--noise", "0.4,0.1"], data=data)
    finally:
        vanilla_ae._report = report
    lines = open(os.path.join(tmp_path, "AE_MSE.res")).read().split("\n")
    assert lines[0] == "data_type,latent_size,MSE" and len(lines) == 4
    for kind in ("continuous", "discrete"):
        noise, host_mse = seen[kind]
        assert noise == np.float32(0.1)
        assert abs(res[(kind, 2)] - host_mse) <= 1e-5 * host_mse
