"""vaeb_marginal_ll / vaeb_marginal_ll_resident / vaeb_encode (include/vaeb_hip.h) against the
float64 oracle: the K-sample importance-weighted bound

    IW_K(x) = logsumexp_k [log p(x | z_k) + log p(z_k) - log q(z_k | x)] - log K

with the reference formed here from oracle.forward_backward's per-(sample, row) terms (LA
estimator: logp_rows + la_rows) and a max-subtracted logsumexp.

Tolerance: 1e-4 relative per row and on the sum, the project's ELBO tolerance
(tests/test_gpu_step.py): a row value is the same kind of quantity, and the float32 NumPy
restatement of these cases is within 2e-7 of float64.  Every case asserts on the reference
itself that logsumexp and the plain mean of log w differ by >= 20x the tolerance (median over
the rows), so an implementation that averaged would fail; mnist20's largest log w is below
-600, so one without the max subtraction returns -inf.

Parameters: every tensor 0.1 * default_rng(3).standard_normal(shape) as float32; eps from the
same generator after them; data from the oracle's synthetic sets with seed 5."""
import functools
import re

import numpy as np
import pytest

from oracle import vaeb_oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-4
CASES = {
    # name: (D, H, Z, continuous, n, K)
    "mnist20": (784, 500, 20, False, 37, 5),
    "frey2_gauss": (560, 200, 2, True, 37, 7),
    "odd_shapes": (37, 19, 3, False, 13, 3),
    "wide_latent": (66, 48, 36, False, 30, 4),     # Z > 32: the non-fused heads
    "gauss_odd_D": (45, 30, 6, True, 17, 64),      # K = 64 planes against a 48-row capacity
}


def make_case(D, H, Z, continuous, n, K):
    """(cfg, float32 params, x, eps [K, n, Z], out) with out the float64 oracle's LA forward."""
    cfg = O.Config(D=D, H=H, Z=Z, continuous=continuous, estimator="LA")
    rng = np.random.default_rng(3)
    params = [(0.1 * rng.standard_normal(s)).astype(np.float32) for _, s in O.param_shapes(cfg)]
    eps = rng.standard_normal((K, n, Z)).astype(np.float32)
    x = O.synthetic_frey(n=n, D=D, seed=5) if continuous else O.synthetic_mnist(n=n, D=D, seed=5)
    p64 = [p.astype(np.float64) for p in params]
    out = O.forward_backward(p64, x.astype(np.float64), eps.astype(np.float64), cfg, need_grad=False)
    return cfg, params, x, eps, out


def iw_reference(out, K):
    lw = out["logp_rows"] + out["la_rows"]          # [K, n]
    mx = lw.max(axis=0)
    return lw, mx + np.log(np.exp(lw - mx).sum(axis=0)) - np.log(K)


@functools.lru_cache(maxsize=None)
def case(name):
    D, H, Z, continuous, n, K = CASES[name]
    cfg, params, x, eps, out = make_case(D, H, Z, continuous, n, K)
    lw, ref = iw_reference(out, K)
    for a in (x, eps, ref, lw):
        a.setflags(write=False)
    return cfg, params, x, eps, out, lw, ref


@functools.lru_cache(maxsize=None)
def mnist50():
    """mnist20's model on n = 50 rows, K = 3 (chunking / resident tests)."""
    cfg, params, x, eps, out = make_case(784, 500, 20, False, 50, 3)
    _, ref = iw_reference(out, 3)
    return cfg, params, x, eps, ref


def make_ctx(cfg, params, B=16, host_eps=None, seed=7, **kw):
    from vaeb_amd import _lib
    ctx = _lib.Context(cfg.D, cfg.H, cfg.Z, B, decoder=_lib.DEC_GAUSSIAN if cfg.continuous else _lib.DEC_BERNOULLI,
                       **kw)
    ctx.set_params(O.flatten(params))
    if host_eps is not None:
        ctx.set_eps_mode(_lib.EPS_HOST)
        ctx.push_eps(host_eps)
    else:
        ctx.set_eps_mode(_lib.EPS_PHILOX, seed)
    return ctx


def stacked(eps, L=1):
    """eps [K, n, Z] as the pushed buffer [L, K * n, Z]: sample-major rows in plane 0."""
    K, n, Z = eps.shape
    out = np.zeros((L, K * n, Z), np.float32)
    out[0] = eps.reshape(K * n, Z)
    return out


def assert_matches(total, rows, ref, what):
    err = np.abs(rows - ref) / np.abs(ref)
    serr = abs(total - ref.sum()) / abs(ref.sum())
    print(f"{what}: max row rel err {err.max():.3e}, sum rel err {serr:.3e}")
    assert np.all(np.isfinite(rows)), what
    assert np.all(np.abs(rows - ref) <= RTOL * np.abs(ref)), (what, err.max())
    assert abs(total - ref.sum()) <= RTOL * abs(ref.sum()), (what, serr)


@pytest.mark.parametrize("name", list(CASES))
def test_rows_match_oracle_host_eps(name):
    cfg, params, x, eps, out, lw, ref = case(name)
    K = eps.shape[0]
    # the reference tells logsumexp from a mean (and, for mnist20, needs the max subtraction)
    gap = np.median(np.abs(ref - lw.mean(axis=0)) / np.abs(ref))
    print(f"{name}: median (IW - mean log w) / |IW| = {gap:.3e}, max log w = {lw.max():.1f}")
    assert gap >= 20 * RTOL
    if name == "mnist20":
        assert lw.max() < -600
    ctx = make_ctx(cfg, params, host_eps=stacked(eps), max_eval_rows=48)
    total, rows = ctx.marginal_ll(x, K, rows=True)
    ctx.close()
    assert_matches(total, rows, ref, name)


def test_context_L_estimator_objective_do_not_enter():
    """An LA, L = 3, mean-objective context (three planes of capacity: all K samples in one
    stack) gives the same rows as the oracle."""
    from vaeb_amd import _lib
    cfg, params, x, eps, out, lw, ref = case("odd_shapes")
    ctx = make_ctx(cfg, params, host_eps=stacked(eps, L=3), L=3, estimator=_lib.EST_LA,
                   objective=_lib.OBJ_MEAN_MAP, max_eval_rows=1000)
    total, rows = ctx.marginal_ll(x, eps.shape[0], rows=True)
    ctx.close()
    assert_matches(total, rows, ref, "odd_shapes L=3 LA mean_map")


def test_chunking_and_noise_keying():
    cfg, params, x, eps, ref = mnist50()
    # host eps, four chunks (the last with 2 rows)
    ctx = make_ctx(cfg, params, host_eps=stacked(eps), max_eval_rows=16)
    total, rows = ctx.marginal_ll(x, 3, rows=True)
    ctx.close()
    assert_matches(total, rows, ref, "mnist n=50 K=3 in chunks of 16")
    # Philox: the draws are keyed by the global row and the sample, not by the chunk
    got = []
    for mer in (16, 1000):
        ctx = make_ctx(cfg, params, seed=7, max_eval_rows=mer)
        got.append(ctx.marginal_ll(x, 3, rows=True))
        ctx.close()
    (s16, r16), (s1000, r1000) = got
    d = np.abs(r16 - r1000) / np.abs(r1000)
    print(f"philox chunk 16 vs 1000: max row rel diff {d.max():.3e}")
    assert np.all(np.isfinite(r16)) and np.all(d <= 1e-6)
    assert abs(s16 - s1000) <= 1e-6 * abs(s1000)


def test_one_sample_equals_la_validate():
    """K = 1 is the one-sample LA estimate: the same device partials as validate on an LA,
    L = 1 context, reduced differently."""
    from vaeb_amd import _lib
    cfg, params, x, eps, out, lw, ref = case("mnist20")
    ctx = make_ctx(cfg, params, host_eps=eps[:1], estimator=_lib.EST_LA, max_eval_rows=48)
    v = ctx.validate(x)
    m = ctx.marginal_ll(x, 1)
    ctx.close()
    print(f"K=1 {m!r} vs LA validate {v!r}: rel diff {abs(m - v) / abs(v):.3e}")
    assert abs(m - v) <= 1e-5 * abs(v)
    assert abs(m - lw[0].sum()) <= RTOL * abs(lw[0].sum())


def test_training_state_is_untouched():
    cfg, params, x, eps, out, lw, ref = case("mnist20")
    xt = O.synthetic_mnist(n=64, seed=6)
    runs = []
    for probe in (True, False):
        ctx = make_ctx(cfg, params, B=16, seed=7, max_eval_rows=48)
        ctx.set_data(xt)
        e = [ctx.update(0)]
        if probe:
            a = ctx.marginal_ll(x, 3, rows=True)
            b = ctx.marginal_ll(x, 3, rows=True)
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.all(np.isfinite(a[1]))
        e.append(ctx.update(1))
        runs.append((e, ctx.get_step(), ctx.get_params(), ctx.get_adagrad_state()))
        e.append(ctx.update(2))
        ctx.close()
    (e0, s0, p0, a0), (e1, s1, p1, a1) = runs
    assert e0 == e1 and s0 == s1
    assert np.array_equal(p0, p1) and np.array_equal(a0, a1)


def test_resident_equals_host_rows():
    cfg, params, x, eps, ref = mnist50()
    ctx = make_ctx(cfg, params, seed=7, max_eval_rows=16)
    host = ctx.marginal_ll(x, 3)
    ctx.set_valid_data(x)
    res = ctx.marginal_ll_resident(3)
    ctx.close()
    print(f"resident {res!r} vs host rows {host!r}")
    assert np.isfinite(res) and abs(res - host) <= 1e-6 * abs(host)


@pytest.mark.parametrize("name", ["mnist20", "frey2_gauss"])
def test_encode_matches_oracle(name):
    cfg, params, x, eps, out, lw, ref = case(name)
    ctx = make_ctx(cfg, params, max_eval_rows=16)
    mu, lv = ctx.encode(x)
    mu_only, none = ctx.encode(x, log_var=False)
    none2, lv_only = ctx.encode(x, mu=False)
    ctx.close()
    print(f"{name}: max |mu - ref| {np.abs(mu - out['mu']).max():.3e}, max |lv - ref| {np.abs(lv - out['lv']).max():.3e}")
    assert np.abs(mu - out["mu"]).max() <= 1e-5 and np.abs(lv - out["lv"]).max() <= 1e-5
    assert none is None and none2 is None
    assert np.array_equal(mu_only, mu) and np.array_equal(lv_only, lv)


def test_errors_leave_a_working_context():
    from vaeb_amd import _lib
    cfg, params, x, eps, out, lw, ref = case("odd_shapes")
    K, n, Z = eps.shape

    def rc_of(fn, *a):
        with pytest.raises(_lib.VaebError) as ei:
            fn(*a)
        return int(re.search(r"error (-?\d+)", str(ei.value)).group(1)), str(ei.value)

    ctx = make_ctx(cfg, params, max_eval_rows=48)
    assert rc_of(ctx.marginal_ll, x, 0)[0] == -1                  # VAEB_ERR_ARG
    assert rc_of(ctx.marginal_ll, x, (1 << 20) + 1)[0] == -1
    assert rc_of(ctx.marginal_ll_resident, 3)[0] == -3            # VAEB_ERR_STATE: no resident set
    ctx.set_eps_mode(_lib.EPS_HOST)
    ctx.push_eps(stacked(eps)[:, :n * K - 1])
    assert rc_of(ctx.marginal_ll, x, K)[0] == -3                  # eps for n * K - 1 rows
    ctx.set_eps_mode(_lib.EPS_PHILOX, 7)
    ctx.set_data(O.synthetic_mnist(n=32, D=cfg.D, seed=6))
    assert np.isfinite(ctx.update(1))                             # the context still trains
    total, rows = ctx.marginal_ll(x, K, rows=True)                # and still serves the call
    assert np.all(np.isfinite(rows)) and np.isfinite(total)
    ctx.close()


def test_errors_bf16_context_and_training_goes_on():
    from vaeb_amd import _lib
    D, H, Z, B = 64, 32, 8, 16
    x = O.synthetic_mnist(n=2 * B, D=D, seed=5)
    ctx = _lib.Context(D, H, Z, B, dtype=_lib.DTYPE_BF16, max_eval_rows=32)
    ctx.set_params(O.flatten(O.init_params(O.Config(D=D, H=H, Z=Z))))
    ctx.set_data(x)
    ctx.set_valid_data(x)
    for fn, a in ((ctx.marginal_ll, (x, 3)), (ctx.marginal_ll_resident, (3,)), (ctx.encode, (x,))):
        with pytest.raises(_lib.VaebError, match=r"error -1: .*served by fp32 contexts"):
            fn(*a)
    assert np.isfinite(ctx.update(0))
    ctx.close()
