"""The layer-stack engine's importance-weighted bound (vaeb_ae_marginal_ll, AEContext.marginal_ll,
ConstructVAE's train.marginal_ll) against the float64 NumPy oracle (tests/vae_stack_iw_oracle.py)
on identical theta / rows / eps.

Tolerance: RTOL = 1e-4 relative, per row and on the sum, the bound tests/test_gpu_marginal_ll.py
uses for the same quantity.  The cases are shared with tests/test_vae_stack_iw_host.py, which
shows that they sit far inside it in float32, tell the bound from the mean of the log-weights
and tell a mis-keyed noise site apart.  Each test prints its figures before it asserts.
"""
import numpy as np
import pytest

from oracle import ae_oracle as A
from tests import vae_stack_oracle as V
from tests.test_gpu_ae import data_for
from tests.test_gpu_vae_stack import loaded, make_ctx
from tests.test_vae_stack_iw_host import (IW_BY_NAME, IW_CASES, IW_IDS, PHILOX_K, RTOL, SEED, STEP, iw_setup,
                                          philox_reference, reference)

pytestmark = pytest.mark.gpu


def iw_ctx(name, max_batch, params=None):
    cfg, X, p, eps = iw_setup(name)
    return loaded(cfg, X, list(p if params is None else params), None, max_batch)


def rel_errors(tag, rows, total, ref_rows, ref_sum=None):
    """Largest per-row and the sum's relative error, printed (the figures DESIGN records)."""
    ref_sum = float(ref_rows.sum()) if ref_sum is None else ref_sum
    e_row = float((np.abs(rows - ref_rows) / np.abs(ref_rows)).max())
    e_sum = abs(total - ref_sum) / abs(ref_sum)
    print(f"[iw] {tag}: max row rel {e_row:.2e}, sum rel {e_sum:.2e} (RTOL {RTOL:.0e})")
    return e_row, e_sum


# ------------------------------------------------------------------ 1. rows against the oracle
@pytest.mark.parametrize("name", IW_IDS)
def test_iw_rows_match_the_oracle_host_eps(name):
    from vaeb_amd import _lib
    cfg, X, params, eps = iw_setup(name)
    _, _, n, K, mb = IW_BY_NAME[name]
    ref = reference(name)
    ctx = iw_ctx(name, mb)
    ctx.set_eps_mode(_lib.EPS_HOST)
    ctx.push_eps(eps.reshape(K * n, cfg.Dz))
    total, rows = ctx.marginal_ll(X, K, rows=True)
    ctx.close()
    e_row, e_sum = rel_errors(f"host eps {name} max_batch {mb}", rows, total, ref["rows"], ref["sum"])
    assert rows.shape == (n,) and np.isfinite(rows).all() and np.isfinite(total)
    assert e_row <= RTOL and e_sum <= RTOL


# ------------------------------------------------------------------ 2. Philox
@pytest.mark.parametrize("name", ["bin_deep_odd", "mnist_like"])
def test_iw_philox_streams_match_the_host_oracle(name):
    from vaeb_amd import _lib
    cfg, X, params, _ = iw_setup(name)
    ref = philox_reference(name)
    ctx = iw_ctx(name, 16)
    ctx.set_eps_mode(_lib.EPS_PHILOX, SEED)
    ctx.set_step(STEP)
    total, rows = ctx.marginal_ll(X, PHILOX_K, rows=True)
    step_after = ctx.get_step()
    ctx.close()
    e_row, e_sum = rel_errors(f"philox {name} K {PHILOX_K} max_batch 16", rows, total, ref)
    assert np.isfinite(rows).all()
    assert e_row <= RTOL and e_sum <= RTOL
    assert step_after == STEP


# ------------------------------------------------------------------ 3. chunking / stacking invariance
def test_iw_row_values_do_not_depend_on_max_batch():
    from vaeb_amd import _lib
    cfg, X, params, _ = iw_setup("mnist_like")
    got = []
    for mb in (16, 1000):   # 3 chunks of 1 plane per pass; 1 chunk, all planes in one pass
        ctx = iw_ctx("mnist_like", mb)
        ctx.set_eps_mode(_lib.EPS_PHILOX, SEED)
        ctx.set_step(STEP)
        got.append(ctx.marginal_ll(X, PHILOX_K, rows=True))
        ctx.close()
    (s_a, r_a), (s_b, r_b) = got
    d = float((np.abs(r_a - r_b) / np.abs(r_b)).max())
    print(f"[iw] max_batch 16 vs 1000: rows bitwise equal {np.array_equal(r_a, r_b)}, max rel {d:.2e}; "
          f"sums {s_a!r} {s_b!r}")
    assert d <= 1e-6
    assert abs(s_a - s_b) <= 1e-6 * abs(s_b)


# ------------------------------------------------------------------ 4. degenerate identity
def test_iw_one_sample_zero_noise_zero_lv_head_is_the_elbo():
    """eps = 0 and lv = 0: log w = loglik(mu) - 1/2 sum mu^2, and so is loglik - KL."""
    from vaeb_amd import _lib
    cfg, X, params, _ = iw_setup("bin_deep_odd")
    params = [np.zeros_like(p) if nm in V.LV_NAMES else p for nm, p in zip(V.names(cfg), params)]
    ctx = iw_ctx("bin_deep_odd", 16, params)
    ctx.set_eps_mode(_lib.EPS_HOST)
    ctx.push_eps(np.zeros((X.shape[0], cfg.Dz), np.float32))
    iw = ctx.marginal_ll(X, 1)
    elbo = ctx.elbo(X)
    ctx.close()
    print(f"[iw] K = 1, zero noise, zero lv head: marginal_ll {iw!r} elbo {elbo!r} rel {abs(iw - elbo) / abs(elbo):.2e}")
    assert np.isfinite(iw) and abs(iw - elbo) <= 1e-5 * abs(elbo)


# ------------------------------------------------------------------ 5. state untouched
def test_iw_changes_no_training_state():
    from vaeb_amd import _lib
    cfg, X, params, _ = iw_setup("bin_deep_odd")
    idx = [np.arange(0, 12, dtype=np.int32), np.arange(5, 23, dtype=np.int32)]
    state, probes = [], []
    for probe in (True, False):
        ctx = iw_ctx("bin_deep_odd", 64)
        ctx.set_eps_mode(_lib.EPS_PHILOX, SEED)
        ctx.set_step(STEP)
        vals = [ctx.train(idx[0])]
        if probe:
            probes = [ctx.marginal_ll(X, 5, rows=True) for _ in range(2)]
        vals.append(ctx.train(idx[1]))
        state.append((vals, ctx.get_params(), ctx.get_adagrad_state(), ctx.get_step()))
        ctx.close()
    (s0, r0), (s1, r1) = probes
    assert s0 == s1 and np.array_equal(r0, r1) and np.isfinite(r0).all()
    (va, pa, aa, ta), (vb, pb, ab, tb) = state
    assert va == vb and ta == tb == STEP + 2
    assert np.array_equal(pa, pb) and np.array_equal(aa, ab)


def test_iw_host_eps_push_stays_and_train_still_needs_its_own():
    from vaeb_amd import _lib
    cfg, X, params, eps = iw_setup("bin_deep_odd")
    _, _, n, K, _ = IW_BY_NAME["bin_deep_odd"]
    idx = np.arange(4, 15, dtype=np.int32)
    eps_t = np.random.default_rng(4).standard_normal((2, idx.size, cfg.Dz)).astype(np.float32)
    state = []
    for probe in (True, False):
        ctx = iw_ctx("bin_deep_odd", 64)
        ctx.set_eps_mode(_lib.EPS_HOST)
        ctx.push_eps(eps_t[0])
        vals = [ctx.train(idx)]
        if probe:
            ctx.push_eps(eps.reshape(K * n, cfg.Dz))
            a = ctx.marginal_ll(X, K, rows=True)
            b = ctx.marginal_ll(X, K, rows=True)   # the push is still there
            assert a[0] == b[0] and np.array_equal(a[1], b[1])
            with pytest.raises(_lib.VaebError, match=r"error -3\b"):
                ctx.train(idx)                     # ... and is no push for 11 rows
        ctx.push_eps(eps_t[1])
        vals.append(ctx.train(idx))
        state.append((vals, ctx.get_params(), ctx.get_adagrad_state()))
        ctx.close()
    (va, pa, aa), (vb, pb, ab) = state
    assert va == vb and np.array_equal(pa, pb) and np.array_equal(aa, ab)


# ------------------------------------------------------------------ 6. NaN poisoning
def test_iw_non_finite_log_weight_poisons_its_row_only():
    from vaeb_amd import _lib
    name, bad = "relu_z16", 7
    cfg, X, params, eps = iw_setup(name)
    _, _, n, K, mb = IW_BY_NAME[name]
    ref = reference(name)["rows"]
    Xb = X.copy()
    Xb[bad] = 3e38
    ctx = iw_ctx(name, mb)
    ctx.set_eps_mode(_lib.EPS_HOST)
    ctx.push_eps(eps.reshape(K * n, cfg.Dz))
    total, rows = ctx.marginal_ll(Xb, K, rows=True)
    ctx.close()
    keep = np.arange(n) != bad
    e_row = float((np.abs(rows[keep] - ref[keep]) / np.abs(ref[keep])).max())
    print(f"[iw] poisoned row {bad}: value {rows[bad]!r}, sum {total!r}; other rows max rel {e_row:.2e}")
    assert np.isnan(rows[bad]) and np.isnan(total)
    assert np.isfinite(rows[keep]).all() and e_row <= RTOL


# ------------------------------------------------------------------ 7. errors
def test_iw_argument_and_state_errors():
    from vaeb_amd import _lib
    cfg, X, params, eps = iw_setup("bin_deep_odd")
    _, _, n, K, _ = IW_BY_NAME["bin_deep_odd"]
    pc = make_ctx(cfg, 8, latent="point")
    with pytest.raises(_lib.VaebError, match=r"error -1\b"):
        pc.marginal_ll(X, 2)
    pc.close()
    ctx = iw_ctx("bin_deep_odd", 16)
    for bad_k in (0, (1 << 20) + 1):
        with pytest.raises(_lib.VaebError, match=r"error -1\b"):
            ctx.marginal_ll(X, bad_k)
    ctx.set_eps_mode(_lib.EPS_HOST)
    ctx.push_eps(eps.reshape(K * n, cfg.Dz)[:-1])
    with pytest.raises(_lib.VaebError, match=r"error -3\b"):
        ctx.marginal_ll(X, K)
    ctx.push_eps(eps[0, :6])
    assert np.isfinite(ctx.train(np.arange(6, dtype=np.int32)))
    ctx.push_eps(eps.reshape(K * n, cfg.Dz))
    total, rows = ctx.marginal_ll(X, K, rows=True)
    ctx.close()
    assert np.isfinite(total) and np.isfinite(rows).all()


# ------------------------------------------------------------------ 8. ConstructVAE
def test_construct_vae_marginal_ll():
    from vaeb_amd import ae
    cfg = A.AEConfig(Dobs=784, Denc=(64,), Dz=8, Ddec=(64,), otype="binary", act="relu")
    X = data_for(cfg, 1000, seed=3)
    np.random.seed(15485863)
    train, *_ = ae.ConstructVAE(X, Denc=[64], Dz=8, Ddec=[64], f="relu")
    ae.train_epochs(train, X.shape[0], 3, verbose=False)
    step = train.ctx.get_step()
    total, rows = train.marginal_ll(X[:50], 8, rows=True)
    print(f"[iw] ConstructVAE: IW_8 sum over 50 rows {total!r}, elbo {train.elbo(X[:50])!r}")
    assert np.isfinite(total) and rows.shape == (50,) and np.isfinite(rows).all()
    assert abs(total - float(rows.astype(np.float64).sum())) <= 1e-6 * abs(total)
    assert train.marginal_ll(X[:50], 8) == total
    assert train.ctx.get_step() == step
