"""Host checks of the layer-stack engine's importance-weighted bound (no GPU): the NumPy oracle
the GPU tests compare against (tests/vae_stack_iw_oracle.py) is pinned to independently written
formulas, the GPU cases are shown to sit far inside their tolerance in float32, to tell the
bound from the mean of the log-weights and a mis-keyed noise site from the right one, and the
ABI addition is checked.

The GPU cases (tests/test_gpu_vae_stack_iw.py) are defined here so both files share them.
"""
import functools
import math
import os
import re

import numpy as np
import pytest

from oracle import ae_oracle as A
from oracle import philox
from tests import vae_stack_iw_oracle as W
from tests import vae_stack_oracle as V
from tests.test_gpu_ae import data_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the bound tests/test_gpu_marginal_ll.py uses for the same quantity: relative, per row and on the sum
RTOL = 1e-4

# name, AEConfig kwargs, n, K, max_batch on the GPU
IW_CASES = [
    ("bin_deep_odd", dict(Dobs=37, Denc=(29, 17), Dz=5, Ddec=(13, 21), otype="binary", s2=2.0), 23, 9, 64),
    ("cont_two_tiles", dict(Dobs=48, Denc=(20,), Dz=20, Ddec=(18, 11), otype="cont", act="sigmoid"), 30, 7, 30),
    ("relu_z16", dict(Dobs=64, Denc=(32,), Dz=16, Ddec=(32,), otype="binary", act="relu"), 32, 3, 100),
    ("mnist_like", dict(Dobs=784, Denc=(64,), Dz=8, Ddec=(64,), otype="binary"), 37, 64, 16),
]
IW_IDS = [c[0] for c in IW_CASES]
IW_BY_NAME = {c[0]: c for c in IW_CASES}

SEED = 0x1234567_89ABCDEF
STEP = (1 << 32) + 12345
PHILOX_K = 3   # with a large K the "stream k" mistake changes one of K samples and logsumexp hides it


@functools.lru_cache(maxsize=None)
def iw_setup(name):
    """cfg, X, params, eps [K, n, Dz] of one case.  Shared (cached): do not write to the arrays."""
    _, kw, n, K, _ = IW_BY_NAME[name]
    cfg = A.AEConfig(**kw)
    rng = np.random.default_rng(3)
    params = [(0.1 * rng.standard_normal(s)).astype(np.float32) for _, s in V.param_shapes(cfg)]
    eps = rng.standard_normal((K, n, cfg.Dz)).astype(np.float32)
    X = data_for(cfg, n, seed=5)
    for a in params + [eps, X]:
        a.setflags(write=False)
    return cfg, X, tuple(params), eps


def p64(params):
    return [p.astype(np.float64) for p in params]


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 oracle of one case with its host eps: dict(lw [K, n], rows [n], sum, ...)."""
    cfg, X, params, eps = iw_setup(name)
    out = W.log_weights(p64(params), X.astype(np.float64), eps.astype(np.float64), cfg)
    out["rows"] = W.iw_from_lw(out["lw"])
    out["sum"] = float(out["rows"].sum())
    return out


def philox_eps(n, Dz, K=PHILOX_K, seed=SEED, step=STEP):
    """The device's draws: sample k from evaluation stream k + 1, keyed by the row in the call's x."""
    return np.stack([philox.eval_eps(seed, step, n, Dz, k + 1) for k in range(K)])


@functools.lru_cache(maxsize=None)
def philox_reference(name):
    cfg, X, params, _ = iw_setup(name)
    return W.iw_rows(p64(params), X.astype(np.float64), philox_eps(X.shape[0], cfg.Dz), cfg)


# ------------------------------------------------------------------ 1. the helper
@pytest.mark.parametrize("name", IW_IDS)
def test_helper_matches_independent_formulas(name):
    cfg, X, params, eps = iw_setup(name)
    ref = reference(name)
    for k, out in enumerate(ref["outs"]):
        assert abs(ref["ll"][k].sum() - out["loglik"]) <= 1e-12 * abs(out["loglik"])
        z, mu, lv = out["z"], out["mu"], out["lv"]
        log_prior = -0.5 * (math.log(2 * math.pi) + z * z).sum(1)
        log_q = -0.5 * (math.log(2 * math.pi) + lv + (z - mu) ** 2 / np.exp(lv)).sum(1)
        want = log_prior - log_q
        assert np.abs(ref["lat"][k] - want).max() <= 1e-12 * np.abs(want).max()
    K = ref["lw"].shape[0]
    direct = np.log(np.exp(ref["lw"] - ref["lw"].max()).mean(0)) + ref["lw"].max()   # one global shift
    assert np.abs(ref["rows"] - direct).max() <= 1e-12 * np.abs(direct).max()
    assert K == IW_BY_NAME[name][3]


# ------------------------------------------------------------------ 2. float32 headroom
@pytest.mark.parametrize("name", IW_IDS)
def test_float32_oracle_run_sits_inside_rtol(name):
    cfg, X, params, eps = iw_setup(name)
    ref = reference(name)["rows"]
    got = W.iw_rows(list(params), X, eps, cfg)
    assert got.dtype == np.float32
    err = np.abs(got - ref) / np.abs(ref)
    print(f"{name}: float32 restatement max rel {err.max():.2e} / {RTOL:.0e}")
    assert err.max() <= RTOL


# ------------------------------------------------------------------ 3. discrimination
@pytest.mark.parametrize("name", IW_IDS)
def test_bound_is_told_from_the_mean_of_the_log_weights(name):
    ref = reference(name)
    gap = np.abs(ref["rows"] - ref["lw"].mean(0)) / np.abs(ref["rows"])
    print(f"{name}: median |IW_K - mean_k log w| / |IW_K| = {np.median(gap):.2e}")
    assert np.median(gap) >= 20 * RTOL


def test_mnist_like_needs_the_max_subtraction():
    """exp(log w) underflows in float32 (and in float64): a fold without the max returns -inf."""
    lw = reference("mnist_like")["lw"]
    print(f"mnist_like: max log w = {lw.max():.1f}")
    assert lw.max() < -500
    with np.errstate(divide="ignore"):
        assert np.isneginf(np.log(np.exp(lw.astype(np.float32)).sum(0))).all()


# ------------------------------------------------------------------ 4. Philox keying
def _mis_keyed(kind, n, Dz):
    j = np.arange(Dz, dtype=np.int64)[None, :]
    row = np.arange(n, dtype=np.int64)[:, None]
    K = PHILOX_K
    if kind == "stream_k":
        return np.stack([philox.eval_eps(SEED, STEP, n, Dz, k) for k in range(K)])
    if kind == "row_mod_16":
        return np.stack([philox.latent_normal(SEED, row % 16, j, STEP, 1 | ((k + 1) << 1)) for k in range(K)])
    if kind == "stacked_row":
        return np.stack([philox.latent_normal(SEED, k * n + row, j, STEP, 1 | ((k + 1) << 1)) for k in range(K)])
    if kind == "train_domain":
        return np.stack([philox.latent_normal(SEED, row, j, STEP, (k + 1) << 1) for k in range(K)])
    if kind == "next_step":
        return philox_eps(n, Dz, step=STEP + 1)
    if kind == "one_stream":
        return np.stack([philox.eval_eps(SEED, STEP, n, Dz, 1)] * K)
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["stream_k", "row_mod_16", "stacked_row", "train_domain", "next_step", "one_stream"])
@pytest.mark.parametrize("name", IW_IDS)
def test_philox_case_tells_a_mis_keyed_site_apart(name, kind):
    cfg, X, params, _ = iw_setup(name)
    n = X.shape[0]
    assert n > 16
    ref = philox_reference(name)
    wrong = W.iw_rows(p64(params), X.astype(np.float64), _mis_keyed(kind, n, cfg.Dz), cfg)
    off = (np.abs(wrong - ref) / np.abs(ref)).max()
    print(f"{name} {kind}: largest per-row relative difference {off / RTOL:.0f} x RTOL")
    assert off >= 100 * RTOL


# ------------------------------------------------------------------ 5. surface
def test_header_and_binding_declare_the_call():
    from vaeb_amd import _lib
    src = open(os.path.join(ROOT, "include", "vaeb_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+vaeb_ae_marginal_ll\s*\(([^)]*)\)\s*;", src)
    assert m and len(m.group(1).split(",")) == 6
    assert "vaeb_ae_marginal_ll" in _lib.EXPORTS
    assert hasattr(_lib.AEContext, "marginal_ll")
