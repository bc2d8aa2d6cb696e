"""Host checks of the layer-stack engine's Gaussian latent (no GPU): the NumPy oracle the GPU
tests compare against (tests/vae_stack_oracle.py) is pinned to float64 torch autograd and to the
point-latent oracle, the GPU tests' inputs are shown to sit inside their tolerances in float32
and to tell a mis-keyed noise site apart, and the ABI additions are checked.

The GPU cases (tests/test_gpu_vae_stack.py) are defined here so both files share them.
"""
import ctypes
import os

import numpy as np
import pytest

from oracle import ae_oracle as A
from oracle import philox
from tests import vae_stack_oracle as V
from tests.test_gpu_ae import check_theta, data_for

# tolerances of tests/test_gpu_ae.py, used by the GPU step tests
VALUE_RTOL = 2e-5
ACC_RTOL = 1e-4

# name, AEConfig kwargs, B, scale the latent heads (x30, bzlv = -1) so lv is not ~0 and z responds
STEP_CASES = [
    ("bin_deep_odd", dict(Dobs=37, Denc=(29, 17), Dz=5, Ddec=(13, 21), otype="binary", s2=2.0), 23, False),
    ("cont_two_tiles", dict(Dobs=48, Denc=(20,), Dz=20, Ddec=(18, 11), otype="cont", act="sigmoid"), 30, True),
    ("relu_z16", dict(Dobs=64, Denc=(32,), Dz=16, Ddec=(32,), otype="binary", act="relu"), 32, False),
    ("mnist_like", dict(Dobs=784, Denc=(64,), Dz=8, Ddec=(64,), otype="binary"), 50, True),
]
STEP_IDS = [c[0] for c in STEP_CASES]

# the Philox-mode train step: every parameter x30, seed and step above 2^32
PHILOX_KW = dict(Dobs=37, Denc=(29, 17), Dz=5, Ddec=(13, 21), otype="binary", s2=2.0)
PHILOX_B = 23
SEED = 0x1234567_89ABCDEF
STEP = (1 << 32) + 12345


def step_setup(kw, B, scale_heads):
    """cfg, Xtr, params, acc, idx, eps of one single-step case (the setup style of
    tests/test_gpu_ae.py: acc = 1e-4, a gathered idx)."""
    cfg = A.AEConfig(**kw)
    X = data_for(cfg, 4 * B)
    params = V.init_params(cfg)
    if scale_heads:
        p = dict(zip(V.names(cfg), params))
        p["Wzmu"] *= 30
        p["Wzlv"] *= 30
        p["bzlv"][:] = -1.0
    rng = np.random.default_rng(2)
    acc = [np.full(p.shape, 1e-4, np.float32) for p in params]
    idx = rng.choice(X.shape[0], size=B, replace=False).astype(np.int32)
    eps = rng.standard_normal((B, cfg.Dz)).astype(np.float32)
    return cfg, X, params, acc, idx, eps


def philox_setup():
    cfg = A.AEConfig(**PHILOX_KW)
    X = data_for(cfg, 4 * PHILOX_B, seed=5)
    params = [(p * 30).astype(np.float32) for p in V.init_params(cfg, seed=11)]
    acc = [np.full(p.shape, 1e-4, np.float32) for p in params]
    idx = np.random.default_rng(6).choice(X.shape[0], size=PHILOX_B, replace=False).astype(np.int32)
    return cfg, X, params, acc, idx


def step64(cfg, X, params, acc, idx, eps):
    return V.train_step([p.astype(np.float64) for p in params], [a.astype(np.float64) for a in acc],
                        X.astype(np.float64), idx, np.asarray(eps, np.float64), cfg)


# ------------------------------------------------------------------ 1. the helper's gradient
def torch_objective(tp, X, eps, cfg):
    import torch
    act = {"tanh": torch.tanh, "sigmoid": torch.sigmoid, "relu": torch.relu}[cfg.act]
    ne, nd = len(cfg.Denc), len(cfg.Ddec)
    h = X
    for i in range(ne):
        h = act(h @ tp[f"Wenc{i}"] + tp[f"benc{i}"])
    mu = h @ tp["Wzmu"] + tp["bzmu"]
    lv = h @ tp["Wzlv"] + tp["bzlv"]
    g = mu + torch.exp(lv / 2) * eps
    for i in range(nd):
        g = act(g @ tp[f"Wdec{i}"] + tp[f"bdec{i}"])
    if cfg.otype == "binary":
        P = torch.sigmoid(g @ tp["Wout"] + tp["bout"])
        loglik = (X * torch.log(P + A.EPS_LOG) + (1 - X) * torch.log(1 - P + A.EPS_LOG)).sum()
    else:
        xm = torch.sigmoid(g @ tp["Wmu"] + tp["bmu"])
        ls2 = g @ tp["Wlogs2"] + tp["blogs2"]
        loglik = (-0.5 * (A.LOG2PI + ls2 + (X - xm) ** 2 / torch.exp(ls2))).sum()
    negkl = 0.5 * (1 + lv - mu * mu - torch.exp(lv)).sum()
    prior = sum(-0.5 * (q * q / cfg.s2 + np.log(2 * np.pi * cfg.s2)).sum() for q in tp.values())
    return loglik + negkl + prior, loglik, negkl


@pytest.mark.parametrize("case", [STEP_CASES[0], STEP_CASES[1]], ids=STEP_IDS[:2])
def test_helper_gradient_matches_autograd(case):
    import torch
    name, kw, B, scale = case
    cfg, X, params, acc, idx, eps = step_setup(kw, B, scale)
    p64 = [p.astype(np.float64) for p in params]
    out = V.forward_backward(p64, X[idx].astype(np.float64), eps.astype(np.float64), cfg)
    tp = {n: torch.tensor(p, dtype=torch.float64, requires_grad=True) for n, p in zip(V.names(cfg), p64)}
    f, loglik, negkl = torch_objective(tp, torch.tensor(X[idx], dtype=torch.float64),
                                       torch.tensor(eps, dtype=torch.float64), cfg)
    f.backward()
    assert abs(out["f"] - f.item()) <= 1e-9 * abs(f.item())
    assert abs(out["loglik"] - loglik.item()) <= 1e-9 * abs(loglik.item())
    assert abs(out["negkl"] - negkl.item()) <= 1e-9 * abs(negkl.item())
    for n, g in zip(V.names(cfg), out["grads"]):
        ref = tp[n].grad.numpy()
        assert np.abs(g - ref).max() <= 1e-9 * np.abs(ref).max(), n


# ------------------------------------------------------------------ 2. degenerate identity
@pytest.mark.parametrize("kw", [STEP_CASES[0][1], STEP_CASES[1][1]], ids=STEP_IDS[:2])
def test_zero_noise_zero_lv_head_is_the_point_model(kw):
    cfg = A.AEConfig(**kw)
    X = data_for(cfg, 40).astype(np.float64)
    point = [(p * 30).astype(np.float64) for p in A.init_params(cfg, seed=3)]
    ref = A.forward_backward(point, X, cfg)
    out = V.forward_backward(V.from_point(point, cfg), X, np.zeros((40, cfg.Dz)), cfg)
    assert out["loglik"] == ref["loglik"]
    rg = dict(zip([n for n, _ in A.param_shapes(cfg)], ref["grads"]))
    for n, g in zip(V.names(cfg), out["grads"]):
        if n in V.LV_NAMES:
            continue
        r = rg[{"Wzmu": "Wz", "bzmu": "bz"}.get(n, n)]
        assert np.abs(g - r).max() <= 1e-12 * np.abs(r).max(), n


# ------------------------------------------------------------------ 3. float32 headroom
def assert_step_close(got, ref, eta):
    """The GPU step test's caps on (value, theta', acc')."""
    (gv, gp, ga), (rv, rp, ra) = got, ref
    assert abs(gv - rv) <= VALUE_RTOL * abs(rv), (gv, rv)
    check_theta(V.flatten(gp), V.flatten(rp), eta)
    ga, ra = V.flatten(ga).astype(np.float64), V.flatten(ra).astype(np.float64)
    assert np.linalg.norm(ga - ra) <= ACC_RTOL * np.linalg.norm(ra)


@pytest.mark.parametrize("case", STEP_CASES, ids=STEP_IDS)
def test_float32_oracle_run_sits_inside_the_gpu_caps(case):
    name, kw, B, scale = case
    cfg, X, params, acc, idx, eps = step_setup(kw, B, scale)
    rv, rp, ra, _ = step64(cfg, X, params, acc, idx, eps)
    gv, gp, ga, _ = V.train_step(params, acc, X, idx, eps, cfg)
    assert gp[0].dtype == np.float32
    assert_step_close((gv, gp, ga), (rv, rp, ra), cfg.eta)


def test_float32_philox_case_sits_inside_the_gpu_caps():
    cfg, X, params, acc, idx = philox_setup()
    eps = V.train_eps(SEED, idx, cfg.Dz, STEP)
    rv, rp, ra, _ = step64(cfg, X, params, acc, idx, eps)
    gv, gp, ga, _ = V.train_step(params, acc, X, idx, eps.astype(np.float32), cfg)
    assert_step_close((gv, gp, ga), (rv, rp, ra), cfg.eta)


# ------------------------------------------------------------------ 4. mis-keying is visible
def _wrong_eps(kind, idx, Dz):
    j = np.arange(Dz, dtype=np.int64)[None, :]
    if kind == "row_is_m":            # keyed by the position in the batch, not the dataset row
        return philox.latent_normal(SEED, np.arange(len(idx), dtype=np.int64)[:, None], j, STEP, 0)
    if kind == "next_step":
        return V.train_eps(SEED, idx, Dz, STEP + 1)
    if kind == "eval_domain":
        return philox.latent_normal(SEED, np.asarray(idx, np.int64)[:, None], j, STEP, 1)
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["row_is_m", "next_step", "eval_domain"])
def test_philox_step_case_tells_a_mis_keyed_site_apart(kind):
    """Under each wrong key the oracle step leaves the correctly keyed one by more than 100 times
    the GPU tolerance: the value by > 100 * 2e-5 relative, or theta' in more than 100 * 1e-4 of
    its elements by > 1e-3 eta (check_theta's share)."""
    cfg, X, params, acc, idx = philox_setup()
    assert not np.array_equal(idx, np.arange(len(idx)))
    rv, rp, _, _ = step64(cfg, X, params, acc, idx, V.train_eps(SEED, idx, cfg.Dz, STEP))
    wv, wp, _, _ = step64(cfg, X, params, acc, idx, _wrong_eps(kind, idx, cfg.Dz))
    d = np.abs(V.flatten(wp).astype(np.float64) - V.flatten(rp).astype(np.float64))
    value_off = abs(wv - rv) > 100 * VALUE_RTOL * abs(rv)
    theta_off = float((d > 1e-3 * cfg.eta).mean()) > 100 * 1e-4
    assert value_off or theta_off, (wv, rv, float((d > 1e-3 * cfg.eta).mean()))


# ------------------------------------------------------------------ 5. ABI
def test_ae_config_layout():
    from vaeb_amd import _lib
    assert ctypes.sizeof(_lib.AEConfigC) == 120
    assert _lib.AEConfigC.latent.offset == 104


def test_create_rejects_an_unknown_latent_before_the_device():
    from vaeb_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = _lib.load()
    c = _lib.AEConfigC()
    c.Dobs, c.Dz, c.n_enc, c.n_dec = 8, 2, 1, 1
    c.Denc[0] = c.Ddec[0] = 4
    c.s2, c.eta, c.max_batch = 1.0, 0.01, 4
    c.latent = 2
    h = ctypes.c_void_p()
    assert L.vaeb_ae_create(ctypes.byref(c), ctypes.byref(h)) == -1
    assert b"latent" in L.vaeb_last_error()
    assert not h.value


def test_param_shapes_gauss_order():
    from vaeb_amd import ae
    shp = ae.param_shapes(37, (29, 17), 5, (13, 21), "cont", latent="gauss")
    assert [n for n, _ in shp] == ["W0", "W1", "b0", "b1", "Wzmu", "Wzlv", "bzmu", "bzlv", "W0", "W1", "b0", "b1",
                                   "Wmu", "Wlogs2", "bmu", "blogs2"]
    assert dict(shp[4:8]) == {"Wzmu": (17, 5), "Wzlv": (17, 5), "bzmu": (5,), "bzlv": (5,)}
    cfg = A.AEConfig(Dobs=37, Denc=(29, 17), Dz=5, Ddec=(13, 21), otype="cont")
    assert [s for _, s in shp] == [s for _, s in V.param_shapes(cfg)]
    assert ae.param_shapes(37, (29, 17), 5, (13, 21), "cont") == ae.param_shapes(37, (29, 17), 5, (13, 21), "cont",
                                                                                latent="point")
