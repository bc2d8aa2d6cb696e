"""Host checks (no GPU) of the layer-stack engine's denoising training (include/vaeb_hip.h
enum vaeb_ae_corruption): the oracle the GPU tests compare against (tests/denoise_oracle.py) is
pinned to float64 torch autograd for every latent and output type, the GPU cases' inputs are shown to sit
inside their caps in float32, to tell a mis-keyed draw apart and to show the two wirings most likely
to be got wrong (the output scored on the corrupted rows; the first layer's gradient taken from the
clean rows), the counter layout is shown to be disjoint from every other draw, and the ABI and Python
additions are checked.

The GPU cases (tests/test_gpu_denoise.py) are defined here so both files share them.  Caps are those
of tests/test_gpu_ae.py / tests/test_vae_stack_host.py (VALUE_RTOL, ACC_RTOL, check_theta).
"""
import ctypes
import dataclasses
import os

import numpy as np
import pytest

from oracle import ae_oracle as A
from oracle import philox
from tests import denoise_oracle as D
from tests import vae_stack_oracle as V
from tests.test_gpu_ae import check_theta
from tests.test_vae_stack_host import (ACC_RTOL, PHILOX_B, SEED, STEP, STEP_CASES, VALUE_RTOL, philox_setup,
                                       step_setup)

COR_SEED = 0x0FEDCBA9_87654321      # the corruption's own seed, above 2^32 as SEED
SHAPES = {"A": STEP_CASES[0], "B": STEP_CASES[1], "C": STEP_CASES[3]}

# name: shape, latent, otype / act overrides, corruption kind, level, iw_samples
DENOISE_CASES = {
    "A_gauss_bin_mask": ("A", "gauss", {}, "mask", 0.3, 1),
    "B_point_cont_gauss": ("B", "point", {}, "gauss", 0.5, 1),
    "C_act_se_saltpepper": ("C", "act", dict(otype="se"), "saltpepper", 0.4, 1),
    "A_iw3_mask": ("A", "gauss", {}, "mask", 0.3, 3),
}
DENOISE_IDS = list(DENOISE_CASES)


@dataclasses.dataclass
class Case:
    cfg: A.AEConfig
    latent: str
    kind: str
    level: float
    K: int
    X: np.ndarray
    params: list
    acc: list
    idx: np.ndarray
    eps: np.ndarray        # [B, Dz], or [K, B, Dz] with K >= 2; None without a Gaussian latent
    draw: np.ndarray       # the host-pushed corruption draws [B, Dobs]


def denoise_case(name):
    """One single-step case on step_setup's data (tests/test_vae_stack_host.py): acc = 1e-4, a gathered
    idx; Gaussian latent: that file's parameters, the heads scaled where it scales them."""
    shape, latent, over, kind, level, K = DENOISE_CASES[name]
    _, kw, B, scale = SHAPES[shape]
    gcfg, X, gparams, _, idx, eps = step_setup(kw, B, scale)
    cfg = dataclasses.replace(gcfg, **over)
    if latent == "gauss":
        params = gparams
    else:
        # every parameter x30 (philox_setup's scale): at theta_0 the encoder's data gradient is below the
        # prior's, and a first-layer gradient taken from the wrong rows would not show
        params = [(p * 30).astype(np.float32) for p in D.init_params(cfg, latent)]
    acc = [np.full(p.shape, 1e-4, np.float32) for p in params]
    rng = np.random.default_rng(17)
    draw = (rng.standard_normal((B, cfg.Dobs)) if kind == "gauss" else rng.random((B, cfg.Dobs))).astype(np.float32)
    if latent != "gauss":
        eps = None
    elif K >= 2:
        eps = rng.standard_normal((K, B, cfg.Dz)).astype(np.float32)
    return Case(cfg, latent, kind, level, K, X, params, acc, idx, eps, draw)


def oracle_step(c, dt, draw=None, score_on_xt=False, wrong=None):
    """(value, theta', acc') of the case's step in dtype dt: xt formed in dt from the clean rows."""
    X = c.X[c.idx].astype(dt)
    xt = D.corrupt(X, c.kind, c.level, (c.draw if draw is None else draw).astype(dt))
    Y = xt if score_on_xt else X
    p = [q.astype(dt) for q in c.params]
    a = [q.astype(dt) for q in c.acc]
    if c.K >= 2:
        assert wrong is None
        v, np_, na, _ = D.iw_train_step(p, a, xt, Y, c.eps.astype(dt), c.cfg)
    else:
        v, np_, na, _ = D.train_step(p, a, xt, Y, c.cfg, c.latent, None if c.eps is None else c.eps.astype(dt), wrong)
    return v, np_, na


def assert_step_close(got, ref, eta):
    """The GPU step test's caps on (value, theta', acc')."""
    (gv, gp, ga), (rv, rp, ra) = got, ref
    assert abs(gv - rv) <= VALUE_RTOL * abs(rv), (gv, rv)
    check_theta(A.flatten(gp), A.flatten(rp), eta)
    ga, ra = A.flatten(ga).astype(np.float64), A.flatten(ra).astype(np.float64)
    assert np.linalg.norm(ga - ra) <= ACC_RTOL * np.linalg.norm(ra)


def far_apart(wrong, ref, eta):
    """More than 100 times the GPU caps apart: the value by > 100 * VALUE_RTOL relative, or theta' in
    more than 100 * 1e-4 of its elements by > 1e-3 eta (check_theta's share)."""
    (wv, wp, _), (rv, rp, _) = wrong, ref
    d = np.abs(A.flatten(wp).astype(np.float64) - A.flatten(rp).astype(np.float64))
    share = float((d > 1e-3 * eta).mean())
    return abs(wv - rv) > 100 * VALUE_RTOL * abs(rv) or share > 100 * 1e-4, (wv, rv, share)


# the Philox-mode step: philox_setup's case (every parameter x30), MASK 0.3, latent and corruption
# draws from their own seeds at one step
PHILOX_KIND, PHILOX_LEVEL = "mask", 0.3


def philox_case(draw=None):
    cfg, X, params, acc, idx = philox_setup()
    r, _ = D.corruption_draws(COR_SEED, idx, cfg.Dobs, STEP)
    eps = V.train_eps(SEED, idx, cfg.Dz, STEP)
    return Case(cfg, "gauss", PHILOX_KIND, PHILOX_LEVEL, 1, X, params, acc, idx, eps, r if draw is None else draw)


# ------------------------------------------------------------------ 1. Xin != Y: autograd
def torch_objective(tp, Xin, Y, eps, cfg, latent):
    import torch
    act = {"tanh": torch.tanh, "sigmoid": torch.sigmoid, "relu": torch.relu}[cfg.act]
    h = Xin
    for i in range(len(cfg.Denc)):
        h = act(h @ tp[f"Wenc{i}"] + tp[f"benc{i}"])
    extra = 0.0
    if latent == "gauss":
        mu, lv = h @ tp["Wzmu"] + tp["bzmu"], h @ tp["Wzlv"] + tp["bzlv"]
        g = mu + torch.exp(lv / 2) * eps
        extra = 0.5 * (1 + lv - mu * mu - torch.exp(lv)).sum()
    else:
        g = h @ tp["Wz"] + tp["bz"]
        if latent == "act":
            g = act(g)
        else:
            extra = -0.5 * (g * g + A.LOG2PI).sum()
    for i in range(len(cfg.Ddec)):
        g = act(g @ tp[f"Wdec{i}"] + tp[f"bdec{i}"])
    if cfg.otype == "cont":
        xm = torch.sigmoid(g @ tp["Wmu"] + tp["bmu"])
        ls2 = g @ tp["Wlogs2"] + tp["blogs2"]
        data = (-0.5 * (A.LOG2PI + ls2 + (Y - xm) ** 2 / torch.exp(ls2))).sum()
    else:
        P = torch.sigmoid(g @ tp["Wout"] + tp["bout"])
        if cfg.otype == "se":
            data = -((Y - P) ** 2).sum()
        else:
            data = (Y * torch.log(P + A.EPS_LOG) + (1 - Y) * torch.log(1 - P + A.EPS_LOG)).sum()
    prior = sum(-0.5 * (q * q / cfg.s2 + np.log(2 * np.pi * cfg.s2)).sum() for q in tp.values())
    return data + extra + prior


ODD_KW = dict(Dobs=37, Denc=(29, 17), Dz=5, Ddec=(13, 21), s2=2.0)
# every valid (latent, otype) pair: this is where each is held to autograd with Xin != Y
AUTOGRAD = [
    ("gauss", dict(ODD_KW, otype="binary")),
    ("point", dict(Dobs=48, Denc=(20,), Dz=20, Ddec=(18, 11), otype="cont", act="sigmoid")),
    ("act", dict(Dobs=64, Denc=(32,), Dz=16, Ddec=(32,), otype="se")),
    ("gauss", dict(ODD_KW, otype="cont", act="sigmoid")),
    ("point", dict(ODD_KW, otype="binary", act="relu")),
    ("point", dict(ODD_KW, otype="se")),
    ("act", dict(ODD_KW, otype="binary", act="sigmoid")),
    ("act", dict(ODD_KW, otype="cont", act="relu")),
]


@pytest.mark.parametrize("latent,kw", AUTOGRAD, ids=["gauss-binary-odd", "point-cont", "act-se", "gauss-cont", "point-binary",
                                                     "point-se", "act-binary", "act-cont"])
def test_gradient_with_a_separate_encoder_input_matches_autograd(latent, kw):
    import torch
    cfg = A.AEConfig(**kw)
    rng = np.random.default_rng(5)
    M = 23
    Y = (rng.random((M, cfg.Dobs)) < 0.3).astype(np.float64) if cfg.otype == "binary" else rng.beta(2.0, 2.0, size=(M, cfg.Dobs))
    Xin = D.corrupt(Y, "saltpepper", 0.4, rng.random(Y.shape))
    assert (Xin != Y).mean() > 0.1
    eps = rng.standard_normal((M, cfg.Dz))
    params = [(p * 20).astype(np.float64) for p in D.init_params(cfg, latent, seed=7)]
    out = D.forward_backward(params, Xin, Y, cfg, latent, eps if latent == "gauss" else None)
    tp = {n: torch.tensor(p, dtype=torch.float64, requires_grad=True) for n, p in zip(D.names(cfg, latent), params)}
    f = torch_objective(tp, torch.tensor(Xin), torch.tensor(Y), torch.tensor(eps), cfg, latent)
    f.backward()
    assert abs(out["f"] - f.item()) <= 1e-9 * abs(f.item())
    for n, g in zip(D.names(cfg, latent), out["grads"]):
        ref = tp[n].grad.numpy()
        assert np.abs(g - ref).max() <= 1e-9 * np.abs(ref).max(), n


# ------------------------------------------------------------------ 3. float32 headroom
@pytest.mark.parametrize("name", DENOISE_IDS)
def test_float32_oracle_run_sits_inside_the_gpu_caps(name):
    c = denoise_case(name)
    got = oracle_step(c, np.float32)
    assert got[1][0].dtype == np.float32
    assert_step_close(got, oracle_step(c, np.float64), c.cfg.eta)


def test_float32_philox_case_sits_inside_the_gpu_caps():
    c = philox_case()
    assert_step_close(oracle_step(c, np.float32), oracle_step(c, np.float64), c.cfg.eta)


def test_corrupt_decides_identically_in_float32_and_float64():
    """r on the 2^-24 grid, the float32 level and its half are exact in both dtypes."""
    c = philox_case()
    X = c.X[c.idx]
    for kind in ("mask", "saltpepper"):
        a = D.corrupt(X.astype(np.float32), kind, 0.3, c.draw)
        b = D.corrupt(X.astype(np.float64), kind, 0.3, c.draw)
        assert a.dtype == np.float32 and np.array_equal(a, b)


# ------------------------------------------------------------------ 4. mis-keying is visible
def wrong_draw(kind, idx, Dobs):
    d = np.arange(Dobs, dtype=np.int64)[None, :]
    row = np.asarray(idx, np.int64)[:, None]
    if kind == "row_is_m":            # keyed by the position in the batch, not the dataset row
        return D.corruption_draws(COR_SEED, np.arange(len(idx)), Dobs, STEP)[0]
    if kind == "next_step":
        return D.corruption_draws(COR_SEED, idx, Dobs, STEP + 1)[0]
    if kind == "out0":                # r from output word 0, not 2
        return (D.corruption_words(COR_SEED, row, D.C1_CORRUPT | d, STEP)[0] >> np.uint64(8)).astype(np.float64) / 2.0 ** 24
    if kind == "no_bit31":            # c1 = d: the latent draws' field
        return (D.corruption_words(COR_SEED, row, d, STEP)[2] >> np.uint64(8)).astype(np.float64) / 2.0 ** 24
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["row_is_m", "next_step", "out0", "no_bit31"])
def test_philox_step_case_tells_a_mis_keyed_draw_apart(kind):
    c = philox_case()
    assert not np.array_equal(c.idx, np.arange(len(c.idx)))
    X = c.X[c.idx].astype(np.float64)
    w = wrong_draw(kind, c.idx, c.cfg.Dobs)
    share = float((D.corrupt(X, c.kind, c.level, w) != D.corrupt(X, c.kind, c.level, c.draw)).mean())
    print(f"{kind}: xt differs in {share:.3f} of its elements")
    assert share > 0.10, share
    ok, figs = far_apart(oracle_step(c, np.float64, draw=w), oracle_step(c, np.float64), c.cfg.eta)
    assert ok, figs


# ------------------------------------------------------------------ 5. the clean target is visible
@pytest.mark.parametrize("name", DENOISE_IDS + ["philox"])
def test_scoring_on_the_corrupted_rows_is_visible(name):
    c = philox_case() if name == "philox" else denoise_case(name)
    ok, figs = far_apart(oracle_step(c, np.float64, score_on_xt=True), oracle_step(c, np.float64), c.cfg.eta)
    assert ok, figs


@pytest.mark.parametrize("name", [n for n in DENOISE_IDS if DENOISE_CASES[n][5] < 2] + ["philox"])
def test_first_layer_gradient_from_the_clean_rows_is_visible(name):
    c = philox_case() if name == "philox" else denoise_case(name)
    ok, figs = far_apart(oracle_step(c, np.float64, wrong="first_grad_clean"), oracle_step(c, np.float64), c.cfg.eta)
    assert ok, figs


# ------------------------------------------------------------------ 6. counter domains
def _as128(words):
    return {tuple(int(v) for v in t) for t in zip(*[np.asarray(w).ravel() for w in words])}


def test_corruption_counters_are_distinct_and_disjoint_from_every_other_draw():
    cfg, X, params, acc, idx = philox_setup()
    K = 3
    cor = _as128(D.corruption_counters(idx, cfg.Dobs, STEP))
    assert len(cor) == len(idx) * cfg.Dobs
    j = np.arange(cfg.Dz, dtype=np.int64)[None, :]
    row = idx.astype(np.int64)[:, None]
    latent = _as128(philox.latent_counters(row, j, STEP, 0))
    iw = set().union(*[_as128(philox.latent_counters(row, j, STEP, k << 1)) for k in range(K)])
    fvs = _as128(philox.fvs_counters(STEP, sum(p.size for p in params)))
    for other in (latent, iw, fvs):
        assert other and not (cor & other)
    # every c1 of the layout has bit 31 set, no other draw's has
    assert all(c[1] >> 31 for c in cor) and not any(c[1] >> 31 for c in latent | iw | fvs)


# ------------------------------------------------------------------ 7. moments
def test_moments_of_2_pow_18_draws():
    """N = 2^18 draws.  A share of N Bernoulli(q) decisions has standard error sqrt(q (1 - q) / N); the
    bounds are 4 of them.  The normals: 5 standard errors of the mean, the variance and the fourth
    moment, as tests/test_philox_oracle.py holds its 2^19 draws."""
    N_ = 1 << 18
    r, n = D.corruption_draws((3 << 32) | 9, np.arange(512) + (1 << 20), 512, STEP)
    assert r.size == N_ and r.min() >= 0 and r.max() < 1 and np.array_equal(r * 2 ** 24, np.floor(r * 2 ** 24))
    p = 0.3
    X = np.full(r.shape, 0.5)
    mask = D.corrupt(X, "mask", p, r)
    sp = D.corrupt(X, "saltpepper", p, r)
    q = float(np.float32(p))
    for what, share, want in (("mask", (mask == 0).mean(), q), ("pepper", (sp == 0).mean(), q / 2),
                              ("salt", (sp == 1).mean(), q / 2)):
        assert abs(share - want) <= 4 * np.sqrt(want * (1 - want) / N_), (what, share)
    assert ((sp == 0) | (sp == 1) | (sp == X)).all() and ((mask == 0) | (mask == X)).all()
    x = n.ravel()
    se_m, se_v, se_4 = 1 / np.sqrt(N_), np.sqrt(2 / N_), np.sqrt(96 / N_)
    assert np.all(np.isfinite(x))
    assert abs(x.mean()) <= 5 * se_m and abs(x.var() - 1) <= 5 * se_v and abs((x ** 4).mean() - 3) <= 5 * se_4
    assert np.abs(x).max() <= np.sqrt(2 * np.log(2.0 ** 24)) + 1e-12
    # r (out2) and n (out0, out1) of one block are uncorrelated
    assert abs(float(((r.ravel() - 0.5) * x).mean())) <= 5 * np.sqrt(1 / 12) / np.sqrt(N_)


def test_issue_figures_of_the_layout():
    """(23 x 37) draws at p = 0.3: the functions of oracle/philox.py take c1 with bit 31 set."""
    cfg, X, params, acc, idx = philox_setup()
    r, n = D.corruption_draws(COR_SEED, idx, cfg.Dobs, STEP)
    assert r.shape == n.shape == (PHILOX_B, cfg.Dobs)
    assert 0.2 < float((r < np.float32(0.3)).mean()) < 0.4


# ------------------------------------------------------------------ 8. ABI and Python surface
def test_ae_config_corruption_field():
    from vaeb_amd import _lib
    assert ctypes.sizeof(_lib.AEConfigC) == 120
    assert _lib.AEConfigC.corruption.offset == 112
    assert _lib.AEConfigC.latent.offset == 104


def test_noise_schedule():
    from vaeb_amd import ae
    assert ae.noise_schedule([.5, .3, .1], 7) == [.5, .5, .5, .3, .3, .1, .1]
    assert ae.noise_schedule([.5, .3, .1], 2) == [.5, .3]
    assert ae.noise_schedule([.2], 3) == [.2, .2, .2]


def test_train_epochs_rejects_a_schedule_of_another_length():
    from vaeb_amd import ae

    def train(idx):
        raise AssertionError("no step may run")

    with pytest.raises(ValueError, match="levels"):
        ae.train_epochs(train, 10, 3, noise=[0.1, 0.2])


def test_cli_rejects_noise_without_corruption_and_an_unknown_kind(tmp_path):
    from vaeb_amd import vanilla_ae
    out = tmp_path / "res"
    with pytest.raises(ValueError, match="--corruption"):
        vanilla_ae.main(["--noise", "0.3,0.1", "--out", str(out)])
    with pytest.raises(ValueError, match="not supported"):
        vanilla_ae.main(["--corruption", "blur", "--out", str(out)])
    assert not out.exists()


def test_create_rejects_an_unknown_corruption_before_the_device():
    from vaeb_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = _lib.load()
    c = _lib.AEConfigC()
    c.Dobs, c.Dz, c.n_enc, c.n_dec = 8, 2, 1, 1
    c.Denc[0] = c.Ddec[0] = 4
    c.s2, c.eta, c.max_batch = 1.0, 0.01, 4
    for bad in (4, -1):
        c.corruption = bad
        h = ctypes.c_void_p()
        assert L.vaeb_ae_create(ctypes.byref(c), ctypes.byref(h)) == -1
        assert b"corruption" in L.vaeb_last_error()
        assert not h.value
