"""Host checks (no GPU) of the two-mode latent prior (include/vaeb_hip.h enum vaeb_ae_prior): the
NumPy oracle the GPU tests compare against (tests/vae_prior_oracle.py) is pinned to float64 torch
autograd of the written-out objective, to tests/vae_stack_iwtrain_oracle.py at a = 0, s = 1 and, in
expectation over eps, to the analytic KL of tests/vae_stack_oracle.py; the GPU cases
(tests/vae_prior_cases.py) are shown to meet the conditions without which a wrong kernel would
pass, to sit inside the borrowed caps in float32, and to tell five kinds of wrong kernel apart;
and the ABI additions are checked as far as they need no device.

The caps are borrowed, none is new: VALUE_RTOL = 2e-5, ACC_RTOL = 1e-4 and check_theta
(tests/test_gpu_ae.py, tests/test_vae_stack_host.py), and per parameter block MARGIN = 16 x the
float32 restatement's error with every such bound <= GRAD_CAP = 1e-4 (tests/ae_grad_cases.py).
vaeb_ae_set_prior's range errors need a context and so a device: tests/test_gpu_vae_prior.py.
"""
import ctypes
import math
import os

import numpy as np
import pytest

from oracle import ae_oracle as A
from tests import ae_grad_cases as G
from tests import vae_prior_cases as C
from tests import vae_prior_oracle as PO
from tests import vae_stack_iwtrain_oracle as T
from tests import vae_stack_oracle as V
from tests.test_vae_stack_host import ACC_RTOL, VALUE_RTOL

STEP_PARAMS = pytest.mark.parametrize("name,form", C.STEPS, ids=C.STEP_IDS)
HEADROOM = 4.0


# ------------------------------------------------------------------ 1. the oracle's gradient
def torch_objective(tp, X, eps, cfg, a, s, form):
    """The objective written out: log p(x | z) + log p(z) - log q(z | x) per sample, the entropy of
    q analytic in the ELBO form, logsumexp over the samples in the IW form."""
    import torch
    act = {"tanh": torch.tanh, "sigmoid": torch.sigmoid, "relu": torch.relu}[cfg.act]
    h = X
    for i in range(len(cfg.Denc)):
        h = act(h @ tp[f"Wenc{i}"] + tp[f"benc{i}"])
    mu = h @ tp["Wzmu"] + tp["bzmu"]
    lv = h @ tp["Wzlv"] + tp["bzlv"]
    eps3 = eps[None] if form == "elbo" else eps
    z = mu[None] + torch.exp(lv / 2)[None] * eps3
    g = z
    for i in range(len(cfg.Ddec)):
        g = act(g @ tp[f"Wdec{i}"] + tp[f"bdec{i}"])
    if cfg.otype == "binary":
        P = torch.sigmoid(g @ tp["Wout"] + tp["bout"])
        ll = (X * torch.log(P + A.EPS_LOG) + (1 - X) * torch.log(1 - P + A.EPS_LOG)).sum(-1)
    else:
        xm = torch.sigmoid(g @ tp["Wmu"] + tp["bmu"])
        ls2 = g @ tp["Wlogs2"] + tp["blogs2"]
        ll = (-0.5 * (A.LOG2PI + ls2 + (X - xm) ** 2 / torch.exp(ls2))).sum(-1)
    # log of the mixture density itself, through logsumexp of its two components
    comp = torch.stack([-0.5 * (z / s) ** 2, -0.5 * ((z - a) / s) ** 2])
    logp = torch.logsumexp(comp, 0) + math.log(0.5) - math.log(s) - 0.5 * math.log(2 * math.pi)
    if form == "elbo":
        entropy = 0.5 * (1 + lv + math.log(2 * math.pi))
        value = ll.sum() + logp.sum() + entropy.sum()
    else:
        logq = -0.5 * (eps3 ** 2 + lv[None] + math.log(2 * math.pi))
        lw = ll + (logp - logq).sum(-1)
        value = (torch.logsumexp(lw, 0) - math.log(lw.shape[0])).sum()
    prior = sum(-0.5 * (q * q / cfg.s2 + np.log(2 * np.pi * cfg.s2)).sum() for q in tp.values())
    return value + prior, value


@pytest.mark.parametrize("name,form", [("dz17_m5_cont_a2", "elbo"), ("dz17_m5_cont_a2", "iw"),
                                       ("dz33_m33_bin", "elbo"), ("dz33_m33_bin", "iw"), ("dz1_m5_bin", "iw")])
def test_oracle_matches_autograd(name, form):
    import torch
    st, c = C.step(name, form), C.CASE[name]
    cfg = st.cfg
    a, s = PO.abi_prior(c.mean1, c.width)
    tp = {n: torch.tensor(p.astype(np.float64), requires_grad=True) for n, p in zip(V.names(cfg), st.params)}
    f, value = torch_objective(tp, torch.tensor(st.Xtr[st.idx].astype(np.float64)),
                               torch.tensor(st.eps.astype(np.float64)), cfg, a, s, form)
    f.backward()
    out = st.out64
    assert abs(out["value"] - value.item()) <= 1e-9 * abs(value.item())
    assert abs(out["f"] - f.item()) <= 1e-9 * abs(f.item())
    for n, g in zip(V.names(cfg), out["grads"]):
        ref = tp[n].grad.numpy()
        assert np.abs(g - ref).max() <= 1e-9 * np.abs(ref).max(), n


# ------------------------------------------------------------------ 2. a = 0, s = 1
@pytest.mark.parametrize("name", ["dz17_m5_cont_a2", "dz33_m33_bin", "dz16_m1_bin"])
def test_iw_form_at_0_1_is_the_normal_prior_oracle(name):
    cfg, Xtr, idx, params, eps = C.inputs(name)
    p64 = [q.astype(np.float64) for q in params]
    X, e = Xtr[idx].astype(np.float64), eps["iw"].astype(np.float64)
    ref = T.forward_backward(p64, X, e, cfg)
    out = PO.forward_backward(p64, X, e, cfg, 0.0, 1.0, "iw")
    assert abs(out["value"] - ref["iw"]) <= 1e-12 * abs(ref["iw"])
    assert np.abs(out["rows"] - ref["rows"]).max() <= 1e-12 * np.abs(ref["rows"]).max()
    for n, g, r in zip(V.names(cfg), out["grads"], ref["grads"]):
        assert np.abs(g - r).max() <= 1e-12 * np.abs(r).max(), n


def test_elbo_form_at_0_1_has_the_analytic_kl_as_its_expectation():
    """Per draw, value(eps) - [loglik(eps) + negKL] = latent(eps) - negKL; its mean over 4096 draws
    lies within 5 standard errors of 0."""
    cfg, Xtr, idx, params, _ = C.inputs("dz17_m5_cont_a2")
    p64 = [q.astype(np.float64) for q in params]
    X = Xtr[idx].astype(np.float64)
    rng = np.random.default_rng(11)
    d = []
    for _ in range(4096):
        e = rng.standard_normal((len(idx), cfg.Dz))
        out = PO.forward_backward(p64, X, e, cfg, 0.0, 1.0, "elbo", need_grad=False)
        ref = V.forward_backward(p64, X, e, cfg, need_grad=False)
        assert abs(out["loglik"] - ref["loglik"]) <= 1e-12 * abs(ref["loglik"])
        d.append(out["value"] - ref["elbo"])
    d = np.asarray(d)
    se = d.std(ddof=1) / math.sqrt(len(d))
    print(f"mean difference {d.mean():+.4f}, standard error {se:.4f}, negKL {ref['negkl']:.3f}")
    assert se > 0 and abs(d.mean()) <= 5 * se


# ------------------------------------------------------------------ 3. the inputs
def test_input_conditions():
    """Over the elements of the GPU cases: r < 0.05, 0.05 <= r <= 0.95 and r > 0.95 each hold at least
    10 % (a kernel that dropped r, or pinned it, would otherwise pass), some case has |t| > 100 (a
    naive softplus overflows float32 from t = 88.8), and mu covers about [-0.5 a, 1.5 a]."""
    r = np.concatenate([C.step(n, f).out64["r"].ravel() for n, f in C.STEPS])
    shares = (float((r < 0.05).mean()), float(((r >= 0.05) & (r <= 0.95)).mean()), float((r > 0.95).mean()))
    print("shares of r < 0.05, between, > 0.95: %.3f %.3f %.3f" % shares)
    assert min(shares) >= 0.10, shares
    tmax = {n: float(np.abs(C.step(n, "elbo").out64["t"]).max()) for n in C.NAMES}
    print("max |t| per case:", {n: round(v, 1) for n, v in tmax.items()})
    assert max(tmax.values()) > 100
    for n in C.NAMES:
        st, c = C.step(n, "elbo"), C.CASE[n]
        u = st.out64["mu"] / c.mean1
        assert -1.5 < u.min() and u.max() < 2.5, (n, u.min(), u.max())
        if st.cfg.Dz >= 15:
            assert u.min() < 0.0 and u.max() > 1.0, (n, u.min(), u.max())
        assert not np.array_equal(st.idx, np.sort(st.idx)) or len(st.idx) == 1


def test_case_table_reaches_the_sizes_it_claims():
    cfgs = {c.name: c.cfg() for c in C.CASES}
    assert {g.Dz for g in cfgs.values()} >= {1, 15, 16, 17, 33}
    assert {c.M for c in C.CASES} >= {1, 5, 33, 100}
    assert {(c.M, c.K) for c in C.CASES} >= {(5, 2), (5, 3)}
    assert {c.width for c in C.CASES} == {0.5, 0.1, 0.05} and any(c.mean1 == 2.0 for c in C.CASES)
    assert {g.otype for g in cfgs.values()} == {"binary", "cont"}
    m = cfgs["mnist_like"]
    assert (m.Dobs, m.Denc, m.Dz, m.Ddec) == (784, (500,), 20, (500,)) and C.CASE["mnist_like"].M == 100
    for n, g in cfgs.items():
        if n != "mnist_like":
            assert 24 <= g.Dobs <= 96 and 12 <= g.Denc[0] <= 40 and 12 <= g.Ddec[0] <= 40


# ------------------------------------------------------------------ 4. float32 headroom
@STEP_PARAMS
def test_float32_restatement_sits_inside_the_caps(name, form):
    """By a factor 4: the zero-accumulator step's value and per-block bounds, and the single step
    from acc = 1e-4 (value, theta', accumulator norm)."""
    st, c = C.step(name, form), C.CASE[name]
    worst = max(st.bound, key=st.bound.get)
    print(f"{name}-{form}: restated value {st.restate_value:.1e}; largest bound {worst} {st.bound[worst]:.1e}")
    assert st.restate_value <= VALUE_RTOL / HEADROOM
    assert max(st.bound.values()) <= G.GRAD_CAP                     # 16 x the restatement: headroom 16
    assert min(st.restate.values()) > 0
    acc = C.acc0(st.params)
    rv, rp, ra, _ = C.step64(st.cfg, st.Xtr, st.params, acc, st.idx, st.eps, c.mean1, c.width, form)
    gv, gp, ga, _ = PO.train_step(st.params, acc, st.Xtr, st.idx, st.eps, st.cfg, c.mean1, c.width, form)
    assert gp[0].dtype == np.float32
    assert abs(gv - rv) <= VALUE_RTOL / HEADROOM * abs(rv)
    d = np.abs(V.flatten(gp) - V.flatten(rp))
    assert d.max() <= (2 * st.cfg.eta + 1e-7) / HEADROOM
    assert float((d > 1e-3 * st.cfg.eta).mean()) <= 1e-4 / HEADROOM
    if d.size < 1e4:                   # check_theta's share allows no element off: the threshold itself
        assert d.max() <= 1e-3 * st.cfg.eta / HEADROOM
    ga, ra = V.flatten(ga).astype(np.float64), V.flatten(ra).astype(np.float64)
    assert np.linalg.norm(ga - ra) <= ACC_RTOL / HEADROOM * np.linalg.norm(ra)


# ------------------------------------------------------------------ 5. wrong kernels are told apart
def caught(kind):
    """The (case, form, what) whose cap the wrong kernel `kind` passes: a gradient block above its
    bound, or the value above VALUE_RTOL.  The naive softplus runs in float32, as a kernel would."""
    hits = []
    for name, form in C.STEPS:
        if kind == "half_not_half_wn" and form != "iw":
            continue
        st, c = C.step(name, form), C.CASE[name]
        dt = np.float32 if kind == "naive_softplus" else np.float64
        with np.errstate(invalid="ignore", over="ignore"):           # the naive softplus: inf, then nan
            out = C.oracle(st.cfg, st.params, st.Xtr[st.idx], st.eps, c.mean1, c.width, form, dt, wrong=kind)
        v = out["value"] / len(st.idx)
        if not abs(v - st.value64) <= VALUE_RTOL * abs(st.value64):
            hits.append((name, form, "value"))
        g = dict(zip(V.names(st.cfg), [np.asarray(q, np.float64) for q in out["grads"]]))
        if kind != "naive_softplus":
            bad = G.rejected(G.block_errors(g, st.g64), st.bound)
            if bad:
                hits.append((name, form, bad[0]))
    return hits


@pytest.mark.parametrize("kind", PO.WRONG)
def test_wrong_kernel_is_told_apart(kind):
    hits = caught(kind)
    print(kind, "->", hits)
    assert hits
    if kind != "naive_softplus":       # a wrong gradient shows in every case it applies to
        forms = {(n, f) for n, f in C.STEPS if kind != "half_not_half_wn" or f == "iw"}
        assert {(n, f) for n, f, _ in hits} == forms


def test_nothing_wrong_passes_and_the_wrong_list_is_the_issues():
    assert PO.WRONG == ("r_dropped", "a_ignored", "c_on_z_alone", "half_not_half_wn", "naive_softplus")
    for name, form in C.STEPS:
        st, c = C.step(name, form), C.CASE[name]
        out = C.oracle(st.cfg, st.params, st.Xtr[st.idx], st.eps, c.mean1, c.width, form, np.float64)
        g = dict(zip(V.names(st.cfg), out["grads"]))
        assert not G.rejected(G.block_errors(g, st.g64), st.bound)


def test_stable_softplus_and_sigmoid_at_the_issues_example():
    """s = 0.05, z = 3: t = 1000.  The naive form is inf in float32; the stable ones are t and 1."""
    t, r, logp, pull = PO.prior_terms(np.float32([3.0]), 1.0, 0.05)
    assert abs(t[0] - 1000.0) < 1e-2 and np.isfinite(logp[0]) and r[0] == 1.0
    assert PO.softplus(t)[0] == t[0] and np.isinf(PO.softplus(t, naive=True)[0])
    t64, _, logp64, _ = PO.prior_terms(np.float64([3.0]), 1.0, 0.05)
    assert abs(logp[0] - logp64[0]) <= 1e-6 * abs(logp64[0])


# ------------------------------------------------------------------ 6. the ABI, without a device
def lib():
    from vaeb_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib, _lib.load()


def test_ae_config_has_the_prior_at_116():
    from vaeb_amd import _lib
    assert ctypes.sizeof(_lib.AEConfigC) == 120
    assert _lib.AEConfigC.prior.offset == 116 and _lib.AEConfigC.prior.size == 4
    assert _lib.AEConfigC.corruption.offset == 112 and _lib.AEConfigC.latent.offset == 104
    assert _lib.AE_PRIOR == {"normal": 0, "twomode": 1}


def small_config(_lib):
    c = _lib.AEConfigC()
    c.Dobs, c.Dz, c.n_enc, c.n_dec = 8, 2, 1, 1
    c.Denc[0] = c.Ddec[0] = 4
    c.s2, c.eta, c.max_batch = 1.0, 0.01, 4
    c.latent = _lib.AE_LATENT["gauss"]
    return c


@pytest.mark.parametrize("prior,latent", [(2, "gauss"), (-1, "gauss"), (1, "point"), (1, "act")])
def test_create_rejects_a_bad_prior_before_the_device(prior, latent):
    _lib, L = lib()
    c = small_config(_lib)
    c.prior, c.latent = prior, _lib.AE_LATENT[latent]
    h = ctypes.c_void_p()
    assert L.vaeb_ae_create(ctypes.byref(c), ctypes.byref(h)) == -1
    assert b"prior" in L.vaeb_last_error()
    assert not h.value


def test_new_calls_are_exported_and_reject_null():
    _lib, L = lib()
    for n in ("vaeb_ae_set_prior", "vaeb_ae_get_prior", "vaeb_ae_encode_bits", "vaeb_ae_decode_bits"):
        assert n in _lib.EXPORTS and hasattr(L, n)
    a, s = ctypes.c_float(), ctypes.c_float()
    assert L.vaeb_ae_set_prior(None, 1.0, 0.25) == -1
    assert L.vaeb_ae_get_prior(None, ctypes.byref(a), ctypes.byref(s)) == -1
    assert L.vaeb_ae_encode_bits(None, None, 1, None) == -1
    assert L.vaeb_ae_decode_bits(None, None, 1, None) == -1
    major, minor = ctypes.c_int32(), ctypes.c_int32()
    assert L.vaeb_version(ctypes.byref(major), ctypes.byref(minor)) == 0 and minor.value >= 4


def test_python_prior_arguments():
    from vaeb_amd import _lib, ae
    assert ae._prior(None) is None
    assert ae._prior("twomode") == (1.0, 0.25)
    assert ae._prior(("twomode", 0.1)) == (1.0, 0.1)
    assert ae._prior(("twomode", 2.0, 0.1)) == (2.0, 0.1)
    X = np.zeros((4, 8), np.float32)
    for bad in ("beta", ("twomode", 1.0, 0.1, 3.0), ("normal",)):
        with pytest.raises(ValueError, match="prior"):
            ae.ConstructVAE(X, Denc=[4], Dz=2, Ddec=[4], prior=bad)     # before a context is made
    with pytest.raises(_lib.VaebError, match="prior"):
        _lib.AEContext(8, [4], 2, [4], latent="gauss", prior="beta")
