"""Host checks (no GPU) of the vanilla squared-error autoencoder's oracle
(tests/vanilla_ae_oracle.py) and of the inputs and bounds of tests/test_gpu_vanilla_ae.py
(tests/vanilla_ae_cases.py).

1. The oracle's gradient against float64 torch autograd of the same logjoint, latent act x otype
   {se, binary, cont} and point x se, over tanh, sigmoid and relu (tolerance of tests/test_ae_oracle.py).
2. The known value: train_step's value is se / M, positive, and mse() of the reconstructions is it.
3. The inputs of the GPU cases are fair: every per-block bound (16 x the float32 restatement's
   error) is <= GRAD_CAP = 1e-4; at scaled weights f'(Z) matters; relu rows keep off the kink and
   have 20-80 % dead units, the latent layer included.  -s prints the restatement table.
4. Six kinds of wrong gradient (vanilla_ae_oracle.WRONG) each miss the bounds of at least one case.
"""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import ae_oracle as A
from tests import ae_grad_cases as G
from tests import vanilla_ae_cases as C
from tests import vanilla_ae_oracle as VA

CASE_PARAMS = pytest.mark.parametrize("name,latent,otype,scaled", C.CASES, ids=C.CASE_IDS)


# ------------------------------------------------------------------ 1. autograd
def torch_logjoint(params, X, cfg, latent):
    p = dict(zip(VA.names(cfg), params))
    f = {"tanh": torch.tanh, "sigmoid": torch.sigmoid, "relu": torch.relu}[cfg.act]
    H = X
    for i in range(len(cfg.Denc)):
        H = f(H @ p[f"Wenc{i}"] + p[f"benc{i}"])
    Z = H @ p["Wz"] + p["bz"]
    if latent == "act":
        Z = f(Z)
    Gd = Z
    for i in range(len(cfg.Ddec)):
        Gd = f(Gd @ p[f"Wdec{i}"] + p[f"bdec{i}"])
    if cfg.otype == "cont":
        mu = torch.sigmoid(Gd @ p["Wmu"] + p["bmu"])
        ls2 = Gd @ p["Wlogs2"] + p["blogs2"]
        value = -0.5 * (np.log(2 * np.pi) + ls2 + (X - mu) ** 2 / torch.exp(ls2)).sum()
        obj = value
    else:
        P = torch.sigmoid(Gd @ p["Wout"] + p["bout"])
        if cfg.otype == "se":
            value = ((X - P) ** 2).sum()
            obj = -value
        else:
            value = (X * torch.log(P + 1e-7) + (1 - X) * torch.log(1 - P + 1e-7)).sum()
            obj = value
    lp = -0.5 * sum(((q ** 2) / cfg.s2 + np.log(2 * np.pi * cfg.s2)).sum() for q in params)
    lz = -0.5 * (Z ** 2 + np.log(2 * np.pi)).sum() if latent == "point" else 0.0
    return value, obj + lp + lz


AUTOGRAD = [(lat, ot, act) for lat, ot in (("act", "se"), ("act", "binary"), ("act", "cont"), ("point", "se"))
            for act in ("tanh", "sigmoid", "relu")]


@pytest.mark.parametrize("latent,otype,act", AUTOGRAD, ids=["-".join(c) for c in AUTOGRAD])
def test_oracle_gradient_matches_autograd(latent, otype, act):
    cfg = A.AEConfig(Dobs=24, Denc=(10, 7), Dz=3, Ddec=(6, 9), otype=otype, act=act, s2=2.0)
    rng = np.random.default_rng(0)
    params = [(0.3 * rng.standard_normal(s)).astype(np.float64) for _, s in VA.param_shapes(cfg)]
    X = rng.random((7, cfg.Dobs))
    if otype == "binary":
        X = (X < 0.4).astype(np.float64)
    out = VA.forward_backward(params, X, cfg, latent)
    tp = [torch.tensor(q, requires_grad=True) for q in params]
    value, lj = torch_logjoint(tp, torch.tensor(X), cfg, latent)
    lj.backward()
    assert abs(out["value"] - value.item()) <= 1e-10 * max(1.0, abs(value.item()))
    assert abs(out["logjoint"] - lj.item()) <= 1e-10 * max(1.0, abs(lj.item()))
    for g, t in zip(out["grads"], tp):
        assert np.allclose(g, t.grad.numpy(), rtol=1e-9, atol=1e-11)


# ------------------------------------------------------------------ 2. the known value
def test_train_step_value_is_se_per_row_and_mse_matches():
    cfg = A.AEConfig(Dobs=12, Denc=(7,), Dz=3, Ddec=(5,), otype="se")
    rng = np.random.default_rng(3)
    params = [p.astype(np.float64) * 30 for p in VA.init_params(cfg, seed=7)]
    Xtr = rng.random((20, cfg.Dobs))
    idx = np.array([5, 2, 17, 9, 11])
    v, new_p, new_a, out = VA.train_step(params, [np.zeros_like(p) for p in params], Xtr, idx, cfg)
    X = Xtr[idx]
    se = float(((X - out["Xpr"]) ** 2).sum())
    assert v > 0 and abs(v - se / 5) <= 1e-14 * v
    assert abs(VA.mse(X, out["Xpr"]) - v) <= 1e-14 * v
    assert out["logjoint"] < -se                       # -se plus the (negative) log prior
    # AdaGrad ascends -se: a small step along the gradient lowers the error
    small = [p + 1e-4 * g for p, g in zip(params, out["data_grads"])]
    assert VA.forward_backward(small, X, cfg, need_grad=False)["value"] < out["value"]
    # the single-pixel case by hand: one row, everything zero -> Xpr = 1/2
    zero = [np.zeros_like(p) for p in params]
    x1 = np.full((1, cfg.Dobs), 0.25)
    o = VA.forward_backward(zero, x1, cfg)
    assert abs(o["value"] - cfg.Dobs * 0.0625) <= 1e-15
    g = dict(zip(VA.names(cfg), o["data_grads"]))
    assert np.allclose(g["bout"], 2 * (0.25 - 0.5) * 0.25)          # 2 r P (1 - P)


def test_layouts():
    cfg = A.AEConfig(Dobs=12, Denc=(7,), Dz=3, Ddec=(5,), otype="se")
    assert VA.param_shapes(cfg) == A.param_shapes(dataclasses.replace(cfg, otype="binary"))
    from vaeb_amd import ae
    mine = [s for _, s in ae.param_shapes(12, [7], 3, [5], "se", latent="act")]
    assert mine == [s for _, s in VA.param_shapes(cfg)]
    with pytest.raises(ValueError):
        ae.param_shapes(12, [7], 3, [5], "se", latent="other")


def test_arguments_are_checked_before_the_device():
    """gauss x se, iw_samples on an act context and the bad vaeb_ae_sq_error arguments are
    VAEB_ERR_ARG without a GPU; ConstructAE keeps to binary | cont; the driver's epoch rule."""
    import ctypes

    from vaeb_amd import _lib, ae, vanilla_ae
    assert (_lib.AE_SE, _lib.AE_LATENT["act"]) == (2, 3)           # latent 2 stays unassigned
    for kw in (dict(otype="se", latent="gauss"), dict(otype="se", latent="act", iw_samples=2)):
        with pytest.raises(_lib.VaebError, match=r"error -1\b"):
            _lib.AEContext(20, [9], 3, [8], max_batch=8, **kw)
    with pytest.raises(_lib.VaebError):
        _lib.AEContext(20, [9], 3, [8], otype="other")
    L = _lib.load()
    out = ctypes.c_double()
    assert L.vaeb_ae_sq_error(None, None, 0, ctypes.byref(out), None) == -1
    with pytest.raises(ValueError):
        ae.ConstructAE(np.zeros((4, 6), np.float32), otype="se")
    assert ae.mse(np.ones((2, 3)), np.zeros((2, 3))) == 3.0
    assert [vanilla_ae.frey_epochs(d) for d in (2, 10, 20)] == [100, 550, 550]


# ------------------------------------------------------------------ 3. the inputs are fair
@CASE_PARAMS
def test_inputs_are_fair(name, latent, otype, scaled):
    st = C.case(name, latent, otype, scaled)
    cfg, out = st.cfg, st.out64
    worst = max(st.bound, key=st.bound.get)
    print(f"{name}-{latent}-{otype}-{'x30' if scaled else 'theta0'} (seed {st.seed}): bound, largest {worst} "
          f"{st.bound[worst]:.1e}; value {st.restate_value:.1e}; max|Z| {np.abs(out['Z']).max():.3f}")
    assert max(st.bound.values()) <= G.GRAD_CAP, st.bound
    assert min(st.restate.values()) > 0                # a zero restatement error would ask for bit equality
    assert st.restate_value <= G.VALUE_RTOL / G.MARGIN
    assert st.Xtr.shape[0] > len(st.idx) == G.SHAPE[name].B
    assert not np.array_equal(st.idx, np.sort(st.idx)) or len(st.idx) == 1
    if otype == "se":
        assert st.value64 > 0
    Z = out["Z"]
    if scaled and latent == "act":
        if cfg.act == "tanh":
            assert (np.abs(Z) > 0.9).any()
        if cfg.act == "sigmoid":
            assert ((Z < 0.3) | (Z > 0.7)).any()
    if scaled:
        assert ((out["Xpr"] < 0.2) | (out["Xpr"] > 0.8)).any()
    if cfg.act == "relu":
        p64 = [p.astype(np.float64) for p in st.params]
        pre = np.concatenate([a.ravel() for a in C.preacts(cfg, latent, p64, out)])
        assert pre.size == sum(cfg.Denc) + sum(cfg.Ddec) + cfg.Dz
        assert np.abs(pre).min() >= G.KINK
        assert 0.2 <= (pre <= 0).mean() <= 0.8


def test_case_table_covers_what_it_claims():
    got = set(C.CASES)
    for n in C.SHAPE_NAMES:
        assert {(n, "act", "se", False), (n, "act", "se", True)} <= got
    assert ("edge_bin_tanh", "act", "binary", True) in got and ("edge_cont_sigmoid", "act", "cont", True) in got
    assert ("edge_bin_tanh", "point", "se", True) in got
    assert max(G.SHAPE[n].B for n in C.SHAPE_NAMES) == 513
    assert {G.SHAPE[n].cfg().act for n in C.SHAPE_NAMES} == {"tanh", "sigmoid", "relu"}


# ------------------------------------------------------------------ 4. wrong gradients are rejected
def applies(kind, latent, otype):
    if kind in ("latent_linear", "keep_minus_z"):
        return latent == "act"
    if kind.startswith("se_"):
        return otype == "se"
    return True


def rejected_on(kind):
    hits = []
    for (name, latent, otype, scaled), cid in zip(C.CASES, C.CASE_IDS):
        if not applies(kind, latent, otype):
            continue
        st = C.case(name, latent, otype, scaled)
        p64 = [p.astype(np.float64) for p in st.params]
        out = VA.forward_backward(p64, st.Xtr[st.idx].astype(np.float64), st.cfg, latent, wrong=kind)
        err = G.block_errors(dict(zip(VA.names(st.cfg), out["grads"])), st.g64)
        if G.rejected(err, st.bound):
            hits.append(cid)
    return hits


@pytest.mark.parametrize("kind", VA.WRONG)
def test_wrong_gradient_is_rejected(kind):
    hits = rejected_on(kind)
    print(f"{kind}: rejected on {len(hits)} cases")
    assert hits, kind


def test_nothing_wrong_is_accepted():
    for name, latent, otype, scaled in C.CASES:
        st = C.case(name, latent, otype, scaled)
        assert not G.rejected(G.block_errors(st.g64, st.g64), st.bound)
