"""NumPy oracle of the layer-stack engine's denoising training (include/vaeb_hip.h
enum vaeb_ae_corruption, vaeb_amd/csrc/ae_corrupt.hpp, engine_ae.inc ae_step) -- TEST HELPER ONLY.

A corrupting step forms xt from the gathered rows X and a draw per element, feeds xt to the
encoder's first layer (forward and weight gradient) and scores the output on the clean X.  So the
oracle is the existing objective of each latent with two inputs in the place of one:

    Xin   the encoder's input rows (xt)
    Y     the observations the output layer scores (X)

The draws follow oracle/philox.py at the counter c0 = idx[m], c1 = 0x80000000 | d, c2, c3 = the
training domain at the step: r = (out2 >> 8) / 2^24, n = the latent normal (out0, out1).

forward_backward is written operation by operation as oracle.ae_oracle (POINT), tests.vanilla_ae_oracle
(POINT / ACT, every otype) and tests.vae_stack_oracle (GAUSS): with Xin is Y it returns their numbers
exactly (tests/test_denoise_host.py).  The importance-weighted step is
tests.vae_stack_iwtrain_oracle.forward_backward(..., Y=...) as it stands.  The dtype of the computation
is that of the parameters.
"""
import math

import numpy as np

from oracle import ae_oracle as A
from oracle import philox
from tests import vae_stack_iwtrain_oracle as T
from tests import vae_stack_oracle as V
from tests import vanilla_ae_oracle as N

C1_CORRUPT = 0x80000000
KINDS = ("mask", "saltpepper", "gauss")
# the two wirings most likely to be got wrong: the first layer's weight gradient taken from the
# clean rows, and (the caller passes Y = Xin) the output scored on the corrupted rows
WRONG = ("first_grad_clean",)


def corruption_words(seed, row, c1, step):
    """The four Philox output words (uint64 arrays) at (row, c1, the training domain at step)."""
    s = philox._u64(seed)
    return philox.philox4x32_10(*philox.latent_counters(row, c1, step, 0), s & philox.M32, s >> np.uint64(32))


def corruption_counters(idx, Dobs, step):
    """The counter words, each [len(idx), Dobs], of one step's corruption draws."""
    idx = np.asarray(idx, np.int64)
    c1 = (C1_CORRUPT | np.arange(Dobs, dtype=np.int64))[None, :]
    return philox.latent_counters(idx[:, None], c1, step, 0)


def corruption_draws(seed, idx, Dobs, step):
    """(r, n), each float64 [len(idx), Dobs]: the uniform on the 2^-24 grid and the standard normal of
    element (m, d)."""
    idx = np.asarray(idx, np.int64)
    c1 = (C1_CORRUPT | np.arange(Dobs, dtype=np.int64))[None, :]
    w = corruption_words(seed, idx[:, None], c1, step)
    r = (w[2] >> np.uint64(8)).astype(np.float64) / 16777216.0
    n = philox.latent_normal(seed, idx[:, None], c1, step, 0)
    return r, n


def corrupt(X, kind, level, draw):
    """xt in the dtype of X; level is rounded to float32 first (the C ABI's float), draw holds r
    (mask, saltpepper) or n (gauss)."""
    assert kind in KINDS
    X = np.asarray(X)
    dt = X.dtype
    p = dt.type(np.float32(level))
    d = np.asarray(draw, dt)
    if kind == "gauss":
        return (X + p * d).astype(dt)
    if kind == "mask":
        return np.where(d < p, dt.type(0), X)
    return np.where(d < p * dt.type(0.5), dt.type(0), np.where(d < p, dt.type(1), X))


def names(cfg, latent):
    return V.names(cfg) if latent == "gauss" else N.names(cfg)


def init_params(cfg, latent, seed=15485863):
    return V.init_params(cfg, seed=seed) if latent == "gauss" else N.init_params(cfg, seed=seed)


def forward_backward(params, Xin, Y, cfg, latent, eps=None, need_grad=True, wrong=None):
    """The objective of `latent` ("point" | "act" | "gauss") and cfg.otype ("binary" | "cont" | "se")
    with the encoder fed Xin and the output scored on Y.  out["value"]: what train() reports before
    the division by M (loglik, loglik + negKL, or se)."""
    assert latent in ("point", "act", "gauss") and cfg.otype in ("binary", "cont", "se")
    assert not (latent == "gauss" and cfg.otype == "se")
    assert wrong is None or wrong in WRONG
    nm = names(cfg, latent)
    p = dict(zip(nm, params))
    dt = params[0].dtype
    e7 = dt.type(A.EPS_LOG)
    Xin, Y = np.asarray(Xin, dt), np.asarray(Y, dt)
    ne, nd = len(cfg.Denc), len(cfg.Ddec)
    H = [Xin]
    for i in range(ne):
        H.append(A._act(cfg.act, H[-1] @ p[f"Wenc{i}"] + p[f"benc{i}"]))
    negkl = 0.0
    if latent == "gauss":
        eps = np.asarray(eps, dt)
        mu = H[-1] @ p["Wzmu"] + p["bzmu"]
        lv = H[-1] @ p["Wzlv"] + p["bzlv"]
        Z = mu + np.exp(lv * dt.type(0.5)) * eps
        negkl = float((0.5 * (1 + lv - mu * mu - np.exp(lv))).sum(dtype=np.float64))
    else:
        az = H[-1] @ p["Wz"] + p["bz"]
        Z = A._act(cfg.act, az) if latent == "act" else az
    G = [Z]
    for i in range(nd):
        G.append(A._act(cfg.act, G[-1] @ p[f"Wdec{i}"] + p[f"bdec{i}"]))
    if cfg.otype == "cont":
        xm = 1.0 / (1.0 + np.exp(-(G[-1] @ p["Wmu"] + p["bmu"])))
        ls2 = G[-1] @ p["Wlogs2"] + p["blogs2"]
        r = Y - xm
        data = float((-0.5 * (A.LOG2PI + ls2 + r * r / np.exp(ls2))).sum(dtype=np.float64))
        obj, P = data, xm
    else:
        P = 1.0 / (1.0 + np.exp(-(G[-1] @ p["Wout"] + p["bout"])))
        r = Y - P
        if cfg.otype == "se":
            data = float((r * r).sum(dtype=np.float64))
            obj = -data
        else:
            data = float((Y * np.log(P + e7) + (1 - Y) * np.log(1.0 - P + e7)).sum(dtype=np.float64))
            obj = data
    s2 = cfg.s2
    logprior = -0.5 * sum(float((q.astype(np.float64) ** 2 / s2 + math.log(2 * math.pi * s2)).sum()) for q in params)
    zprior = -0.5 * float((Z.astype(np.float64) ** 2 + A.LOG2PI).sum()) if latent == "point" else 0.0
    out = dict(H=H, Z=Z, G=G, Xpr=P, data=data, negkl=negkl, value=data + negkl,
               f=obj + negkl + logprior + zprior)
    if not need_grad:
        return out

    g = {}
    if cfg.otype == "cont":
        e = np.exp(-ls2)
        dAmu = r * e * xm * (1 - xm)
        dAls = -0.5 + 0.5 * r * r * e
        g["Wmu"], g["bmu"] = G[-1].T @ dAmu, dAmu.sum(0)
        g["Wlogs2"], g["blogs2"] = G[-1].T @ dAls, dAls.sum(0)
        dG = dAmu @ p["Wmu"].T + dAls @ p["Wlogs2"].T
    else:
        if cfg.otype == "se":
            dA = 2.0 * r
            dA = dA * P * (1 - P)
        else:
            dP = Y / (P + e7) - (1 - Y) / (1.0 - P + e7)
            dA = dP * P * (1 - P)
        g["Wout"], g["bout"] = G[-1].T @ dA, dA.sum(0)
        dG = dA @ p["Wout"].T
    for i in reversed(range(nd)):
        dPre = dG * A._dact(cfg.act, G[i + 1])
        g[f"Wdec{i}"], g[f"bdec{i}"] = G[i].T @ dPre, dPre.sum(0)
        dG = dPre @ p[f"Wdec{i}"].T
    if latent == "gauss":
        dz = dG
        dmu = dz - mu
        dlv = 0.5 * dz * (Z - mu) + 0.5 * (1 - np.exp(lv))
        g["Wzmu"], g["bzmu"] = H[-1].T @ dmu, dmu.sum(0)
        g["Wzlv"], g["bzlv"] = H[-1].T @ dlv, dlv.sum(0)
        dH = dmu @ p["Wzmu"].T + dlv @ p["Wzlv"].T
    else:
        dZ = dG * A._dact(cfg.act, Z) if latent == "act" else dG - Z
        g["Wz"], g["bz"] = H[-1].T @ dZ, dZ.sum(0)
        dH = dZ @ p["Wz"].T
    for i in reversed(range(ne)):
        dPre = dH * A._dact(cfg.act, H[i + 1])
        first_in = Y if (i == 0 and wrong == "first_grad_clean") else H[i]
        g[f"Wenc{i}"], g[f"benc{i}"] = first_in.T @ dPre, dPre.sum(0)
        if i > 0:
            dH = dPre @ p[f"Wenc{i}"].T
    out["data_grads"] = [g[n].astype(dt) for n in nm]
    out["grads"] = [(g[n] - p[n] / s2).astype(dt) for n in nm]
    return out


def train_step(params, acc, Xin, Y, cfg, latent, eps=None, wrong=None):
    """One corrupting train(idx) on the gathered rows: (value / M, theta', acc', aux)."""
    out = forward_backward(params, Xin, Y, cfg, latent, eps, wrong=wrong)
    new_p, new_a = A.adagrad(params, acc, out["grads"], cfg.eta)
    return out["value"] / Y.shape[0], new_p, new_a, out


def iw_train_step(params, acc, Xin, Y, eps, cfg):
    """The importance-weighted step (eps [K, M, Dz]) with the encoder fed Xin and every sample
    plane scored on Y: (L_K / M, theta', acc', aux)."""
    out = T.forward_backward(params, Xin, eps, cfg, Y=Y)
    new_p, new_a = A.adagrad(params, acc, out["grads"], cfg.eta)
    return out["iw"] / Y.shape[0], new_p, new_a, out
