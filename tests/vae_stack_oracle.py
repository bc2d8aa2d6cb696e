"""NumPy oracle of the layer-stack engine's Gaussian latent (include/vaeb_hip.h
enum vaeb_ae_latent, vaeb_amd/csrc/ae_mlp.hpp F_LATENT / B_LATENT) -- TEST HELPER ONLY.

The model, on gathered rows X [M x Dobs] with given eps [M x Dz] (H the last encoder activation):

    mu = H Wzmu + bzmu      lv = H Wzlv + bzlv      z = mu + exp(lv / 2) eps
    loglik = oracle.ae_oracle's output layer on the decoder fed with z
    negKL  = 1/2 sum (1 + lv - mu^2 - exp(lv))
    f      = loglik + negKL + NormalPrior(theta, s2);   train returns (loglik + negKL) / M

Activations, the output layers' formulas and AdaGrad are oracle.ae_oracle's; the dtype of the
computation is that of the parameters (float64 for the reference runs, float32 for the
tolerance-headroom runs).
"""
import math

import numpy as np

from oracle import ae_oracle as A
from oracle import philox

LATENT_NAMES = ("Wzmu", "Wzlv", "bzmu", "bzlv")
LV_NAMES = ("Wzlv", "bzlv")


def param_shapes(cfg):
    """oracle.ae_oracle.param_shapes with [Wz, bz] replaced, in place, by
    [Wzmu, Wzlv, bzmu, bzlv]."""
    out = []
    for n, s in A.param_shapes(cfg):
        if n == "Wz":
            out += [("Wzmu", s), ("Wzlv", s)]
        elif n == "bz":
            out += [("bzmu", s), ("bzlv", s)]
        else:
            out.append((n, s))
    return out


def names(cfg):
    return [n for n, _ in param_shapes(cfg)]


def init_params(cfg, seed=15485863, scale=0.01):
    rs = np.random.RandomState(seed)
    return [rs.normal(0.0, scale, size=s).astype(np.float32) for _, s in param_shapes(cfg)]


def flatten(params):
    return A.flatten(params)


def unflatten(flat, cfg):
    out, o = [], 0
    for _, s in param_shapes(cfg):
        n = int(np.prod(s))
        out.append(np.asarray(flat[o:o + n]).reshape(s))
        o += n
    return out


def from_point(point_params, cfg):
    """The Gaussian-latent parameters whose mu head is the point model's Z layer and whose lv
    head is zero."""
    p = dict(zip([n for n, _ in A.param_shapes(cfg)], point_params))
    out = []
    for n, s in param_shapes(cfg):
        if n in ("Wzmu", "bzmu"):
            out.append(p["Wz" if n == "Wzmu" else "bz"].copy())
        elif n in LV_NAMES:
            out.append(np.zeros(s, point_params[0].dtype))
        else:
            out.append(p[n].copy())
    return out


def forward_backward(params, X, eps, cfg, need_grad=True):
    """value pieces (loglik, negKL), mu / lv / z, Xpr and the gradient of f in theta order."""
    nm = names(cfg)
    p = dict(zip(nm, params))
    dt = params[0].dtype
    X, eps = np.asarray(X, dt), np.asarray(eps, dt)
    ne, nd = len(cfg.Denc), len(cfg.Ddec)
    H = [X]
    for i in range(ne):
        H.append(A._act(cfg.act, H[-1] @ p[f"Wenc{i}"] + p[f"benc{i}"]))
    mu = H[-1] @ p["Wzmu"] + p["bzmu"]
    lv = H[-1] @ p["Wzlv"] + p["bzlv"]
    z = mu + np.exp(lv * dt.type(0.5)) * eps
    G = [z]
    for i in range(nd):
        G.append(A._act(cfg.act, G[-1] @ p[f"Wdec{i}"] + p[f"bdec{i}"]))
    if cfg.otype == "binary":
        a = G[-1] @ p["Wout"] + p["bout"]
        P = 1.0 / (1.0 + np.exp(-a))
        loglik = float((X * np.log(P + dt.type(A.EPS_LOG)) + (1 - X) * np.log(1 - P + dt.type(A.EPS_LOG))).sum(dtype=np.float64))
        Xpr = P
    else:
        amu = G[-1] @ p["Wmu"] + p["bmu"]
        xm = 1.0 / (1.0 + np.exp(-amu))
        ls2 = G[-1] @ p["Wlogs2"] + p["blogs2"]
        r = X - xm
        loglik = float((-0.5 * (A.LOG2PI + ls2 + r * r / np.exp(ls2))).sum(dtype=np.float64))
        Xpr = xm
    negkl = float((0.5 * (1 + lv - mu * mu - np.exp(lv))).sum(dtype=np.float64))
    s2 = cfg.s2
    logprior = -0.5 * sum(float((q.astype(np.float64) ** 2 / s2 + math.log(2 * math.pi * s2)).sum()) for q in params)
    out = dict(loglik=loglik, negkl=negkl, elbo=loglik + negkl, f=loglik + negkl + logprior, mu=mu, lv=lv, z=z,
               Xpr=Xpr, H=H, G=G)
    if not need_grad:
        return out

    g = {}
    if cfg.otype == "binary":
        dP = X / (P + dt.type(A.EPS_LOG)) - (1 - X) / (1 - P + dt.type(A.EPS_LOG))
        dA = dP * P * (1 - P)
        g["Wout"], g["bout"] = G[-1].T @ dA, dA.sum(0)
        dG = dA @ p["Wout"].T
    else:
        e = np.exp(-ls2)
        dAmu = r * e * xm * (1 - xm)
        dAls = -0.5 + 0.5 * r * r * e
        g["Wmu"], g["bmu"] = G[-1].T @ dAmu, dAmu.sum(0)
        g["Wlogs2"], g["blogs2"] = G[-1].T @ dAls, dAls.sum(0)
        dG = dAmu @ p["Wmu"].T + dAls @ p["Wlogs2"].T
    for i in reversed(range(nd)):
        dPre = dG * A._dact(cfg.act, G[i + 1])
        g[f"Wdec{i}"], g[f"bdec{i}"] = G[i].T @ dPre, dPre.sum(0)
        dG = dPre @ p[f"Wdec{i}"].T
    dz = dG                                              # no "- Z": the KL replaces the Z prior
    dmu = dz - mu
    dlv = 0.5 * dz * (z - mu) + 0.5 * (1 - np.exp(lv))
    g["Wzmu"], g["bzmu"] = H[-1].T @ dmu, dmu.sum(0)
    g["Wzlv"], g["bzlv"] = H[-1].T @ dlv, dlv.sum(0)
    dH = dmu @ p["Wzmu"].T + dlv @ p["Wzlv"].T
    for i in reversed(range(ne)):
        dPre = dH * A._dact(cfg.act, H[i + 1])
        g[f"Wenc{i}"], g[f"benc{i}"] = H[i].T @ dPre, dPre.sum(0)
        if i > 0:
            dH = dPre @ p[f"Wenc{i}"].T
    out["data_grads"] = [g[n].astype(dt) for n in nm]
    out["grads"] = [(g[n] - p[n] / s2).astype(dt) for n in nm]
    return out


def train_step(params, acc, Xtr, idx, eps, cfg):
    """One train(idx): returns ((loglik + negKL) / |idx|, theta', acc', aux)."""
    X = Xtr[np.asarray(idx)]
    out = forward_backward(params, X, eps, cfg)
    new_p, new_a = A.adagrad(params, acc, out["grads"], cfg.eta)
    return out["elbo"] / X.shape[0], new_p, new_a, out


def train_eps(seed, idx, Dz, step):
    """The device's training noise: keyed by the dataset row idx[m], c1 = j, domain 0."""
    idx = np.asarray(idx, np.int64)
    return philox.latent_normal(seed, idx[:, None], np.arange(Dz, dtype=np.int64)[None, :], step, 0)
