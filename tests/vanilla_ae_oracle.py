"""CPU oracle for the vanilla squared-error autoencoder step -- TEST HELPER ONLY.

NumPy restatement of the reference's vanilla-ae/ae.py, written from the maths, used to CHECK the
layer-stack engine's VAEB_AE_SE output and VAEB_AE_LATENT_ACT latent (vaeb_amd/csrc/ae_mlp.hpp,
engine_ae.inc); the product path never imports it.

  * ae.py:52-56  encoder MLP, then the code Z = f(Hz Wz + bz): the latent goes through f
                 (latent "act"; "point" is the degenerate-vae's linear Z with its N(0, 1) prior).
  * ae.py:59-68  decoder MLP, Xpr = sigmoid(Hx Wout + bout), se = sum (X - Xpr)^2 (otype "se";
                 "binary" and "cont" are the degenerate-vae outputs of oracle/ae_oracle.py).
  * ae.py:71-72  logjoint = -se + NormalPrior(theta, s2)   (no prior on Z under "act").
  * ae.py:75-83  train(idx): AdaGrad ascends logjoint on the rows Xtr[idx] and returns se / |idx|.
  * ae.py:120-121 mse(X, Xpr) = mean over rows of sum_d (X - Xpr)^2.

cfg is an oracle.ae_oracle.AEConfig whose otype may also be "se"; the theta layout of "se" is the
binary one ([Wout, bout]) and the layout of latent "act" is the point one ([Wz, bz]).  The functions
are dtype-generic: the float32 restatement of a step is the same code fed float32 arrays.

`wrong` makes one thing wrong in the gradient (tests/test_vanilla_ae_host.py shows that each is
rejected by the bounds of the GPU test):
  latent_linear    the activated latent's f'(Z) left out
  keep_minus_z     the - Z of the N(0, 1) prior kept on the activated latent
  se_no_2          the factor 2 of the squared-error delta dropped
  se_sign          the squared-error delta's sign flipped (descending -se)
  se_no_pq         the sigmoid's P (1 - P) dropped from the squared-error delta
  early_update     every layer's AdaGrad update (from a zero accumulator) applied before the data
                   gradient reads its weights
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from oracle import ae_oracle as A
from oracle.ae_oracle import _act, _dact, adagrad, epoch_batches, init_params as _init, param_shapes as _shapes

WRONG = ("latent_linear", "keep_minus_z", "se_no_2", "se_sign", "se_no_pq", "early_update")


def layout(cfg):
    """cfg with the otype whose theta tail it has (se: binary's [Wout, bout])."""
    return dataclasses.replace(cfg, otype="binary") if cfg.otype == "se" else cfg


def param_shapes(cfg):
    return _shapes(layout(cfg))


def init_params(cfg, seed=15485863):
    return _init(layout(cfg), seed=seed)


def names(cfg):
    return [n for n, _ in param_shapes(cfg)]


def forward_backward(params, X, cfg, latent="act", need_grad=True, wrong=None):
    """One evaluation of the graph on gathered rows X and the reverse-mode gradient of logjoint in
    theta order.  out["value"] is what train() reports before the division by M: se (otype "se",
    positive) or loglik."""
    assert latent in ("act", "point") and cfg.otype in ("se", "binary", "cont")
    assert wrong is None or wrong in WRONG
    nm = names(cfg)
    p = dict(zip(nm, params))
    dt = params[0].dtype
    X = np.asarray(X, dt)
    ne, nd = len(cfg.Denc), len(cfg.Ddec)
    H = [X]
    for i in range(ne):
        H.append(_act(cfg.act, H[-1] @ p[f"Wenc{i}"] + p[f"benc{i}"]))
    az = H[-1] @ p["Wz"] + p["bz"]
    Z = _act(cfg.act, az) if latent == "act" else az          # ae.py:55
    G = [Z]
    for i in range(nd):
        G.append(_act(cfg.act, G[-1] @ p[f"Wdec{i}"] + p[f"bdec{i}"]))
    out = dict(H=H, Z=Z, Zpre=az, G=G)
    if cfg.otype == "cont":
        mu = 1.0 / (1.0 + np.exp(-(G[-1] @ p["Wmu"] + p["bmu"])))
        ls2 = G[-1] @ p["Wlogs2"] + p["blogs2"]
        r = X - mu
        value = float((-0.5 * (A.LOG2PI + ls2 + r * r / np.exp(ls2))).sum(dtype=np.float64))
        obj, P = value, mu
    else:
        P = 1.0 / (1.0 + np.exp(-(G[-1] @ p["Wout"] + p["bout"])))   # ae.py:66
        r = X - P
        if cfg.otype == "se":
            value = float((r * r).sum(dtype=np.float64))             # ae.py:67
            obj = -value                                             # ae.py:72
        else:
            value = float((X * np.log(P + A.EPS_LOG) + (1 - X) * np.log(1.0 - P + A.EPS_LOG)).sum(dtype=np.float64))
            obj = value
    out["Xpr"], out["value"] = P, value
    out["se" if cfg.otype == "se" else "loglik"] = value
    s2 = cfg.s2
    logprior = -0.5 * sum(float((q.astype(np.float64) ** 2 / s2 + math.log(2 * math.pi * s2)).sum()) for q in params)
    zprior = -0.5 * float((Z.astype(np.float64) ** 2 + A.LOG2PI).sum()) if latent == "point" else 0.0
    out["logjoint"] = obj + logprior + zprior
    if not need_grad:
        return out

    g = {}
    eta = np.asarray(cfg.eta, dt)

    def put(w, b, inp, d):
        """The layer's gradient; returns the weights its data gradient reads."""
        g[w], g[b] = inp.T @ d, d.sum(0)
        if wrong != "early_update":
            return p[w]
        gw = (g[w] - p[w] / s2).astype(dt)
        (w1,), _ = adagrad([p[w]], [np.zeros_like(p[w])], [gw], eta)
        return w1

    if cfg.otype == "cont":
        e = np.exp(-ls2)
        dmu, dls = r * e * mu * (1 - mu), -0.5 + 0.5 * r * r * e
        dG = dmu @ put("Wmu", "bmu", G[-1], dmu).T + dls @ put("Wlogs2", "blogs2", G[-1], dls).T
    else:
        if cfg.otype == "se":                                        # d(-se)/da = 2 (X - P) P (1 - P)
            dA = (1.0 if wrong == "se_no_2" else 2.0) * r
            if wrong != "se_no_pq":
                dA = dA * P * (1 - P)
            if wrong == "se_sign":
                dA = -dA
        else:
            dA = (X / (P + A.EPS_LOG) - (1 - X) / (1.0 - P + A.EPS_LOG)) * P * (1 - P)
        dG = dA @ put("Wout", "bout", G[-1], dA).T
    for i in reversed(range(nd)):
        dPre = dG * _dact(cfg.act, G[i + 1])
        dG = dPre @ put(f"Wdec{i}", f"bdec{i}", G[i], dPre).T
    if latent == "act":
        dZ = dG if wrong == "latent_linear" else dG * _dact(cfg.act, Z)
        if wrong == "keep_minus_z":
            dZ = dZ - Z
    else:
        dZ = dG - Z
    dH = dZ @ put("Wz", "bz", H[-1], dZ).T
    for i in reversed(range(ne)):
        dPre = dH * _dact(cfg.act, H[i + 1])
        w = put(f"Wenc{i}", f"benc{i}", H[i], dPre)
        if i > 0:
            dH = dPre @ w.T
    out["data_grads"] = [g[n].astype(dt) for n in nm]
    out["grads"] = [(g[n] - p[n] / s2).astype(dt) for n in nm]
    return out


def train_step(params, acc, Xtr, idx, cfg, latent="act"):
    """train(idx) (ae.py:75-83): (value / |idx|, theta', acc', aux); value = se under otype "se"."""
    X = Xtr[np.asarray(idx)]
    out = forward_backward(params, X, cfg, latent)
    new_p, new_a = adagrad(params, acc, out["grads"], cfg.eta)
    return out["value"] / X.shape[0], new_p, new_a, out


def mse(X, Xpr):
    """ae.py:120-121."""
    return float(np.mean(np.sum((X - Xpr) ** 2, 1)))


__all__ = ["WRONG", "layout", "param_shapes", "init_params", "names", "forward_backward", "train_step", "mse",
           "epoch_batches", "adagrad"]
