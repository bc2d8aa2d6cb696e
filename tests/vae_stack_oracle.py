"""NumPy oracle of the layer-stack engine's Gaussian latent (include/vaeb_hip.h
enum vaeb_ae_latent, vaeb_amd/csrc/ae_mlp.hpp F_LATENT / B_LATENT) -- TEST HELPER ONLY.

The model, on gathered rows X [M x Dobs] with given eps [M x Dz] (H the last encoder activation):

    mu = H Wzmu + bzmu      lv = H Wzlv + bzlv      z = mu + exp(lv / 2) eps
    loglik = oracle.ae_oracle's output layer on the decoder fed with z
    negKL  = 1/2 sum (1 + lv - mu^2 - exp(lv))
    f      = loglik + negKL + NormalPrior(theta, s2);   train returns (loglik + negKL) / M

The forward, the backward and AdaGrad are oracle.ae_oracle's (latent "gauss", eps [M, Dz]); this file
keeps the names of the Gaussian-latent theta, from_point and the device's training noise.  The dtype
of the computation is that of the parameters (float64 for the reference runs, float32 for the
tolerance-headroom runs).
"""
import functools

import numpy as np

from oracle import ae_oracle as A
from oracle import philox

LATENT_NAMES = ("Wzmu", "Wzlv", "bzmu", "bzlv")
LV_NAMES = ("Wzlv", "bzlv")

# oracle.ae_oracle's theta with [Wz, bz] replaced, in place, by [Wzmu, Wzlv, bzmu, bzlv]
param_shapes = functools.partial(A.param_shapes, latent="gauss")
names = functools.partial(A.names, latent="gauss")
init_params = functools.partial(A.init_params, latent="gauss")
unflatten = functools.partial(A.unflatten, latent="gauss")
flatten = A.flatten


def from_point(point_params, cfg):
    """The Gaussian-latent parameters whose mu head is the point model's Z layer and whose lv
    head is zero."""
    p = dict(zip(A.names(cfg), point_params))
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
    return A.forward_backward(params, X, cfg, need_grad, latent="gauss", eps=eps)


def train_step(params, acc, Xtr, idx, eps, cfg):
    """One train(idx): returns ((loglik + negKL) / |idx|, theta', acc', aux)."""
    return A.train_step(params, acc, Xtr, idx, cfg, latent="gauss", eps=eps)


def train_eps(seed, idx, Dz, step):
    """The device's training noise: keyed by the dataset row idx[m], c1 = j, domain 0."""
    idx = np.asarray(idx, np.int64)
    return philox.latent_normal(seed, idx[:, None], np.arange(Dz, dtype=np.int64)[None, :], step, 0)
