"""NumPy oracle of the layer-stack engine's two-mode latent prior (include/vaeb_hip.h enum
vaeb_ae_prior, vaeb_amd/csrc/ae_mlp.hpp AePriorArgs) -- TEST HELPER ONLY, on top of
tests/vae_stack_oracle.py (parameters, noise keys) and tests/vae_stack_iwtrain_oracle.py (the stacked
sample planes), which it imports and leaves as they are.

Per latent dimension  p(z) = 1/2 N(z; 0, s^2) + 1/2 N(z; a, s^2),  c = 1 / s^2:

    t = a (2 z - a) c / 2      r = sigmoid(t)
    log p(z) = -1/2 log 2 pi - log(2 s) - 1/2 c z^2 + softplus(t)       dlog p / dz = -c (z - a r)

form "elbo" (eps [M, Dz]): the prior term at the step's sample, the entropy analytic
    latent = sum [1/2 (1 + lv) - log(2 s) - 1/2 c z^2 + softplus(t)]     value = loglik + latent
    g = dz - c (z - a r)      dmu = g      dlv = 1/2 g (z - mu) + 1/2
form "iw" (eps [K, M, Dz]): the K-sample importance-weighted bound
    lat_k = sum_j [1/2 eps^2 + 1/2 lv - log(2 s) - 1/2 c z^2 + softplus(t)]
    u = dz - wn c (z - a r)   dmu_k = u    dlv_k = 1/2 u (z - mu) + 1/2 wn

Both forms run on the stacked rows g = k M + m (the ELBO form: one plane, wn = 1).  a and s are the
float32 values the ABI carries; c and log(2 s) are formed from them in double and then take the
dtype of the run, as the host does for the launches.  The dtype of the computation is that of the
parameters (float64: the reference; float32: the restatement that sizes the GPU tests' bounds).
"""
import math

import numpy as np

from oracle import ae_oracle as A
from tests import vae_stack_iwtrain_oracle as T
from tests import vae_stack_oracle as V

FORMS = ("elbo", "iw")
# wrong kernels (tests/test_vae_prior_host.py): the responsibility dropped (r = 1: the pull is to a
# whatever z), a ignored (the prior N(0, s^2), value and gradient), c on z alone (c z - a r), the
# 1/2 wn of dlv_k left 1/2 (iw form), softplus as log(1 + e^t)
WRONG = ("r_dropped", "a_ignored", "c_on_z_alone", "half_not_half_wn", "naive_softplus")


def abi_prior(mean1, width):
    """(a, s) as the float32 values vaeb_ae_set_prior receives, in double."""
    return float(np.float32(mean1)), float(np.float32(width))


def softplus(t, naive=False):
    if naive:
        with np.errstate(over="ignore"):
            return np.log(1 + np.exp(t))
    return np.maximum(t, 0) + np.log(1 + np.exp(-np.abs(t)))


def sigmoid(t):
    e = np.exp(-np.abs(t))
    q = 1 / (1 + e)
    return np.where(t >= 0, q, e * q)


def prior_terms(z, mean1, width, wrong=None):
    """t, r, log p(z) + 1/2 log 2 pi and the pull c (z - a r) = -dlog p / dz, in z's dtype."""
    dt = z.dtype
    a64, s64 = abi_prior(mean1, width)
    a, c, log2s = dt.type(a64), dt.type(1.0 / (s64 * s64)), dt.type(math.log(2.0 * s64))
    half = dt.type(0.5)
    av = dt.type(0) if wrong == "a_ignored" else a
    t = half * av * (2 * z - av) * c
    r = np.ones_like(z) if wrong == "r_dropped" else sigmoid(t)
    logp = softplus(t, naive=wrong == "naive_softplus") - log2s - half * c * z * z
    pull = c * z - av * r if wrong == "c_on_z_alone" else c * (z - av * r)
    return t, r, logp, pull


def forward_backward(params, X, eps, cfg, mean1, width, form, need_grad=True, Y=None, wrong=None):
    """value (loglik + latent, or L_K), rows (iw), wn, t, r, mu / lv / z [K, M, Dz] and the gradient
    of value + NormalPrior(theta, s2) in theta order.  Y: the observations scored (default X: a
    corrupting step passes the clean rows as Y and the corrupted ones as X)."""
    assert form in FORMS and (wrong is None or wrong in WRONG)
    nm = V.names(cfg)
    p = dict(zip(nm, params))
    dt = params[0].dtype
    X, eps = np.asarray(X, dt), np.asarray(eps, dt)
    Y = X if Y is None else np.asarray(Y, dt)
    if form == "elbo":
        assert eps.ndim == 2
        eps = eps[None]
    K, M, Dz = eps.shape
    ne, nd = len(cfg.Denc), len(cfg.Ddec)
    half = dt.type(0.5)
    H = [X]
    for i in range(ne):
        H.append(A._act(cfg.act, H[-1] @ p[f"Wenc{i}"] + p[f"benc{i}"]))
    mu = H[-1] @ p["Wzmu"] + p["bzmu"]
    lv = H[-1] @ p["Wzlv"] + p["bzlv"]
    z = mu[None] + np.exp(lv * half)[None] * eps                   # [K, M, Dz]
    Zs = z.reshape(K * M, Dz)                                      # stacked row g = k M + m
    Ys = np.tile(Y, (K, 1))
    G = [Zs]
    for i in range(nd):
        G.append(A._act(cfg.act, G[-1] @ p[f"Wdec{i}"] + p[f"bdec{i}"]))
    e7 = dt.type(A.EPS_LOG)
    if cfg.otype == "binary":
        P = 1.0 / (1.0 + np.exp(-(G[-1] @ p["Wout"] + p["bout"])))
        ll = (Ys * np.log(P + e7) + (1 - Ys) * np.log(1 - P + e7)).sum(1)
        Xpr = P
    else:
        xm = 1.0 / (1.0 + np.exp(-(G[-1] @ p["Wmu"] + p["bmu"])))
        ls2 = G[-1] @ p["Wlogs2"] + p["blogs2"]
        rr = Ys - xm
        ll = (-0.5 * (A.LOG2PI + ls2 + rr * rr / np.exp(ls2))).sum(1)
        Xpr = xm
    t, r, logp, pull = prior_terms(z, mean1, width, wrong)
    out = dict(mu=mu, lv=lv, z=z, t=t, r=r, Xpr=Xpr, H=H, G=G)
    if form == "elbo":
        latent = float((half * (1 + lv) + logp[0]).sum(dtype=np.float64))
        loglik = float(ll.sum(dtype=np.float64))
        value = loglik + latent
        wn = np.ones((1, M), dt)
        out.update(loglik=loglik, latent=latent)
    else:
        lat = (half * (eps * eps + lv[None]) + logp).sum(2)        # [K, M]
        lw = (ll.reshape(K, M) + lat).astype(dt)
        mx = lw.max(0)
        e = np.exp(lw - mx)
        s = e.sum(0)
        rows = mx + np.log(s) - np.log(dt.type(K))
        wn = e / s
        value = float(rows.sum(dtype=np.float64))
        out.update(rows=rows, lw=lw, lat=lat)
    s2 = cfg.s2
    logprior = -0.5 * sum(float((q.astype(np.float64) ** 2 / s2 + math.log(2 * math.pi * s2)).sum()) for q in params)
    out.update(value=value, wn=wn, f=value + logprior)
    if not need_grad:
        return out

    ws = wn.reshape(K * M, 1).astype(dt)
    g = {}
    if cfg.otype == "binary":
        dP = Ys / (P + e7) - (1 - Ys) / (1 - P + e7)
        dA = dP * P * (1 - P) * ws
        g["Wout"], g["bout"] = G[-1].T @ dA, dA.sum(0)
        dG = dA @ p["Wout"].T
    else:
        ex = np.exp(-ls2)
        dAmu = rr * ex * xm * (1 - xm) * ws
        dAls = (-0.5 + 0.5 * rr * rr * ex) * ws
        g["Wmu"], g["bmu"] = G[-1].T @ dAmu, dAmu.sum(0)
        g["Wlogs2"], g["blogs2"] = G[-1].T @ dAls, dAls.sum(0)
        dG = dAmu @ p["Wmu"].T + dAls @ p["Wlogs2"].T
    for i in reversed(range(nd)):
        dPre = dG * A._dact(cfg.act, G[i + 1])
        g[f"Wdec{i}"], g[f"bdec{i}"] = G[i].T @ dPre, dPre.sum(0)
        dG = dPre @ p[f"Wdec{i}"].T
    u = dG - ws * pull.reshape(K * M, Dz)                          # dz - wn c (z - a r)
    dmu_k = u
    dlv_k = half * u * (Zs - np.tile(mu, (K, 1))) + (half if wrong == "half_not_half_wn" else half * ws)
    dmu = dmu_k.reshape(K, M, Dz).sum(0)                           # ascending k
    dlv = dlv_k.reshape(K, M, Dz).sum(0)
    g["Wzmu"], g["bzmu"] = H[-1].T @ dmu, dmu.sum(0)
    g["Wzlv"], g["bzlv"] = H[-1].T @ dlv, dlv.sum(0)
    dH = dmu @ p["Wzmu"].T + dlv @ p["Wzlv"].T
    for i in reversed(range(ne)):
        dPre = dH * A._dact(cfg.act, H[i + 1])
        g[f"Wenc{i}"], g[f"benc{i}"] = H[i].T @ dPre, dPre.sum(0)
        if i > 0:
            dH = dPre @ p[f"Wenc{i}"].T
    out["data_grads"] = [np.asarray(g[n]).astype(dt) for n in nm]
    out["grads"] = [(g[n] - p[n] / s2).astype(dt) for n in nm]
    return out


def train_step(params, acc, Xtr, idx, eps, cfg, mean1, width, form, Xenc=None):
    """One train(idx): (value / |idx|, theta', acc', aux).  Xenc: the encoder's input rows of a
    corrupting step (vaeb_ae_corrupt's), scored against the clean Xtr[idx]."""
    Y = Xtr[np.asarray(idx)]
    out = forward_backward(params, Y if Xenc is None else Xenc, eps, cfg, mean1, width, form, Y=Y)
    new_p, new_a = A.adagrad(params, acc, out["grads"], cfg.eta)
    return out["value"] / Y.shape[0], new_p, new_a, out


def train_eps(seed, idx, Dz, step, form, K=None):
    """The device's training noise of a step: the keys of the N(0, 1) context, unchanged."""
    return V.train_eps(seed, idx, Dz, step) if form == "elbo" else T.train_eps(seed, idx, Dz, step, K)
