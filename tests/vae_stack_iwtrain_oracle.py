"""NumPy oracle of the layer-stack engine's training step on the importance-weighted bound
(include/vaeb_hip.h vaeb_ae_config.iw_samples, vaeb_amd/csrc/engine_ae.inc ae_step / ae_iw_forward) -- TEST
HELPER ONLY, on top of tests/vae_stack_oracle.py and tests/vae_stack_iw_oracle.py.

On gathered rows X [M x Dobs] with eps [K, M, Dz], mu and lv once per row:

    z_k     = mu + exp(lv / 2) eps_k
    log w_k = loglik_row(x | z_k) + 1/2 sum_j (eps_kj^2 + lv_j - z_kj^2)
    L_K     = sum_m [logsumexp_k log w_mk - log K]
    f       = L_K + NormalPrior(theta, s2);   train returns L_K / M

    grad f  = sum_m sum_k wn_mk grad log w_mk - theta / s2,   wn_mk = w_mk / sum_k' w_mk'

The backward runs on the K M stacked rows (g = k M + m) with the output deltas scaled by wn, as the
device does; test_vae_stack_iwtrain_host.py pins it to float64 torch autograd of L_K.  The dtype of
the computation is that of the parameters.
"""
import math

import numpy as np

from oracle import ae_oracle as A
from oracle import philox
from tests import vae_stack_iw_oracle as W
from tests import vae_stack_oracle as V


# wrong backwards: wn = 1 / K; wn normalised over the batch instead of per row; the -wn z term
# missing; the 1/2 wn term missing; the ELBO step's analytic-KL terms (-mu, 1/2 (1 - e^lv)) in the
# place of the latent term's
WRONG = ("uniform_weights", "batch_normalised", "no_minus_wz", "no_half_w", "analytic_kl")


def forward_backward(params, X, eps, cfg, need_grad=True, Y=None, wrong=None):
    """L_K (iw), the row values, wn [K, M], log w, mu / lv / z and the gradient of f in theta order.
    Y: the observations the output layer scores (default X; a test of the gather passes others).
    wrong: one of WRONG, a deliberately wrong backward (test_vae_stack_iwtrain_host.py)."""
    assert wrong is None or wrong in WRONG
    nm = V.names(cfg)
    p = dict(zip(nm, params))
    dt = params[0].dtype
    X, eps = np.asarray(X, dt), np.asarray(eps, dt)
    Y = X if Y is None else np.asarray(Y, dt)
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
        r = Ys - xm
        ll = (-0.5 * (A.LOG2PI + ls2 + r * r / np.exp(ls2))).sum(1)
        Xpr = xm
    lat = half * (eps * eps + lv[None] - z * z).sum(2)             # [K, M]
    lw = (ll.reshape(K, M) + lat).astype(dt)
    mx = lw.max(0)
    e = np.exp(lw - mx)
    s = e.sum(0)
    rows = mx + np.log(s) - np.log(dt.type(K))
    wn = e / s
    iw = float(rows.sum(dtype=np.float64))
    s2 = cfg.s2
    logprior = -0.5 * sum(float((q.astype(np.float64) ** 2 / s2 + math.log(2 * math.pi * s2)).sum()) for q in params)
    out = dict(iw=iw, rows=rows, wn=wn, lw=lw, f=iw + logprior, mu=mu, lv=lv, z=z, Xpr=Xpr, H=H, G=G)
    if not need_grad:
        return out

    if wrong == "uniform_weights":
        wn = np.full_like(wn, 1.0 / K)
    elif wrong == "batch_normalised":
        eb = np.exp(lw - lw.max())
        wn = eb / eb.sum() * M
    ws = wn.reshape(K * M, 1).astype(dt)
    g = {}
    if cfg.otype == "binary":
        dP = Ys / (P + e7) - (1 - Ys) / (1 - P + e7)
        dA = dP * P * (1 - P) * ws
        g["Wout"], g["bout"] = G[-1].T @ dA, dA.sum(0)
        dG = dA @ p["Wout"].T
    else:
        ex = np.exp(-ls2)
        dAmu = r * ex * xm * (1 - xm) * ws
        dAls = (-0.5 + 0.5 * r * r * ex) * ws
        g["Wmu"], g["bmu"] = G[-1].T @ dAmu, dAmu.sum(0)
        g["Wlogs2"], g["blogs2"] = G[-1].T @ dAls, dAls.sum(0)
        dG = dAmu @ p["Wmu"].T + dAls @ p["Wlogs2"].T
    for i in reversed(range(nd)):
        dPre = dG * A._dact(cfg.act, G[i + 1])
        g[f"Wdec{i}"], g[f"bdec{i}"] = G[i].T @ dPre, dPre.sum(0)
        dG = dPre @ p[f"Wdec{i}"].T
    u = dG if wrong in ("no_minus_wz", "analytic_kl") else dG - ws * Zs   # weighted delta into z, minus wn z
    dmu_k = u
    dlv_k = half * u * (Zs - np.tile(mu, (K, 1)))
    if wrong not in ("no_half_w", "analytic_kl"):
        dlv_k = dlv_k + half * ws
    dmu = dmu_k.reshape(K, M, Dz).sum(0)                           # ascending k
    dlv = dlv_k.reshape(K, M, Dz).sum(0)
    if wrong == "analytic_kl":                                     # the ELBO step's terms left in
        dmu = dmu - mu
        dlv = dlv + half * (1 - np.exp(lv))
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


def train_step(params, acc, Xtr, idx, eps, cfg):
    """One train(idx) with iw_samples = eps.shape[0]: returns (L_K / |idx|, theta', acc', aux)."""
    X = Xtr[np.asarray(idx)]
    out = forward_backward(params, X, eps, cfg)
    new_p, new_a = A.adagrad(params, acc, out["grads"], cfg.eta)
    return out["iw"] / X.shape[0], new_p, new_a, out


def train_eps(seed, idx, Dz, step, K):
    """The device's training noise [K, M, Dz]: sample k of dataset row idx[m] at c0 = idx[m], c1 = j,
    the training domain with sample stream k (domain k << 1)."""
    idx = np.asarray(idx, np.int64)
    j = np.arange(Dz, dtype=np.int64)[None, :]
    return np.stack([philox.latent_normal(seed, idx[:, None], j, step, k << 1) for k in range(K)])


def marginal_rows(params, X, eps, cfg):
    """tests/vae_stack_iw_oracle.py's row values for the same eps (the two files agree)."""
    return W.iw_rows(params, X, eps, cfg)
