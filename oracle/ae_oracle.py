"""CPU oracle for the layer-stack engine's training step -- TEST INFRASTRUCTURE ONLY.

NumPy restatement of /root/reference/degenerate-vae (Python 2 + Theano, not runnable
here) and of the objectives built on its graph, used to CHECK the HIP layer-stack engine
(vaeb_amd/csrc/ae_mlp.hpp, engine_ae.inc); the product path never imports it.

  * ae.py:41-117 ConstructAE: encoder MLP (mlp.py:66-74 ConstructMLP, f = tanh), linear
    latent Z = Hz Wz + bz (ae.py:49), decoder MLP, output layer by otype (ae.py:58-73),
    logjoint = loglik + NormalPrior(theta, s2) + NormalPrior([Z], 1) (ae.py:77-78),
    train(idx) returns loglik / |idx| over the gathered rows Xtr[idx] (ae.py:82-89).
  * mlp.py:36-49 WeightMatrix / BiasVector: N(0, 0.01) draws (std 0.01) from the GLOBAL
    numpy RandomState, in construction order; mlp.py:87-91 ConstructNormalPrior.
  * logpdf.py:46-47 OutToProbs (sigmoid), :72-73 OutToReal, :85-86 bernoulli with the
    1e-7 inside both logs, :112-114 indep_normal.
  * infalg.py:148-164 AdaGrad.construct: g = dlogjoint/dtheta; g_ac += g^2;
    theta += eta g / (sqrt(g_ac) + 1e-6).

Pinning: the logpdf.py:119-123 known answer (tests/test_oracle_pins.py); the gradient of
this restatement is checked against float64 torch autograd (tests/test_ae_oracle.py).
Bitwise Theano behaviour is "parity unpinned" (see DESIGN.md).

ONE forward and ONE reverse sweep serve every objective of the engine (forward_backward):

    latent   "point"  Z = Hz Wz + bz with the N(0, 1) prior on Z          theta [.., Wz, bz, ..]
             "act"    Z = f(Hz Wz + bz), no prior on Z (the vanilla-ae)   theta [.., Wz, bz, ..]
             "gauss"  mu, lv heads, z = mu + exp(lv / 2) eps              theta [.., Wzmu, Wzlv, bzmu, bzlv, ..]
    otype    "binary" | "cont" | "se" (sum (Y - Xpr)^2; theta tail of "binary")
    X, Y     the encoder's input rows and the observations the output scores (default X)
    eps      [M, Dz]: one sample, the ELBO with the analytic KL (normal prior) or the prior term at the
             sample and the analytic entropy (two-mode prior);  [K, M, Dz]: the K-sample
             importance-weighted bound, decoder and backward on the stacked rows g = k M + m
    prior    None (N(0, 1)) or (mean1, width): 1/2 N(0, s^2) + 1/2 N(a, s^2) per latent dimension

The reverse sweep is built from named steps (STEPS): out_deltas, latent_deltas, layer_grad, dact, wn
and prior_terms.  `steps` replaces any of them: a deliberately wrong gradient is this sweep with one
step substituted, and is defined beside the host test that uses it (tests/*_oracle.py WRONG,
tests/test_ae_grads_host.py), never here.  The dtype of the computation is that of the parameters:
the float32 restatement of a step is the same code fed float32 arrays.
"""
from __future__ import annotations

import dataclasses
import math
import types

import numpy as np

LOG2PI = math.log(2.0 * math.pi)
EPS_LOG = 1e-7   # logpdf.py:86
LATENTS = ("point", "act", "gauss")


@dataclasses.dataclass
class AEConfig:
    Dobs: int
    Denc: tuple = (500,)
    Dz: int = 20
    Ddec: tuple = (500,)
    otype: str = "binary"      # "binary" | "cont" (ae.py:58-73) | "se" (vanilla-ae)
    s2: float = 1.0            # prior variance on theta (ae.py:41)
    eta: float = 0.01          # AdaGrad(0.01)
    act: str = "tanh"          # f (ae.py:41)


# ------------------------------------------------------------------ theta
def layout(cfg):
    """cfg with the otype whose theta tail it has (se: binary's [Wout, bout])."""
    return dataclasses.replace(cfg, otype="binary") if cfg.otype == "se" else cfg


def param_shapes(cfg: AEConfig, latent="point"):
    """theta order (ae.py:51,56,64,72): Wenc..., benc..., the latent layer ([Wz, bz], or
    [Wzmu, Wzlv, bzmu, bzlv] under "gauss"), Wdec..., bdec..., then [Wout, bout] (binary, se) or
    [Wmu, Wlogs2, bmu, blogs2] (cont)."""
    assert latent in LATENTS
    denc, ddec = list(cfg.Denc), list(cfg.Ddec)
    d_in = [cfg.Dobs] + denc
    shp = [(f"Wenc{i}", (d_in[i], d_in[i + 1])) for i in range(len(denc))]
    shp += [(f"benc{i}", (denc[i],)) for i in range(len(denc))]
    wz, bz = (denc[-1], cfg.Dz), (cfg.Dz,)
    if latent == "gauss":
        shp += [("Wzmu", wz), ("Wzlv", wz), ("bzmu", bz), ("bzlv", bz)]
    else:
        shp += [("Wz", wz), ("bz", bz)]
    d_dec = [cfg.Dz] + ddec
    shp += [(f"Wdec{i}", (d_dec[i], d_dec[i + 1])) for i in range(len(ddec))]
    shp += [(f"bdec{i}", (ddec[i],)) for i in range(len(ddec))]
    if cfg.otype == "cont":
        shp += [("Wmu", (ddec[-1], cfg.Dobs)), ("Wlogs2", (ddec[-1], cfg.Dobs)),
                ("bmu", (cfg.Dobs,)), ("blogs2", (cfg.Dobs,))]
    else:
        shp += [("Wout", (ddec[-1], cfg.Dobs)), ("bout", (cfg.Dobs,))]
    return shp


def names(cfg, latent="point"):
    return [n for n, _ in param_shapes(cfg, latent)]


def init_params(cfg: AEConfig, seed=15485863, scale=0.01, latent="point"):
    """Draws in construction order, which is theta order, from numpy's global-style RandomState
    (ae.py:48-72): every weight AND bias ~ N(0, 0.01) (mlp.py:39,49), float32."""
    rs = np.random.RandomState(seed)
    return [rs.normal(0.0, scale, size=s).astype(np.float32) for _, s in param_shapes(cfg, latent)]


def flatten(params):
    return np.concatenate([np.asarray(p, np.float32).ravel() for p in params])


def unflatten(flat, cfg: AEConfig, latent="point"):
    out, o = [], 0
    for _, s in param_shapes(cfg, latent):
        n = int(np.prod(s))
        out.append(np.asarray(flat[o:o + n]).reshape(s))
        o += n
    return out


# ------------------------------------------------------------------ pieces of the forward
def _act(name, a):
    if name == "tanh":
        return np.tanh(a)
    if name == "sigmoid":
        return 1.0 / (1.0 + np.exp(-a))
    if name == "relu":
        return np.maximum(a, 0.0)
    raise ValueError(name)


def _dact(name, h):
    """Derivative in terms of the activation output h."""
    if name == "tanh":
        return 1.0 - h * h
    if name == "sigmoid":
        return h * (1.0 - h)
    if name == "relu":
        return (h > 0).astype(h.dtype)
    raise ValueError(name)


def abi_prior(mean1, width):
    """(a, s) of the two-mode prior as the float32 values the C ABI carries, in double."""
    return float(np.float32(mean1)), float(np.float32(width))


def prior_constants(dt, mean1, width):
    """a, c = 1 / s^2 and log(2 s): formed in double from the ABI's floats, then in the run's dtype."""
    a64, s64 = abi_prior(mean1, width)
    return dt.type(a64), dt.type(1.0 / (s64 * s64)), dt.type(math.log(2.0 * s64))


def softplus(t):
    return np.maximum(t, 0) + np.log(1 + np.exp(-np.abs(t)))


def stable_sigmoid(t):
    e = np.exp(-np.abs(t))
    q = 1 / (1 + e)
    return np.where(t >= 0, q, e * q)


def prior_terms(z, mean1, width):
    """The two-mode prior p(z) = 1/2 N(z; 0, s^2) + 1/2 N(z; a, s^2) per dimension, in z's dtype:
    t = a (2 z - a) c / 2, r = sigmoid(t), log p(z) + 1/2 log 2 pi = softplus(t) - log(2 s) - c z^2 / 2
    and the pull c (z - a r) = -dlog p / dz."""
    a, c, log2s = prior_constants(z.dtype, mean1, width)
    half = z.dtype.type(0.5)
    t = half * a * (2 * z - a) * c
    r = stable_sigmoid(t)
    return t, r, softplus(t) - log2s - half * c * z * z, c * (z - a * r)


def logsumexp_rows(lw):
    """lw [K, M] -> (max-subtracted logsumexp over the K samples minus log K [M], the normalised
    weights wn [K, M]), in lw's dtype."""
    mx = lw.max(0)
    e = np.exp(lw - mx)
    s = e.sum(0)
    return mx + np.log(s) - np.log(lw.dtype.type(lw.shape[0])), e / s


# ------------------------------------------------------------------ the steps of the reverse sweep
# Each takes the forward's state f first (see forward_backward for its fields).
def out_deltas(f):
    """[(W, d objective / d pre-activation)] of the output layer's heads, scaled by the sample weights."""
    Y, P, r = f.Ys, f.Xpr, f.r
    if f.cfg.otype == "cont":
        e = np.exp(-f.ls2)
        return [("Wmu", r * e * P * (1 - P) * f.ws), ("Wlogs2", (-0.5 + 0.5 * r * r * e) * f.ws)]
    if f.cfg.otype == "se":                                  # d(-se)/da = 2 (Y - P) P (1 - P)
        dA = 2.0 * r
        return [("Wout", dA * P * (1 - P) * f.ws)]
    dP = Y / (P + f.e7) - (1 - Y) / (1.0 - P + f.e7)
    return [("Wout", dP * P * (1 - P) * f.ws)]


def _point_deltas(f, dG):
    return [("Wz", dG - f.Z)]                                # + d/dZ of NormalPrior([Z], 1)


def _act_deltas(f, dG):
    return [("Wz", dG * f.dact(f.Z, f.Zpre))]               # no prior on the activated code


def _gauss_kl_deltas(f, dG):
    """One sample, the analytic KL in the place of the Z prior."""
    dmu = dG - f.mu
    dlv = 0.5 * dG * (f.Z - f.mu) + 0.5 * (1 - np.exp(f.lv))
    return [("Wzmu", dmu), ("Wzlv", dlv)]


def _gauss_sample_deltas(f, dG):
    """The prior term at the samples (K planes of the importance-weighted bound, or the two-mode
    ELBO's one plane with wn = 1): u = dz - wn pull, dlv_k = 1/2 u (z - mu) + 1/2 wn, summed over
    k ascending."""
    K, M, Dz = f.K, f.M, f.cfg.Dz
    u = dG - f.ws * f.pull
    dlv_k = f.half * u * (f.Z - np.tile(f.mu, (K, 1))) + f.half * f.ws
    return [("Wzmu", u.reshape(K, M, Dz).sum(0)), ("Wzlv", dlv_k.reshape(K, M, Dz).sum(0))]


LATENT_DELTAS = {"point": _point_deltas, "act": _act_deltas, "gauss_kl": _gauss_kl_deltas,
                 "gauss_sample": _gauss_sample_deltas}


def latent_deltas(f, dG):
    """[(W, delta)] of the latent layer's heads from dG, the delta into the decoder's input rows."""
    return LATENT_DELTAS[f.objective](f, dG)


def layer_grad(f, w, inp, d, back=True):
    """(dW, db, delta into the layer's input -- None unless back) of the layer with weights w."""
    return inp.T @ d, d.sum(0), d @ f.p[w].T if back else None


def dact(f, h, a):
    """f' of a hidden (or activated latent) layer from its output h; a is its pre-activation."""
    return _dact(f.cfg.act, h)


def wn(f):
    """The sample weights [K, M] the backward scales the output deltas by."""
    return f.wn


STEPS = dict(out_deltas=out_deltas, latent_deltas=latent_deltas, layer_grad=layer_grad, dact=dact, wn=wn,
             prior_terms=prior_terms)


# ------------------------------------------------------------------ the one forward and backward
def forward_backward(params, X, cfg: AEConfig, need_grad=True, *, latent="point", Y=None, eps=None, prior=None,
                     steps=None):
    """One evaluation of the graph on gathered rows X and the reverse-mode gradient of
    f = objective + NormalPrior(theta, s2) in theta order (module docstring: latent, Y, eps, prior, steps).

    Returns H, G (activations, G[0] = Z the decoder's input rows), Hpre, Gpre, Xpr, ll (the output
    layer's value per row), wn, value (what train() reports before the division by M), f = logjoint,
    grads, data_grads, and by objective: data = loglik | se (summed forms), Zpre (point, act), mu, lv, z
    (gauss), negkl, elbo (normal-prior ELBO), latent, t, r (two-mode), lat, lw, rows, iw (K samples)."""
    assert latent in LATENTS and cfg.otype in ("binary", "cont", "se")
    assert not (latent == "gauss" and cfg.otype == "se") and (prior is None or latent == "gauss")
    S = dict(STEPS, **(steps or {}))
    nm = names(cfg, latent)
    p = dict(zip(nm, params))
    dt = params[0].dtype
    X = np.asarray(X, dt)
    Y = X if Y is None else np.asarray(Y, dt)
    M, Dz = X.shape[0], cfg.Dz
    ne, nd = len(cfg.Denc), len(cfg.Ddec)
    half, e7 = dt.type(0.5), dt.type(EPS_LOG)
    f = types.SimpleNamespace(cfg=cfg, latent=latent, p=p, dt=dt, M=M, K=1, Y=Y, half=half, e7=e7)
    f.dact = lambda h, a: S["dact"](f, h, a)

    H, Hpre = [X], []
    for i in range(ne):
        Hpre.append(H[-1] @ p[f"Wenc{i}"] + p[f"benc{i}"])
        H.append(_act(cfg.act, Hpre[-1]))
    out = dict(H=H, Hpre=Hpre)
    if latent == "gauss":
        eps = np.asarray(eps, dt)
        samples = eps.ndim == 3                                      # the importance-weighted form
        eps3 = eps if samples else eps[None]
        f.K = K = eps3.shape[0]
        f.mu = mu = H[-1] @ p["Wzmu"] + p["bzmu"]
        f.lv = lv = H[-1] @ p["Wzlv"] + p["bzlv"]
        z = mu[None] + np.exp(lv * half)[None] * eps3                # [K, M, Dz]
        f.Z = z.reshape(K * M, Dz)                                   # stacked row g = k M + m
        f.objective = "gauss_sample" if samples or prior is not None else "gauss_kl"
        out.update(mu=mu, lv=lv, z=z.reshape(eps.shape))
    else:
        samples, K = False, 1
        f.Zpre = H[-1] @ p["Wz"] + p["bz"]
        f.Z = _act(cfg.act, f.Zpre) if latent == "act" else f.Zpre   # vanilla-ae ae.py:55
        f.objective = latent
        out.update(Zpre=f.Zpre)
    f.Ys = Ys = np.tile(Y, (K, 1))
    G, Gpre = [f.Z], []
    for i in range(nd):
        Gpre.append(G[-1] @ p[f"Wdec{i}"] + p[f"bdec{i}"])
        G.append(_act(cfg.act, Gpre[-1]))

    # the output layer: L, the objective's data term per element (se: its negative)
    if cfg.otype == "cont":
        f.Xpr = 1.0 / (1.0 + np.exp(-(G[-1] @ p["Wmu"] + p["bmu"])))
        f.ls2 = G[-1] @ p["Wlogs2"] + p["blogs2"]
        f.r = Ys - f.Xpr
        L = -0.5 * (LOG2PI + f.ls2 + f.r * f.r / np.exp(f.ls2))
    else:
        f.Xpr = P = 1.0 / (1.0 + np.exp(-(G[-1] @ p["Wout"] + p["bout"])))   # vanilla-ae ae.py:66
        f.r = Ys - P
        L = f.r * f.r if cfg.otype == "se" else Ys * np.log(P + e7) + (1 - Ys) * np.log(1.0 - P + e7)
    ll = L.sum(1)
    out.update(Z=f.Z, G=G, Gpre=Gpre, Xpr=f.Xpr, ll=ll)

    # the latent's term and the value
    f.wn = np.ones((K, M), dt)
    f.pull, zprior = f.Z, 0.0
    if prior is not None:
        t, r, logp, pull = S["prior_terms"](z, *prior)
        f.pull = pull.reshape(K * M, Dz)
        out.update(t=t.reshape(eps.shape), r=r.reshape(eps.shape))
    if samples:
        if prior is None:
            lat = half * (eps * eps + lv[None] - z * z).sum(2)       # [K, M]
        else:
            lat = (half * (eps * eps + lv[None]) + logp).sum(2)
        lw = (ll.reshape(K, M) + lat).astype(dt)
        rows, f.wn = logsumexp_rows(lw)
        f.lw = lw
        value = float(rows.sum(dtype=np.float64))
        out.update(lat=lat, lw=lw, rows=rows, iw=value)
    else:
        if prior is None:
            data = float(L.sum(dtype=np.float64))
        else:
            data = float(ll.sum(dtype=np.float64))
        out["data"] = out["se" if cfg.otype == "se" else "loglik"] = value = data
        if latent == "point":
            zprior = -0.5 * float((f.Z.astype(np.float64) ** 2 + LOG2PI).sum())
        elif latent == "gauss" and prior is None:
            negkl = float((0.5 * (1 + lv - mu * mu - np.exp(lv))).sum(dtype=np.float64))
            value = data + negkl
            out.update(negkl=negkl, elbo=value)
        elif latent == "gauss":
            out["latent"] = float((half * (1 + lv) + logp[0]).sum(dtype=np.float64))
            value = data + out["latent"]
    s2 = cfg.s2
    logprior = -0.5 * sum(float((q.astype(np.float64) ** 2 / s2 + math.log(2 * math.pi * s2)).sum()) for q in params)
    obj = -value if cfg.otype == "se" else value                     # vanilla-ae ae.py:72
    out.update(wn=f.wn, value=value)
    out["f"] = out["logjoint"] = obj + logprior + zprior
    if not need_grad:
        return out

    f.ws = S["wn"](f).reshape(K * M, 1).astype(dt)
    g = {}

    def back(heads, inp, need_in=True):
        """The gradients of the layer's heads; the sum of their deltas into inp."""
        dIn = None
        for w, d in heads:
            g[w], g["b" + w[1:]], d_in = S["layer_grad"](f, w, inp, d, need_in)
            dIn = d_in if dIn is None else dIn + d_in
        return dIn

    dG = back(S["out_deltas"](f), G[-1])
    for i in reversed(range(nd)):
        dG = back([(f"Wdec{i}", dG * f.dact(G[i + 1], Gpre[i]))], G[i])
    dH = back(S["latent_deltas"](f, dG), H[-1])
    for i in reversed(range(ne)):
        dH = back([(f"Wenc{i}", dH * f.dact(H[i + 1], Hpre[i]))], H[i], i > 0)
    out["data_grads"] = [np.asarray(g[n]).astype(dt) for n in nm]
    out["grads"] = [(g[n] - p[n] / s2).astype(dt) for n in nm]
    return out


def adagrad(params, acc, grads, eta):
    """infalg.py:148-164."""
    new_p, new_a = [], []
    for th, a, g in zip(params, acc, grads):
        a2 = a + g * g
        new_p.append((th + eta * g / (np.sqrt(a2) + 1e-6)).astype(th.dtype))
        new_a.append(a2.astype(th.dtype))
    return new_p, new_a


def step(params, acc, X, cfg: AEConfig, **kw):
    """One AdaGrad ascent on gathered rows X (kw: forward_backward's): (value / M, theta', acc', aux)."""
    out = forward_backward(params, X, cfg, **kw)
    new_p, new_a = adagrad(params, acc, out["grads"], cfg.eta)
    return out["value"] / X.shape[0], new_p, new_a, out


def train_step(params, acc, Xtr, idx, cfg: AEConfig, **kw):
    """train(idx) (ae.py:82-89): returns (value / |idx|, theta', acc', aux)."""
    return step(params, acc, Xtr[np.asarray(idx)], cfg, **kw)


def epoch_batches(Ntr, batch_size, rs):
    """LearnMNIST / LearnFreyFace epoch loop (ae.py:140-151): a fresh permutation per epoch,
    batches of batch_size with the last partial batch KEPT."""
    idx = rs.permutation(np.arange(Ntr)).astype(np.int32)
    return [idx[lb:min(lb + batch_size, Ntr)] for lb in range(0, Ntr, batch_size)]


def rmse(X, Xpr):
    """ae.py:121-122."""
    return float(np.sqrt(np.mean(np.sum((X - Xpr) ** 2, 1))))
