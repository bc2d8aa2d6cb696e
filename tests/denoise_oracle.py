"""NumPy oracle of the layer-stack engine's denoising training (include/vaeb_hip.h
enum vaeb_ae_corruption, vaeb_amd/csrc/ae_corrupt.hpp, engine_ae.inc ae_step) -- TEST HELPER ONLY.

A corrupting step forms xt from the gathered rows X and a draw per element, feeds xt to the
encoder's first layer (forward and weight gradient) and scores the output on the clean X.  So the
oracle is the existing objective of each latent with two inputs in the place of one:

    Xin   the encoder's input rows (xt)
    Y     the observations the output layer scores (X)

The draws follow oracle/philox.py at the counter c0 = idx[m], c1 = 0x80000000 | d, c2, c3 = the
training domain at the step: r = (out2 >> 8) / 2^24, n = the latent normal (out0, out1).

forward_backward is oracle.ae_oracle.forward_backward with both given, for every latent and otype and
for the importance-weighted step (eps [K, M, Dz]); this file keeps the corruption's counters, draws and
corrupt().  The dtype of the computation is that of the parameters.
"""
import numpy as np

from oracle import ae_oracle as A
from oracle import philox

C1_CORRUPT = 0x80000000
KINDS = ("mask", "saltpepper", "gauss")
# the two wirings most likely to be got wrong: the first layer's weight gradient taken from the
# clean rows (the sweep with layer_grad substituted), and (the caller passes Y = Xin) the output scored
# on the corrupted rows
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


names = A.names


def init_params(cfg, latent, seed=15485863):
    return A.init_params(cfg, seed=seed, latent=latent)


def _first_grad_clean(f, w, inp, d, back=True):
    return A.layer_grad(f, w, f.Y if w == "Wenc0" else inp, d, back)


_SUBSTITUTED = {"first_grad_clean": dict(layer_grad=_first_grad_clean)}


def forward_backward(params, Xin, Y, cfg, latent, eps=None, need_grad=True, wrong=None):
    """The objective of `latent` ("point" | "act" | "gauss") and cfg.otype ("binary" | "cont" | "se")
    with the encoder fed Xin and the output scored on Y.  out["value"]: what train() reports before
    the division by M (loglik, loglik + negKL, or se)."""
    out = A.forward_backward(params, Xin, cfg, need_grad, latent=latent, Y=Y, eps=eps,
                             steps=wrong and _SUBSTITUTED[wrong])
    out.setdefault("negkl", 0.0)
    return out


def train_step(params, acc, Xin, Y, cfg, latent, eps=None, wrong=None):
    """One corrupting train(idx) on the gathered rows: (value / M, theta', acc', aux)."""
    res = A.step(params, acc, Xin, cfg, latent=latent, Y=Y, eps=eps, steps=wrong and _SUBSTITUTED[wrong])
    res[3].setdefault("negkl", 0.0)
    return res


def iw_train_step(params, acc, Xin, Y, eps, cfg):
    """The importance-weighted step (eps [K, M, Dz]) with the encoder fed Xin and every sample
    plane scored on Y: (L_K / M, theta', acc', aux)."""
    assert np.ndim(eps) == 3
    return A.step(params, acc, Xin, cfg, latent="gauss", Y=Y, eps=eps)
