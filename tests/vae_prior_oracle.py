"""NumPy oracle of the layer-stack engine's two-mode latent prior (include/vaeb_hip.h enum
vaeb_ae_prior, vaeb_amd/csrc/ae_mlp.hpp AePriorArgs) -- TEST HELPER ONLY: oracle.ae_oracle.forward_backward
with prior = (mean1, width), the parameters and noise keys of tests/vae_stack_oracle.py and
tests/vae_stack_iwtrain_oracle.py.

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
import functools

import numpy as np

from oracle import ae_oracle as A
from oracle.ae_oracle import abi_prior, stable_sigmoid as sigmoid  # noqa: F401
from tests import vae_stack_iwtrain_oracle as T
from tests import vae_stack_oracle as V

FORMS = ("elbo", "iw")
# wrong kernels (tests/test_vae_prior_host.py): the responsibility dropped (r = 1: the pull is to a
# whatever z), a ignored (the prior N(0, s^2), value and gradient), c on z alone (c z - a r), the
# 1/2 wn of dlv_k left 1/2 (iw form), softplus as log(1 + e^t)
WRONG = ("r_dropped", "a_ignored", "c_on_z_alone", "half_not_half_wn", "naive_softplus")


def softplus(t, naive=False):
    if naive:
        with np.errstate(over="ignore"):
            return np.log(1 + np.exp(t))
    return A.softplus(t)


def prior_terms(z, mean1, width, wrong=None):
    """oracle.ae_oracle.prior_terms (t, r, log p(z) + 1/2 log 2 pi, the pull c (z - a r)), with one
    thing wrong in it."""
    if wrong == "a_ignored":
        return A.prior_terms(z, 0.0, width)
    t, r, logp, pull = A.prior_terms(z, mean1, width)
    a, c, log2s = A.prior_constants(z.dtype, mean1, width)
    if wrong == "r_dropped":
        r = np.ones_like(z)
        pull = c * (z - a * r)
    elif wrong == "naive_softplus":
        logp = softplus(t, naive=True) - log2s - z.dtype.type(0.5) * c * z * z
    elif wrong == "c_on_z_alone":
        pull = c * z - a * r
    return t, r, logp, pull


def _half_not_half_wn(f, dG):
    K, M, Dz = f.K, f.M, f.cfg.Dz
    u = dG - f.ws * f.pull
    dlv_k = f.half * u * (f.Z - np.tile(f.mu, (K, 1))) + f.half
    return [("Wzmu", u.reshape(K, M, Dz).sum(0)), ("Wzlv", dlv_k.reshape(K, M, Dz).sum(0))]


def substituted(wrong):
    """The steps of the sweep that `wrong` replaces."""
    if wrong == "half_not_half_wn":
        return dict(latent_deltas=_half_not_half_wn)
    return dict(prior_terms=functools.partial(prior_terms, wrong=wrong))


def forward_backward(params, X, eps, cfg, mean1, width, form, need_grad=True, Y=None, wrong=None):
    """value (loglik + latent, or L_K), rows (iw), wn, t, r, mu / lv / z [K, M, Dz] and the gradient
    of value + NormalPrior(theta, s2) in theta order.  Y: the observations scored (default X: a
    corrupting step passes the clean rows as Y and the corrupted ones as X)."""
    assert form in FORMS and (wrong is None or wrong in WRONG)
    assert np.ndim(eps) == (2 if form == "elbo" else 3)
    out = A.forward_backward(params, X, cfg, need_grad, latent="gauss", Y=Y, eps=eps, prior=(mean1, width),
                             steps=wrong and substituted(wrong))
    for k in ("z", "t", "r"):                                      # the ELBO form's one plane
        out[k] = out[k].reshape((-1,) + out[k].shape[-2:])
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
