"""NumPy oracle of the layer-stack engine's training step on the importance-weighted bound
(include/vaeb_hip.h vaeb_ae_config.iw_samples, vaeb_amd/csrc/engine_ae.inc ae_step / ae_iw_forward) -- TEST
HELPER ONLY, on top of tests/vae_stack_oracle.py and tests/vae_stack_iw_oracle.py.

On gathered rows X [M x Dobs] with eps [K, M, Dz], mu and lv once per row:

    z_k     = mu + exp(lv / 2) eps_k
    log w_k = loglik_row(x | z_k) + 1/2 sum_j (eps_kj^2 + lv_j - z_kj^2)
    L_K     = sum_m [logsumexp_k log w_mk - log K]
    f       = L_K + NormalPrior(theta, s2);   train returns L_K / M

    grad f  = sum_m sum_k wn_mk grad log w_mk - theta / s2,   wn_mk = w_mk / sum_k' w_mk'

It is oracle.ae_oracle.forward_backward with eps of three dimensions: the backward runs on the K M
stacked rows (g = k M + m) with the output deltas scaled by wn, as the device does;
test_vae_stack_iwtrain_host.py pins it to float64 torch autograd of L_K.  This file keeps the device's
training noise and WRONG, the sweep with one step substituted.
"""
import numpy as np

from oracle import ae_oracle as A
from oracle import philox
from tests import vae_stack_iw_oracle as W


def _batch_normalised(f):
    eb = np.exp(f.lw - f.lw.max())
    return eb / eb.sum() * f.M


def _latent(minus_wz=True, half_w=True, analytic_kl=False):
    """oracle.ae_oracle's sampled-latent deltas with terms left out, or the ELBO step's put in."""
    def deltas(f, dG):
        K, M, Dz = f.K, f.M, f.cfg.Dz
        u = dG - f.ws * f.Z if minus_wz else dG                   # weighted delta into z, minus wn z
        dlv_k = f.half * u * (f.Z - np.tile(f.mu, (K, 1)))
        if half_w:
            dlv_k = dlv_k + f.half * f.ws
        dmu, dlv = u.reshape(K, M, Dz).sum(0), dlv_k.reshape(K, M, Dz).sum(0)
        if analytic_kl:
            dmu, dlv = dmu - f.mu, dlv + f.half * (1 - np.exp(f.lv))
        return [("Wzmu", dmu), ("Wzlv", dlv)]
    return deltas


# wrong backwards: wn = 1 / K; wn normalised over the batch instead of per row; the -wn z term
# missing; the 1/2 wn term missing; the ELBO step's analytic-KL terms (-mu, 1/2 (1 - e^lv)) in the
# place of the latent term's
_SUBSTITUTED = {
    "uniform_weights": dict(wn=lambda f: np.full_like(f.wn, 1.0 / f.K)),
    "batch_normalised": dict(wn=_batch_normalised),
    "no_minus_wz": dict(latent_deltas=_latent(minus_wz=False)),
    "no_half_w": dict(latent_deltas=_latent(half_w=False)),
    "analytic_kl": dict(latent_deltas=_latent(minus_wz=False, half_w=False, analytic_kl=True)),
}
WRONG = tuple(_SUBSTITUTED)


def forward_backward(params, X, eps, cfg, need_grad=True, Y=None, wrong=None):
    """L_K (iw), the row values, wn [K, M], log w, mu / lv / z and the gradient of f in theta order.
    Y: the observations the output layer scores (default X; a test of the gather passes others).
    wrong: one of WRONG, a deliberately wrong backward (test_vae_stack_iwtrain_host.py)."""
    assert np.ndim(eps) == 3
    return A.forward_backward(params, X, cfg, need_grad, latent="gauss", Y=Y, eps=eps,
                              steps=wrong and _SUBSTITUTED[wrong])


def train_step(params, acc, Xtr, idx, eps, cfg):
    """One train(idx) with iw_samples = eps.shape[0]: returns (L_K / |idx|, theta', acc', aux)."""
    assert np.ndim(eps) == 3
    return A.train_step(params, acc, Xtr, idx, cfg, latent="gauss", eps=eps)


def train_eps(seed, idx, Dz, step, K):
    """The device's training noise [K, M, Dz]: sample k of dataset row idx[m] at c0 = idx[m], c1 = j,
    the training domain with sample stream k (domain k << 1)."""
    idx = np.asarray(idx, np.int64)
    j = np.arange(Dz, dtype=np.int64)[None, :]
    return np.stack([philox.latent_normal(seed, idx[:, None], j, step, k << 1) for k in range(K)])


def marginal_rows(params, X, eps, cfg):
    """tests/vae_stack_iw_oracle.py's row values for the same eps (the two files agree)."""
    return W.iw_rows(params, X, eps, cfg)
