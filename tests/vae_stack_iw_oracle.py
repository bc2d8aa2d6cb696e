"""NumPy oracle of the layer-stack engine's importance-weighted bound (include/vaeb_hip.h
vaeb_ae_marginal_ll, vaeb_amd/csrc/ae_iwae.hpp) -- TEST HELPER ONLY.

Per row of X and sample k, on top of tests/vae_stack_oracle.py's forward pass fed eps[k] (one
M-row forward per sample, as the device evaluates; its per-row log-likelihood is the forward's "ll"):

    log w_k = loglik_row(x | z_k) + 1/2 sum_j (eps_kj^2 + lv_j - z_kj^2)
    IW_K(x) = logsumexp_k log w_k - log K

The dtype of the computation is that of the parameters.
"""
import numpy as np

from oracle import ae_oracle as A
from tests import vae_stack_oracle as V


def log_weights(params, X, eps, cfg):
    """eps [K, n, Dz] -> dict of lw, ll, lat (each [K, n]), the forward results per sample
    (outs) and mu, lv [n, Dz]."""
    dt = params[0].dtype
    eps = np.asarray(eps, dt)
    ll, lat, outs = [], [], []
    for e in eps:
        out = V.forward_backward(params, X, e, cfg, need_grad=False)
        z, lv = out["z"], out["lv"]
        ll.append(out["ll"])
        lat.append(dt.type(0.5) * (e * e + lv - z * z).sum(1))
        outs.append(out)
    ll, lat = np.stack(ll), np.stack(lat)
    return dict(lw=ll + lat, ll=ll, lat=lat, outs=outs, mu=outs[0]["mu"], lv=outs[0]["lv"])


def iw_from_lw(lw):
    """[n]: max-subtracted logsumexp over the K samples minus log K, in lw's dtype."""
    return A.logsumexp_rows(lw)[0]


def iw_rows(params, X, eps, cfg):
    return iw_from_lw(log_weights(params, X, eps, cfg)["lw"])
