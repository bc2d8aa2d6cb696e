"""The vanilla squared-error autoencoder step on oracle/ae_oracle.py -- TEST HELPER ONLY.

The reference's vanilla-ae/ae.py, used to CHECK the layer-stack engine's VAEB_AE_SE output and
VAEB_AE_LATENT_ACT latent (vaeb_amd/csrc/ae_mlp.hpp, engine_ae.inc); the product path never imports it.

  * ae.py:52-56  encoder MLP, then the code Z = f(Hz Wz + bz): the latent goes through f
                 (latent "act"; "point" is the degenerate-vae's linear Z with its N(0, 1) prior).
  * ae.py:59-68  decoder MLP, Xpr = sigmoid(Hx Wout + bout), se = sum (X - Xpr)^2 (otype "se").
  * ae.py:71-72  logjoint = -se + NormalPrior(theta, s2)   (no prior on Z under "act").
  * ae.py:75-83  train(idx): AdaGrad ascends logjoint on the rows Xtr[idx] and returns se / |idx|.
  * ae.py:120-121 mse(X, Xpr) = mean over rows of sum_d (X - Xpr)^2.

The forward, the backward and the theta layout are oracle.ae_oracle's (latent "act" | "point", otype
"se" | "binary" | "cont"); this file keeps mse and WRONG, the sweep with one step substituted
(tests/test_vanilla_ae_host.py shows that each is rejected by the bounds of the GPU test):
  latent_linear    the activated latent's f'(Z) left out
  keep_minus_z     the - Z of the N(0, 1) prior kept on the activated latent
  se_no_2          the factor 2 of the squared-error delta dropped
  se_sign          the squared-error delta's sign flipped (descending -se)
  se_no_pq         the sigmoid's P (1 - P) dropped from the squared-error delta
  early_update     every layer's AdaGrad update (from a zero accumulator) applied before the data
                   gradient reads its weights
"""
import numpy as np

from oracle import ae_oracle as A
from oracle.ae_oracle import adagrad, epoch_batches, init_params, layout, names, param_shapes  # noqa: F401


def _early_update(f, w, inp, d, back=True):
    gw, gb, _ = A.layer_grad(f, w, inp, d, back=False)
    W, dt = f.p[w], f.dt
    (w1,), _ = adagrad([W], [np.zeros_like(W)], [(gw - W / f.cfg.s2).astype(dt)], np.asarray(f.cfg.eta, dt))
    return gw, gb, d @ w1.T if back else None


_SUBSTITUTED = {
    "latent_linear": dict(latent_deltas=lambda f, dG: [("Wz", dG)]),
    "keep_minus_z": dict(latent_deltas=lambda f, dG: [("Wz", dG * f.dact(f.Z, f.Zpre) - f.Z)]),
    "se_no_2": dict(out_deltas=lambda f: [("Wout", 1.0 * f.r * f.Xpr * (1 - f.Xpr))]),
    "se_sign": dict(out_deltas=lambda f: [("Wout", -(2.0 * f.r * f.Xpr * (1 - f.Xpr)))]),
    "se_no_pq": dict(out_deltas=lambda f: [("Wout", 2.0 * f.r)]),
    "early_update": dict(layer_grad=_early_update),
}
WRONG = tuple(_SUBSTITUTED)


def forward_backward(params, X, cfg, latent="act", need_grad=True, wrong=None):
    """oracle.ae_oracle.forward_backward; out["value"] is what train() reports before the division by
    M: se (otype "se", positive) or loglik.  wrong: one of WRONG."""
    assert latent in ("act", "point")
    return A.forward_backward(params, X, cfg, need_grad, latent=latent, steps=wrong and _SUBSTITUTED[wrong])


def train_step(params, acc, Xtr, idx, cfg, latent="act"):
    """train(idx) (ae.py:75-83): (value / |idx|, theta', acc', aux); value = se under otype "se"."""
    return A.train_step(params, acc, Xtr, idx, cfg, latent=latent)


def mse(X, Xpr):
    """ae.py:120-121."""
    return float(np.mean(np.sum((X - Xpr) ** 2, 1)))
