"""One training step per decoder-launch form (latent.hpp decout_z_body) against the CPU oracle
(oracle/vaeb_oracle.py, float64) on identical theta / x / host-injected eps, at the smallest
shapes that reach the edges of the launch's prologue and main loop.

Which kernel a shape selects (engine_f32.inc: enc_form / ho_mode, enqueue_forward,
launch_decout_z):
  * the encoder hand-off goes by the fan-in ceil(H / 16): above 16 (H > 256) the encoder only
    stores its [mu | lv] slabs and the decoder sums them (AT = 2, `ZM 2`); up to 16 it is the
    counted atomics and the decoder forms z from mu, lv, eps in memory (AT = 1);
  * a Bernoulli decoder runs decout_z2_kernel (two 16-column tiles per workgroup), a Gaussian
    one decout_z_kernel<2, ..> (two output planes, one tile, the 128-VGPR cap);
  * ZS = ceil(Z / 4) rounded up to 1 / 2 / 4 / 5 / 8 latent quads; V1 (16-byte W1 / b1 loads)
    needs H % 4 == 0.

  slab_partial_k     D=33 H=500 Z=20 B=100: decout_z2_kernel<5, true, 2>.  The slab form; the
                     last K block is partial (448..499); rows 100..111 are padding (rowok false:
                     the tanh select); of the two workgroup columns the last one's first tile
                     has one column (32) and its second lies wholly past D.
  atomic_idle_waves  D=40 H=72 Z=20 B=20: decout_z2_kernel<5, true, 1>.  The atomic form; waves
                     2-7 are epilogue waves without a K block (64 * wave >= H), wave 1's block
                     is partial (64..71).
  scalar_w1          D=36 H=70 Z=3 B=17: decout_z2_kernel<1, false, 1>.  H % 4 != 0: the scalar
                     W1 / b1 loads and hd stores; one latent quad; row block 1 is one valid row
                     and 15 padded ones.
  gauss_cap          D=24 H=40 Z=2 B=17 Gaussian: decout_z_kernel<2, 1, true, 1>, the form under
                     the 128-VGPR cap, which keeps its x / b2 / b6 prefetch at the first K block.
  atomic_LA_L2       the second shape with the LA estimator and L = 2: the gs / la_part branch of
                     the element phase and a second z plane (l = 1).

Compared as tests/test_gpu_step.py::test_single_step_parity compares them, with its tolerances
(stated in that module's docstring): ELBO relative 1e-4; forward activations h, mu, z (and hd,
which this launch recomputes and stores) absolute 1e-5; data gradients norm-wise 1e-4 per tensor;
theta' by check_theta; the Adagrad state norm-wise 1e-4.
"""
import numpy as np
import pytest

from oracle import vaeb_oracle as O
from tests.test_gpu_step import check_theta, data_for, make_ctx, rel

pytestmark = pytest.mark.gpu

CASES = [
    ("slab_partial_k", dict(D=33, H=500, Z=20), 100),
    ("atomic_idle_waves", dict(D=40, H=72, Z=20), 20),
    ("scalar_w1", dict(D=36, H=70, Z=3), 17),
    ("gauss_cap", dict(D=24, H=40, Z=2, continuous=True), 17),
    ("atomic_LA_L2", dict(D=40, H=72, Z=20, estimator="LA", L=2), 20),
]


@pytest.mark.parametrize("name,kw,B", CASES, ids=[c[0] for c in CASES])
def test_decoder_form_step_parity(name, kw, B):
    cfg = O.Config(**kw)
    x = data_for(cfg, 4 * B)
    rng = np.random.default_rng(3)
    # non-zero biases so every bias path is exercised
    params = [p if p.ndim == 2 else (0.01 * rng.standard_normal(p.shape)).astype(np.float32)
              for p in O.init_params(cfg)]
    acc = [np.zeros_like(p) for p in params]
    eps = rng.standard_normal((cfg.L, B, cfg.Z)).astype(np.float32)
    idx = 2
    xb = x[idx * B:(idx + 1) * B]

    ctx = make_ctx(cfg, B)
    ctx.set_data(x)
    ctx.set_params(O.flatten(params))
    ctx.set_adagrad_state(O.flatten(acc))
    ctx.set_eps_mode(1)
    ctx.push_eps(eps)
    elbo = ctx.update(idx)

    p64 = [p.astype(np.float64) for p in params]
    a64 = [a.astype(np.float64) for a in acc]
    ref_elbo, ref_p, ref_a, aux = O.step(p64, a64, xb.astype(np.float64), eps.astype(np.float64), cfg)

    Bp = (B + 15) // 16 * 16
    h = ctx.activation("h", Bp * cfg.H).reshape(-1, cfg.H)[:B]
    mu = ctx.activation("mu", Bp * cfg.Z).reshape(-1, cfg.Z)[:B]
    z = ctx.activation("z", cfg.L * Bp * cfg.Z).reshape(cfg.L, Bp, cfg.Z)
    hd = ctx.activation("hd", cfg.L * Bp * cfg.H).reshape(cfg.L, Bp, cfg.H)
    g = ctx.get_grads()
    newp = ctx.get_params()
    newa = ctx.get_adagrad_state()
    ctx.close()
    ref_hd = aux["hd"].reshape(cfg.L, B, cfg.H)
    grels = {n: rel(gg.reshape(s), rr)
             for (n, s), gg, rr in zip(O.param_shapes(cfg), O.unflatten(g, cfg), aux["data_grads"])}
    dth = np.abs(newp - O.flatten(ref_p))
    print(f"{name}: elbo rel {abs(elbo - ref_elbo) / abs(ref_elbo):.3g}  h {np.abs(h - aux['h']).max():.3g}  "
          f"mu {np.abs(mu - aux['mu']).max():.3g}  z {np.abs(z[:, :B] - aux['z']).max():.3g}  "
          f"hd {np.abs(hd[:, :B] - ref_hd).max():.3g}  grads {max(grels.values()):.3g}  "
          f"theta max {dth.max():.3g} frac {float((dth > 1e-3 * cfg.lr).mean()):.3g}  "
          f"acc {rel(newa, O.flatten(ref_a)):.3g}")

    assert abs(elbo - ref_elbo) <= 1e-4 * abs(ref_elbo), (elbo, ref_elbo)
    assert np.abs(h - aux["h"]).max() <= 1e-5
    assert np.abs(mu - aux["mu"]).max() <= 1e-5
    assert np.abs(z[:, :B] - aux["z"]).max() <= 1e-5
    assert np.abs(hd[:, :B] - ref_hd).max() <= 1e-5
    # padding rows of z and hd are written as zeros (the select on rowok, not a multiply)
    assert not z[:, B:].any() and not hd[:, B:].any()
    for n, r in grels.items():
        assert r <= 1e-4, (n, r)
    check_theta(newp, O.flatten(ref_p), cfg.lr)
    assert rel(newa, O.flatten(ref_a)) <= 1e-4
