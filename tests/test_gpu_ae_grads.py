"""Per-element gradient parity of the layer-stack engine's training step (vaeb_ae_train:
vaeb_amd/csrc/ae_mlp.hpp PAeFwd / PAeBwd / PAeWgrad, engine_ae.inc ae_step) against the float64
oracles, point latent (oracle/ae_oracle.py) and Gaussian latent with host eps
(tests/vae_stack_oracle.py), at theta_0 and at scaled weights, at the tile engine's edges.

The device's gradient is recovered from what the ABI returns: the step starts from a ZERO AdaGrad
accumulator, so acc' = g^2 and g = sign(theta' - theta) sqrt(acc') (tests/ae_grad_cases.py, which
also holds the case table and the inputs).  Per parameter block, max|g - g64| / max|g64| has to be
<= 16 x the same figure of the float32 NumPy restatement of the step; the step's value within
VALUE_RTOL = 2e-5.  tests/test_ae_grads_host.py shows that ten kinds of wrong gradient each miss
these bounds and that the bounds are all <= 1e-4.  No bound comes from the device.

Order of update.  ae_step (in ae_bwd_layer) updates a layer's weights right after the launch that
reads them for the data gradient.  A layer updated BEFORE that read would shift the gradient below
it by O(eta) = 1e-2 relative at scaled weights, four orders above the bounds, so the scaled rows cover the order of
the launches; there is no separate test.

Stale rows.  test_small_batch_after_a_large_one takes a 33-row step, then a 5-row step on the same
context: the activation and delta buffers then hold rows 5..32 of the first step, which no kernel
of the second may read.

Measured on an MI355X (every test prints its line; -s shows them).  Per case the block nearest to
its bound: device error / restatement error / bound, and the value's relative error.

  case                           block    device  / restate / bound      value
  edge_bin_tanh-point-theta0     Wout     3.0e-07 / 2.5e-07 / 4.0e-06   6.6e-08
  edge_bin_tanh-point-x30        Wdec1    1.8e-07 / 8.6e-08 / 1.4e-06   1.2e-08
  edge_bin_tanh-gauss-theta0     bzlv     4.9e-06 / 9.4e-07 / 1.5e-05   1.1e-08
  edge_bin_tanh-gauss-x30        bzlv     1.7e-07 / 3.9e-08 / 6.3e-07   8.9e-09
  edge_cont_sigmoid-point-theta0 bmu      2.9e-07 / 2.4e-07 / 3.9e-06   6.5e-08
  edge_cont_sigmoid-point-x30    bmu      1.4e-07 / 7.4e-08 / 1.2e-06   3.0e-08
  edge_cont_sigmoid-gauss-theta0 blogs2   1.4e-07 / 1.0e-07 / 1.6e-06   2.1e-08
  edge_cont_sigmoid-gauss-x30    Wzlv     2.5e-07 / 1.5e-07 / 2.3e-06   9.0e-09
  edge_relu_b1-point-theta0      bdec0    1.1e-07 / 8.4e-08 / 1.3e-06   1.3e-08
  edge_relu_b1-point-x30         bdec0    9.4e-08 / 7.9e-08 / 1.3e-06   6.7e-08
  edge_relu_b1-gauss-theta0      Wdec0    2.2e-07 / 1.6e-07 / 2.6e-06   2.5e-08
  edge_relu_b1-gauss-x30         bzlv     9.5e-08 / 1.9e-08 / 3.0e-07   1.2e-07
  k512_513-point-theta0          Wz       2.1e-07 / 1.3e-07 / 2.0e-06   1.1e-08
  k512_513-point-x30             bmu      3.5e-07 / 2.0e-07 / 3.1e-06   4.9e-08
  k512_513-gauss-theta0          Wmu      3.4e-07 / 1.7e-07 / 2.7e-06   9.2e-09
  k512_513-gauss-x30             bmu      3.4e-07 / 2.0e-07 / 3.2e-06   4.2e-09
  batch_512-point-theta0         benc0    1.4e-07 / 2.5e-07 / 4.0e-06   3.0e-08
  batch_512-point-x30            Wenc0    1.5e-07 / 2.2e-07 / 3.5e-06   3.8e-08
  batch_512-gauss-theta0         Wenc0    1.9e-07 / 3.3e-07 / 5.2e-06   4.3e-09
  batch_512-gauss-x30            bdec0    1.7e-07 / 4.0e-07 / 6.3e-06   2.1e-08
  batch_513-point-theta0         Wdec0    2.1e-07 / 4.3e-07 / 6.8e-06   7.6e-08
  batch_513-point-x30            benc0    1.6e-07 / 2.6e-07 / 4.1e-06   1.2e-08
  batch_513-gauss-theta0         Wdec0    3.3e-07 / 3.6e-07 / 5.7e-06   2.6e-08
  batch_513-gauss-x30            Wzlv     1.0e-07 / 2.8e-07 / 4.5e-06   8.9e-09
  latent_deep_k-gauss-theta0     Wzmu     1.2e-07 / 5.0e-08 / 8.0e-07   3.2e-08
  latent_deep_k-gauss-x30        Wenc0    2.1e-07 / 1.8e-07 / 2.8e-06   1.0e-08
  stale-point 33 rows            bmu      3.5e-07 / 2.0e-07 / 3.1e-06   4.9e-08
  stale-point then 5 rows        Wlogs2   5.1e-07 / 2.0e-07 / 3.2e-06   9.0e-09
  stale-gauss 33 rows            bmu      3.4e-07 / 2.0e-07 / 3.2e-06   4.2e-09
  stale-gauss then 5 rows        benc0    2.0e-07 / 1.0e-07 / 1.6e-06   8.2e-08

The device is at most 5.2 x the restatement, i.e. 0.33 of its bound (bzlv of
edge_bin_tanh-gauss-theta0: at |lv| ~ 0.01 the term 1/2 (1 - e^lv) loses two digits to
cancellation in float32, and the device's exponential is the ~1-ulp hardware one); on the
batch_512 / batch_513 rows it is below the restatement, whose NumPy column sums over 512 rows run
in sequence where the device adds eight K slices.  Nothing failed on the first run and no kernel
changed.
"""
import numpy as np
import pytest

from oracle import ae_oracle as A
from tests import ae_grad_cases as G

pytestmark = pytest.mark.gpu


def make_ctx(cfg, max_batch, latent):
    from vaeb_amd import _lib
    return _lib.AEContext(cfg.Dobs, cfg.Denc, cfg.Dz, cfg.Ddec, otype=cfg.otype, act=cfg.act, s2=cfg.s2,
                          eta=cfg.eta, max_batch=max_batch, latent=latent)


def zero_acc_step(ctx, st):
    """theta, a zero accumulator and (Gaussian latent) the host eps of st loaded, one train(idx):
    (value, theta', acc')."""
    from vaeb_amd import _lib
    ctx.set_params(st.theta())
    ctx.set_adagrad_state(np.zeros(ctx.P, np.float32))
    if st.latent == "gauss":
        ctx.set_eps_mode(_lib.EPS_HOST)
        ctx.push_eps(st.eps)
    v = ctx.train(st.idx)
    return v, ctx.get_params(), ctx.get_adagrad_state()


def assert_step(label, st, v, th1, ac1):
    err = st.device_errors(th1, ac1)
    vrel = abs(v - st.value64) / abs(st.value64)
    print(G.table_line(label, err, st.bound, st.restate) + f"   value {vrel:.1e}")
    bad = G.rejected(err, st.bound)
    assert not bad, {n: (err[n], st.restate[n], st.bound[n]) for n in bad}
    assert vrel <= G.VALUE_RTOL, (v, st.value64)


@pytest.mark.parametrize("name,latent,scaled", G.CASES, ids=G.CASE_IDS)
def test_ae_step_gradient_per_block(name, latent, scaled):
    st = G.case(name, latent, scaled)
    B = len(st.idx)
    ctx = make_ctx(st.cfg, B, latent)
    try:
        assert ctx.P == sum(int(np.prod(s)) for _, s in st.shapes)
        ctx.set_data(st.Xtr)
        v, th1, ac1 = zero_acc_step(ctx, st)
    finally:
        ctx.close()
    assert_step(f"{name}-{latent}-{'x30' if scaled else 'theta0'}", st, v, th1, ac1)


@pytest.mark.parametrize("latent", ["point", "gauss"])
def test_small_batch_after_a_large_one(latent):
    """k512_513 at scaled weights: a step at B = max_batch = 33, then theta and a zero accumulator
    again and a step with 5 other rows of the same Xtr; both meet their own bounds."""
    big = G.case("k512_513", latent, True)
    assert len(big.idx) == 33
    rng = np.random.default_rng(7)
    idx5 = rng.choice(big.Xtr.shape[0], size=5, replace=False).astype(np.int32)
    eps5 = rng.standard_normal((5, big.cfg.Dz)).astype(np.float32) if latent == "gauss" else None
    small = G.make_step(big.cfg, latent, big.params, big.Xtr, idx5, eps5)
    assert max(small.bound.values()) <= G.GRAD_CAP
    ctx = make_ctx(big.cfg, 33, latent)
    try:
        ctx.set_data(big.Xtr)
        first = zero_acc_step(ctx, big)
        second = zero_acc_step(ctx, small)
    finally:
        ctx.close()
    assert_step(f"stale-{latent} 33 rows", big, *first)
    assert_step(f"stale-{latent} then 5 rows", small, *second)
