"""The fp32 step engine per element, away from theta_0, against the float64 oracle through the C
ABI: cases, states, criterion and bounds are those of tests/f32_parity_cases.py (its header);
tests/test_f32_parity_host.py shows on the host that the inputs are fair and that the criterion
rejects wrong gradients which the norm-wise 1e-4 at theta_0 accepts.

Every test prints one line per device step (-s shows them):

    case-state   worst quantity  device / restatement / bound  |  worst optimizer block (same)  |  value

`worst` is the quantity nearest to its bound; quantities are h, mu, lv, z, hd, dA2, dA6, dA1, dMuLv,
dA3 and the data-gradient blocks gW3 ... (reference order); optimizer blocks are dth.<block>
(theta' - theta) and dac.<block> (acc' - acc) against oracle.adagrad_update in float64 on the
gradient the device reports.  A step that reports VAEB_ERR_NUMERIC raises in update() (or in
epoch_elbo() after update_many) and fails its test.
"""
import numpy as np
import pytest

from oracle import philox as P
from oracle import vaeb_oracle as O
from tests import f32_parity_cases as C
from tests.test_gpu_many_samples import MODES, SWITCHES
from tests.test_gpu_step import make_ctx
from tests.test_philox_oracle import STEP

pytestmark = pytest.mark.gpu

PHILOX_SEED = (41 << 32) | 0x1357ACE
EVAL_ROWS = 64            # evaluation chunk: B = 100 runs as 64 + 36 rows, B = 19 as one short chunk


def device_step(ctx, st):
    """One update() of the minibatch of `st` on a context holding its theta / acc / noise; the
    table line and the failures."""
    value = ctx.update(st.idx)
    got, pad, g = C.read_step(ctx, st.cfg, st.B)
    theta1, acc1 = ctx.get_params(), ctx.get_adagrad_state()
    return C.judge(st, value, got, pad, g, theta1, acc1), theta1, acc1


def run_host_eps_step(st, what=""):
    ctx = make_ctx(st.cfg, st.B, keep_grads=True, use_graph=True)
    try:
        ctx.set_data(st.x)
        ctx.set_params(st.theta())
        ctx.set_adagrad_state(st.acc_flat())
        ctx.set_eps_mode(1)
        ctx.push_eps(st.eps)
        (line, bad), _, _ = device_step(ctx, st)
    finally:
        ctx.close()
    print(line + what)
    assert not bad, (bad, line + what)


@pytest.mark.parametrize("name,state", C.CASES, ids=C.CASE_IDS)
def test_step_per_element(name, state):
    """One training step at scaled and at start-up weights under every criterion of
    tests/f32_parity_cases.py.  Recorded on the first run on an MI355X:

    mnist20-x30                       gb1    3.6e-07 / 3.4e-07 / 5.4e-06 | dac.b1 1.6e-07 / 5.5e-08 / 1.9e-06 | value 3.6e-10
    frey2_gauss-x30                   gW4    5.2e-07 / 3.7e-07 / 5.9e-06 | dth.W4 9.5e-07 / 9.5e-07 / 1.5e-05 | value 4.2e-08
    odd_shapes-x30                    dA1    1.9e-07 / 1.4e-07 / 2.3e-06 | dth.W3 4.3e-06 / 4.3e-06 / 6.9e-05 | value 1.0e-08
    atomic_LA_L2-x30                  gW3    2.0e-07 / 1.7e-07 / 2.7e-06 | dth.W2 3.0e-06 / 3.0e-06 / 4.7e-05 | value 4.3e-08
    gauss_latent28_slab_odd_H-x30     h      3.8e-07 / 3.3e-07 / 5.3e-06 | dth.W3 5.3e-06 / 5.3e-06 / 8.4e-05 | value 5.6e-09
    mean_map_frey10-x30               gb5    2.2e-07 / 9.5e-08 / 1.9e-06 | dth.b6 1.6e-06 / 1.5e-06 / 2.4e-05 | value 5.9e-08
    bern_latent18_odd_H_deep-x30      gW4    2.2e-07 / 1.9e-07 / 3.0e-06 | dth.W3 1.6e-06 / 1.6e-06 / 2.5e-05 | value 1.3e-08
    wide_latent_generic-x30           z      2.0e-07 / 1.2e-07 / 1.9e-06 | dth.W3 6.0e-06 / 5.9e-06 / 9.4e-05 | value 4.4e-08
    L6_LA_deferred-x30                gb4    1.4e-07 / 1.2e-07 / 1.9e-06 | dac.W1 1.3e-07 / 5.8e-08 / 1.9e-06 | value 4.7e-08
    H1040_gauss_L5-x30                dMuLv  1.4e-06 / 1.0e-06 / 1.7e-05 | dth.b4 3.9e-07 / 3.6e-07 / 5.7e-06 | value 6.0e-08
    slab_partial_k-x30                gb4    2.5e-07 / 1.3e-07 / 2.0e-06 | dth.W5 1.6e-06 / 1.6e-06 / 2.5e-05 | value 3.0e-08
    gauss_cap-x30                     z      1.9e-07 / 7.9e-08 / 1.9e-06 | dth.W4 2.6e-06 / 2.6e-06 / 4.2e-05 | value 3.9e-08
    mnist20-startup                   gb5    1.9e-07 / 1.3e-07 / 2.1e-06 | dth.b5 1.4e-07 / 6.7e-08 / 1.9e-06 | value 1.0e-08
    frey2_gauss-startup               hd     5.2e-07 / 1.3e-07 / 2.1e-06 | dth.W4 2.4e-07 / 1.9e-07 / 3.0e-06 | value 4.8e-08
    mean_map_frey10-startup           gW5    3.9e-07 / 3.2e-07 / 5.1e-06 | dth.W3 2.6e-07 / 2.5e-07 / 4.0e-06 | value 4.0e-08
    bern_latent18_odd_H_deep-startup  gW4    2.6e-07 / 1.5e-07 / 2.4e-06 | dac.W1 1.3e-07 / 8.9e-08 / 1.9e-06 | value 5.7e-08
    mnist_LA_L2-startup               gW4    5.8e-07 / 3.7e-07 / 6.0e-06 | dth.W3 3.1e-07 / 3.1e-07 / 5.0e-06 | value 2.3e-08
    """
    run_host_eps_step(C.case(name, state))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["atomic_LA_L2", "gauss_latent28_slab_odd_H"])
def test_handoff_forms_at_x30(name, mode, monkeypatch):
    """The x30 step under each switch setting of tests/test_gpu_many_samples.py MODES (the context
    reads the switches when it is created): counted atomics, slabs + ticket, the decoder-summed
    encoder slabs, the unfolded latent backward, the ticketed backward reducer, the in-step dW2.
    Recorded on the first run on an MI355X:

    atomic_LA_L2-x30                  gW3    2.0e-07 / 1.7e-07 / 2.7e-06 | dth.W2 3.0e-06 / 3.0e-06 / 4.7e-05 | value 4.3e-08  [atomic]
    atomic_LA_L2-x30                  gW3    2.0e-07 / 1.7e-07 / 2.7e-06 | dth.W2 3.0e-06 / 3.0e-06 / 4.8e-05 | value 4.6e-08  [slab]
    atomic_LA_L2-x30                  gW3    2.9e-07 / 1.7e-07 / 2.7e-06 | dth.W2 3.0e-06 / 3.0e-06 / 4.8e-05 | value 4.3e-08  [decred]
    atomic_LA_L2-x30                  gb4    1.6e-07 / 1.0e-07 / 1.9e-06 | dth.W2 3.0e-06 / 3.0e-06 / 4.7e-05 | value 4.3e-08  [unfolded]
    atomic_LA_L2-x30                  gW3    2.0e-07 / 1.7e-07 / 2.7e-06 | dth.W2 3.0e-06 / 3.0e-06 / 4.8e-05 | value 4.6e-08  [ticket]
    atomic_LA_L2-x30                  gW3    2.0e-07 / 1.7e-07 / 2.7e-06 | dth.W2 3.0e-06 / 3.0e-06 / 4.7e-05 | value 4.3e-08  [dw2now]
    gauss_latent28_slab_odd_H-x30     dA6    8.6e-07 / 3.8e-07 / 6.1e-06 | dth.W3 5.3e-06 / 5.3e-06 / 8.4e-05 | value 9.1e-08  [atomic]
    gauss_latent28_slab_odd_H-x30     dA6    8.6e-07 / 3.8e-07 / 6.1e-06 | dth.W3 5.3e-06 / 5.3e-06 / 8.4e-05 | value 9.1e-08  [slab]
    gauss_latent28_slab_odd_H-x30     h      3.8e-07 / 3.3e-07 / 5.3e-06 | dth.W3 5.3e-06 / 5.3e-06 / 8.4e-05 | value 5.6e-09  [decred]
    gauss_latent28_slab_odd_H-x30     dA6    8.6e-07 / 3.8e-07 / 6.1e-06 | dth.W3 5.3e-06 / 5.3e-06 / 8.4e-05 | value 9.1e-08  [unfolded]
    gauss_latent28_slab_odd_H-x30     dA6    8.6e-07 / 3.8e-07 / 6.1e-06 | dth.W3 5.3e-06 / 5.3e-06 / 8.4e-05 | value 9.1e-08  [ticket]
    gauss_latent28_slab_odd_H-x30     dA6    8.6e-07 / 3.8e-07 / 6.1e-06 | dth.W3 5.3e-06 / 5.3e-06 / 8.4e-05 | value 9.1e-08  [dw2now]
    """
    for var, v in zip(SWITCHES, MODES[mode]):
        monkeypatch.setenv(var, v)
    run_host_eps_step(C.case(name, "x30"), what=f"  [{mode}]")


@pytest.mark.parametrize("name", ["mnist20", "frey2_gauss"])
def test_startup_three_steps(name):
    """Three Philox-mode steps from the start-up state, the noise drawn on the host by
    oracle/philox.py (as tests/test_gpu_philox.py): before each step theta and acc are read from
    the device and the oracle steps from them (teacher forcing), under the criteria above; then
    update_many of the same three minibatches from the same state ends bit-identical in theta and
    acc -- the per-step read-back flushes the deferred dW2, update_many lets it land inside the
    next encoder launch.  Recorded on the first run on an MI355X:

    mnist20 step 0-startup            gW1    4.0e-07 / 3.4e-07 / 5.5e-06 | dth.W5 3.0e-07 / 3.0e-07 / 4.8e-06 | value 8.0e-09
    mnist20 step 1-startup            gb3    4.6e-07 / 4.1e-07 / 6.5e-06 | dth.W3 2.0e-07 / 1.9e-07 / 3.1e-06 | value 3.1e-08
    mnist20 step 2-startup            gb5    2.5e-07 / 2.3e-07 / 3.7e-06 | dth.W5 3.1e-07 / 2.7e-07 / 4.3e-06 | value 1.5e-09
    frey2_gauss step 0-startup        hd     4.5e-07 / 9.7e-08 / 1.9e-06 | dth.b3 2.3e-07 / 2.1e-07 / 3.4e-06 | value 1.6e-09
    frey2_gauss step 1-startup        hd     2.8e-07 / 1.2e-07 / 1.9e-06 | dth.b3 1.8e-07 / 1.8e-07 / 2.9e-06 | value 5.9e-08
    frey2_gauss step 2-startup        hd     2.0e-07 / 1.5e-07 / 2.4e-06 | dac.b2 1.7e-07 / 8.5e-08 / 1.9e-06 | value 1.2e-07
    """
    st0 = C.case(name, "startup")
    cfg, B = st0.cfg, st0.B
    order = np.array([2, 0, 3], np.int32)

    def context():
        ctx = make_ctx(cfg, B, keep_grads=True, use_graph=True)
        ctx.set_data(st0.x)
        ctx.set_params(st0.theta())
        ctx.set_adagrad_state(st0.acc_flat())
        ctx.set_eps_mode(0, PHILOX_SEED)
        ctx.set_step(STEP)
        return ctx

    lines, failures = [], []
    ctx = context()
    try:
        for t, b in enumerate(order):
            theta, acc, step = ctx.get_params(), ctx.get_adagrad_state(), ctx.get_step()
            assert step == STEP + t
            eps = P.train_eps(PHILOX_SEED, step, int(b), B, B, 0, cfg.L, cfg.Z)
            st = C.make_step(f"{name} step {t}", "startup", cfg, B, st0.x, int(b), O.unflatten(theta, cfg),
                             O.unflatten(acc, cfg), eps)
            (line, bad), theta1, acc1 = device_step(ctx, st)
            lines.append(line)
            failures += [(t, k) for k in bad]
    finally:
        ctx.close()
    print("\n".join(lines))
    assert not failures, (failures, lines)

    ctx = context()
    try:
        ctx.update_many(order)
        _, n = ctx.epoch_elbo()          # raises on VAEB_ERR_NUMERIC
        many = ctx.get_params(), ctx.get_adagrad_state()
    finally:
        ctx.close()
    assert n == len(order)
    assert np.array_equal(many[0], theta1), float(np.abs(many[0] - theta1).max())
    assert np.array_equal(many[1], acc1), float(np.abs(many[1] - acc1).max())


@pytest.mark.parametrize("name", ["mnist20", "frey2_gauss", "H1040_gauss_L5"])
def test_eval_path_at_x30(name):
    """validate (host eps), encode and reconstruct at the x30 state: the evaluation chunks run the
    per-row-block kernels (PEnc, heads_dechid_kernel, PDecOut in MODE_EVAL / MODE_RECON) that a
    training step with Z <= 32 never launches.  err and bound as for the step; the float64
    references are the step's own forward (validate = its SGVB, encode = its mu, lv) and
    oracle.reconstruct_full at z = mu.  Recorded on the first run on an MI355X:

    mnist20-x30:
        mu 2.4e-07 / 8.1e-07 / 1.3e-05, lv 2.1e-07 / 9.5e-07 / 1.5e-05, y 6.1e-07 / 1.2e-06 / 1.9e-05
        validate 4.1e-09 / 8.5e-09 / 1.9e-06
    frey2_gauss-x30:
        mu 2.4e-07 / 4.5e-07 / 7.2e-06, lv 2.8e-07 / 4.8e-07 / 7.7e-06, y 4.4e-07 / 6.5e-07 / 1.0e-05
        log_sigma 3.5e-07 / 6.8e-07 / 1.1e-05, validate 3.0e-08 / 7.1e-09 / 1.9e-06
    H1040_gauss_L5-x30:
        mu 2.6e-07 / 7.2e-07 / 1.2e-05, lv 3.1e-07 / 1.3e-06 / 2.0e-05, y 5.9e-07 / 1.1e-06 / 1.7e-05
        log_sigma 4.4e-07 / 1.3e-06 / 2.1e-05, validate 2.0e-08 / 2.1e-07 / 3.4e-06
    """
    st = C.case(name, "x30")
    cfg, B = st.cfg, st.B
    xb = st.x[st.idx * B:(st.idx + 1) * B]
    y64, ls64 = O.reconstruct_full(C.f64(st.params), xb.astype(np.float64), None, cfg)
    y32, ls32 = O.reconstruct_full(st.params, xb, None, cfg)
    q64 = {"mu": st.q64["mu"], "lv": st.q64["lv"], "y": y64}
    restate = {"mu": st.restate["mu"], "lv": st.restate["lv"], "y": C.err(y32, y64), "validate": st.restate_value}
    if cfg.continuous:
        q64["log_sigma"] = ls64
        restate["log_sigma"] = C.err(ls32, ls64)
    bound = C.bound_of(restate)
    ctx = make_ctx(cfg, B, keep_grads=False, max_eval_rows=EVAL_ROWS)
    try:
        ctx.set_params(st.theta())
        ctx.set_eps_mode(1)
        ctx.push_eps(st.eps)
        v = ctx.validate(xb)
        got = dict(zip(("mu", "lv"), ctx.encode(xb)))
        if cfg.continuous:
            got["y"], got["log_sigma"] = ctx.reconstruct_full(xb, 0)
            assert np.array_equal(ctx.reconstruct(xb), got["y"])
        else:
            got["y"] = ctx.reconstruct(xb)
    finally:
        ctx.close()
    e = C.errors(got, q64)
    e["validate"] = abs(v - float(st.out64["sgvb"])) / abs(float(st.out64["sgvb"]))
    print(f"{name}-x30 eval: " + ", ".join(f"{k} {e[k]:.1e} / {restate[k]:.1e} / {bound[k]:.1e}" for k in e))
    assert C.rejected(e, bound) == [], e
