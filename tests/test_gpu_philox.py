"""The device's Philox noise and Philox-mode steps against the host oracle (oracle/philox.py +
oracle/vaeb_oracle.py, float64), through the C ABI.

Every other parity test injects its noise from the host; every run that matters draws it on
the device.  Here the noise is the device's own, and the oracle draws the same numbers from
the documented key (include/vaeb_hip.h): (seed, step, global row, l * Z + j) in the training
domain, (seed, step, row of the call, j, stream) in the evaluation domain, (seed, step,
parameter group) for the FVS weight noise.  All cases run at a batch index > 0 with a step
counter and a seed above 2^32; tests/test_philox_oracle.py shows on the host that each of them
tells a mis-keyed site apart.  The step counter is read back (get_step) before each call.

Tolerances
  * eps itself: |device - oracle| <= EPS_ATOL for every element.  A correctly rounded float32
    evaluation of the same formula is within 4.2e-7 of the float64 oracle; the device adds the
    hardware log / sqrt / cos approximations.  Observed on one MI355X over every eps comparison
    of this file: 5.68e-7 at most; EPS_ATOL is 4x that, so another
    clock or compiler does not flip it, and no element may exceed it.  A wrong key gives
    differences of order 1.
  * Philox-mode steps, trajectories, evaluations, the FVS step and the 16-bit engines: exactly
    the tolerances of the host-eps tests they mirror (named at each test).
"""
import functools

import numpy as np
import pytest

from oracle import philox as P
from oracle import vaeb_oracle as O
from tests.test_philox_oracle import (ALL_TRAIN, EPS_CASES, FVS_CASE, H16_CASES, H16_IDX, IDX, STEP, STEP_CASES,
                                      TRAJ_CASE)

pytestmark = pytest.mark.gpu

EPS_ATOL = 2.3e-6

EST = {"LB": 0, "LA": 1, "FV": 2, "FVS": 3}
SWITCHES = ("VAEB_ATOMIC_HO", "VAEB_ENC_RED", "VAEB_FOLD_BWD", "VAEB_BWD_DEFER", "VAEB_DW2_DEFER")
# the settings test_gpu_step.py::test_atomic_and_slab_handoffs_agree enumerates
MODES = {"atomic": ("1", "0", "1", "1", "1"), "slab": ("0", "0", "1", "1", "1"),
         "decred": ("1", "1", "1", "1", "1"), "unfolded": ("1", "0", "0", "1", "1"),
         "ticket": ("0", "0", "1", "0", "1"), "dw2now": ("1", "0", "1", "1", "0")}


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def check_theta(new, ref, lr):
    d = np.abs(new - ref)
    assert d.max() <= 2 * lr + 1e-7, d.max()
    frac = float((d > 1e-3 * lr).mean())
    assert frac <= 1e-4, frac


def data_for(cfg, n, seed=0):
    if cfg.continuous:
        return O.synthetic_frey(n=n, D=cfg.D, seed=seed)
    return O.synthetic_mnist(n=n, D=cfg.D, seed=seed)


def r16(n):
    return (n + 15) // 16 * 16


def make_ctx(c, use_graph=True, keep_grads=True, dtype=0, max_eval_rows=None):
    from vaeb_amd import _lib
    cfg = O.Config(**c.kw)
    return _lib.Context(cfg.D, cfg.H, cfg.Z, c.B, L=cfg.L, decoder=int(cfg.continuous), estimator=EST[cfg.estimator],
                        lr=cfg.lr, B_global=c.B_global, row_offset=c.row_offset, keep_grads=keep_grads,
                        use_graph=use_graph, max_eval_rows=max_eval_rows or max(c.B, 16), dtype=dtype)


def device_eps(ctx, c):
    """The step's eps as the fp32 engine stored it: [L][B rounded up to 16][Z]."""
    L, Z = c.kw.get("L", 1), c.kw["Z"]
    return ctx.activation("eps", L * r16(c.B) * Z).reshape(L, r16(c.B), Z)[:, :c.B]


def assert_eps(got, want, what):
    err = float(np.abs(got - want).max())
    print(f"eps {what}: max |device - oracle| = {err:.3e}")
    assert got.shape == want.shape
    assert int((np.abs(got - want) > EPS_ATOL).sum()) == 0, (what, err)


@functools.lru_cache(maxsize=None)
def _inputs(name, idx, acc0, rng_seed):
    c = ALL_TRAIN[name][0]
    cfg = O.Config(**c.kw)
    x = data_for(cfg, (idx + 2) * c.B_global)
    rng = np.random.default_rng(rng_seed)
    params = [p if p.ndim == 2 else (0.01 * rng.standard_normal(p.shape)).astype(np.float32)
              for p in O.init_params(cfg)]
    acc = [np.full_like(p, acc0) for p in params]
    r0 = idx * c.B_global + c.row_offset
    xb = x[r0:r0 + c.B].astype(np.float64)
    for a in [x, xb] + params + acc:
        a.setflags(write=False)
    return cfg, x, params, acc, xb


def inputs(c, idx, acc0=0.0, rng_seed=3):
    """(cfg, x, params, acc, this rank's rows of minibatch idx), as test_single_step_parity draws
    them (non-zero biases so every bias path is exercised); computed once per case."""
    return _inputs(c.name, idx, acc0, rng_seed)


@functools.lru_cache(maxsize=None)
def _step_reference(name, step, idx, q, acc0, rng_seed):
    c = ALL_TRAIN[name][0]
    cfg, x, params, acc, xb = inputs(c, idx, acc0, rng_seed)
    eps = P.train_eps(c.seed, step, idx, c.B, c.B_global, c.row_offset, cfg.L, cfg.Z)
    p64 = [p.astype(np.float64) for p in params]
    a64 = [a.astype(np.float64) for a in acc]
    return eps, O.step(p64, a64, xb, eps, cfg, q=q)


def step_reference(c, step, idx=IDX, q=None, acc0=0.0, rng_seed=3):
    """O.step on the oracle's own draw of the step's noise, computed once per case and step."""
    return _step_reference(c.name, step, idx, q, acc0, rng_seed)


def start(c, ctx, idx=IDX, acc0=0.0, rng_seed=3):
    cfg, x, params, acc, _ = inputs(c, idx, acc0, rng_seed)
    ctx.set_data(x)
    ctx.set_params(O.flatten(params))
    ctx.set_adagrad_state(O.flatten(acc))
    ctx.set_eps_mode(0, c.seed)
    ctx.set_step(STEP)
    return cfg


def check_eps_both_launch_forms(c, ctx):
    """eps of one update() (an eager step, the rows addressed from the launch arguments) and of
    one update_async() (the order / cursor form: a replayed graph when the context has one),
    each against the oracle at the counter read before it.  Returns update()'s (step, ELBO)."""
    step = ctx.get_step()
    assert step >> 32
    elbo = ctx.update(IDX)
    assert_eps(device_eps(ctx, c), P.train_eps(c.seed, step, IDX, c.B, c.B_global, c.row_offset, c.kw.get("L", 1),
                                                c.kw["Z"]), f"{c.name} update")
    return step, elbo


def check_async_eps(c, ctx):
    step = ctx.get_step()
    ctx.update_async(IDX)
    ctx.synchronize()
    assert_eps(device_eps(ctx, c), P.train_eps(c.seed, step, IDX, c.B, c.B_global, c.row_offset, c.kw.get("L", 1),
                                                c.kw["Z"]), f"{c.name} update_async")
    assert ctx.get_step() == step + 1


def check_step(c, ctx, cfg, step, elbo):
    """The assertions of test_gpu_step.py::test_single_step_parity, at its tolerances (the ELBO is
    SGVB / B_global, the oracle's SGVB / B)."""
    _, (ref_elbo, ref_p, ref_a, aux) = step_reference(c, step)
    assert abs(elbo * c.B_global - ref_elbo * c.B) <= 1e-4 * abs(ref_elbo * c.B), (elbo, ref_elbo)
    g = ctx.get_grads()
    for (n, s), gg, rr in zip(O.param_shapes(cfg), O.unflatten(g, cfg), aux["data_grads"]):
        assert rel(gg.reshape(s), rr) <= 1e-4, (n, rel(gg.reshape(s), rr))
    check_theta(ctx.get_params(), O.flatten(ref_p), cfg.lr)
    assert rel(ctx.get_adagrad_state(), O.flatten(ref_a)) <= 1e-4


# ------------------------------------------------------------------ (a) the draws themselves
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("c", EPS_CASES, ids=[c.name for c in EPS_CASES])
def test_eps_matches_oracle(c, use_graph):
    ctx = make_ctx(c, use_graph=use_graph, keep_grads=False)
    start(c, ctx)
    check_eps_both_launch_forms(c, ctx)
    check_async_eps(c, ctx)
    check_async_eps(c, ctx)     # with a graph: the replay (the first call captures)
    ctx.close()


SWITCH_CASES = [c for c in STEP_CASES if c.name in ("fused", "two_fx_slots")]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("c", SWITCH_CASES, ids=[c.name for c in SWITCH_CASES])
def test_eps_and_step_under_every_switch_setting(c, mode, monkeypatch):
    """Every fp32 step form a switch selects draws the same eps (each form has its own draw site:
    the atomic hand-off's row block, the slab reducer, the decoder launch that sums the encoder's
    slabs) and takes the oracle's step with it, as a graph and as eager launches."""
    for var, v in zip(SWITCHES, MODES[mode]):
        monkeypatch.setenv(var, v)
    for use_graph in (True, False):
        ctx = make_ctx(c, use_graph=use_graph)
        cfg = start(c, ctx)
        step, elbo = check_eps_both_launch_forms(c, ctx)
        check_step(c, ctx, cfg, step, elbo)
        check_async_eps(c, ctx)
        check_async_eps(c, ctx)
        ctx.close()


# --------------------------------------------------------- (b) one Philox-mode step vs O.step
@pytest.mark.parametrize("c", STEP_CASES, ids=[c.name for c in STEP_CASES])
def test_philox_step_matches_oracle(c):
    """The device's step on its own noise == the oracle's step on the oracle's draw of it: a
    backward pass that re-drew a different eps than the forward pass used (or an ELBO taken at
    another z than the gradient) fails the gradient bound."""
    ctx = make_ctx(c)
    cfg = start(c, ctx)
    step, elbo = check_eps_both_launch_forms(c, ctx)
    check_step(c, ctx, cfg, step, elbo)
    # forward activations, as test_single_step_parity
    _, (_, _, _, aux) = step_reference(c, step)
    mu = ctx.activation("mu", r16(c.B) * cfg.Z).reshape(-1, cfg.Z)[:c.B]
    assert np.abs(mu - aux["mu"]).max() <= 1e-5
    ctx.close()


# ------------------------------------------------------------------------ (c) several steps
def test_philox_trajectory_update_many():
    """Five steps: per-step update() ELBOs and one update_many() call (graph replay, the
    device-resident batch order and step counter) against five oracle steps on train_eps(step0 +
    t); tolerances of test_trajectory_50_steps_mnist (ELBO 1e-3 relative, theta 5e-3)."""
    c = TRAJ_CASE
    order = np.array([2, 5, 1, 6, 3], np.int32)
    cfg = O.Config(**c.kw)
    x = data_for(cfg, 8 * c.B)
    params = O.init_params(cfg)
    got = {}
    for form in ("sync", "many"):
        ctx = make_ctx(c, keep_grads=False)
        ctx.set_data(x)
        ctx.set_params(O.flatten(params))
        ctx.set_eps_mode(0, c.seed)
        ctx.set_step(STEP)
        step0 = ctx.get_step()
        if form == "sync":
            elbos = [ctx.update(int(b)) for b in order]
        else:
            ctx.update_many(order)
            tot, n = ctx.epoch_elbo()
            assert n == len(order)
            elbos = tot
        assert ctx.get_step() == step0 + len(order)
        got[form] = (step0, elbos, ctx.get_params())
        ctx.close()
    assert got["sync"][0] == got["many"][0]
    p = [q.astype(np.float64) for q in params]
    a = [np.zeros_like(q) for q in p]
    refs = []
    for t, b in enumerate(order):
        eps = P.train_eps(c.seed, got["sync"][0] + t, int(b), c.B, c.B, 0, 1, cfg.Z)
        e, p, a, _ = O.step(p, a, x[b * c.B:(b + 1) * c.B].astype(np.float64), eps, cfg)
        refs.append(e)
    refs = np.array(refs)
    elbos = np.array(got["sync"][1])
    assert np.all(np.abs(elbos - refs) <= 1e-3 * np.abs(refs)), np.abs(elbos - refs).max()
    assert abs(got["many"][1] - refs.sum()) <= 1e-3 * abs(refs.sum())
    for form in got:
        assert np.abs(got[form][2] - O.flatten(p)).max() <= 5e-3, form


# ------------------------------------------------------------------- (d) evaluation domains
@pytest.mark.parametrize("continuous", [False, True], ids=["bernoulli", "gaussian"])
def test_evaluation_domains_match_oracle(continuous):
    """n = 77 rows in chunks of 32 (three chunks, n % 16 != 0): validate and validate_resident on
    stream 0 (tolerance of test_validate_matches_oracle), reconstruct_sampled(x, 3) on streams
    1..3 (1e-5, test_reconstruct_sampled_matches_oracle), marginal_ll(x, K) on streams k + 1
    (test_gpu_marginal_ll.py's reference and RTOL): the last two pin the header's "exactly the
    streams vaeb_reconstruct_sampled uses".  Rows are keyed by their index in the call, not in
    the chunk."""
    from tests.test_gpu_marginal_ll import RTOL, assert_matches, iw_reference
    from vaeb_amd import _lib
    cfg = O.Config(D=560, H=200, Z=2, continuous=True) if continuous else O.Config(D=784, H=500, Z=20)
    n, K, seed = 77, 4, (33 << 32) | 0x1234567
    rng = np.random.default_rng(3)
    params = [(0.1 * rng.standard_normal(s)).astype(np.float32) for _, s in O.param_shapes(cfg)]
    p64 = [p.astype(np.float64) for p in params]
    x = data_for(cfg, n, seed=5)
    x64 = x.astype(np.float64)
    ctx = _lib.Context(cfg.D, cfg.H, cfg.Z, 16, decoder=int(continuous), max_eval_rows=32)
    ctx.set_params(O.flatten(params))
    ctx.set_eps_mode(_lib.EPS_PHILOX, seed)
    ctx.set_step(STEP)

    step = ctx.get_step()
    v = ctx.validate(x)
    assert ctx.get_step() == step      # evaluation draws at the counter and leaves it
    ref = O.validate(p64, x64, P.eval_eps(seed, step, n, cfg.Z, 0)[None], cfg)
    print(f"validate rel err {abs(v - ref) / abs(ref):.3e}")
    assert abs(v - ref) <= 1e-4 * abs(ref), (v, ref)

    ctx.set_valid_data(x)
    step = ctx.get_step()
    vr = ctx.validate_resident()
    assert ctx.get_step() == step
    ref = O.validate(p64, x64, P.eval_eps(seed, step, n, cfg.Z, 0)[None], cfg)
    assert abs(vr - ref) <= 1e-4 * abs(ref), (vr, ref)

    step = ctx.get_step()
    y = ctx.reconstruct_sampled(x, 3)
    assert ctx.get_step() == step
    eps = np.stack([P.eval_eps(seed, step, n, cfg.Z, s) for s in (1, 2, 3)])
    ref_y = O.reconstruct(p64, x64, eps, cfg)
    print(f"reconstruct_sampled max err {np.abs(y - ref_y).max():.3e}")
    assert np.abs(y - ref_y).max() <= 1e-5

    step = ctx.get_step()
    total, rows = ctx.marginal_ll(x, K, rows=True)
    assert ctx.get_step() == step
    eps = np.stack([P.eval_eps(seed, step, n, cfg.Z, k + 1) for k in range(K)])
    cfg_la = O.Config(D=cfg.D, H=cfg.H, Z=cfg.Z, continuous=continuous, estimator="LA")
    out = O.forward_backward(p64, x64, eps, cfg_la, need_grad=False)
    lw, ref_rows = iw_reference(out, K)
    assert np.median(np.abs(ref_rows - lw.mean(axis=0)) / np.abs(ref_rows)) >= 20 * RTOL
    assert_matches(total, rows, ref_rows, f"marginal_ll philox continuous={continuous}")
    ctx.close()


# ------------------------------------------------------------------- (e) FVS weight noise
def test_fvs_weight_noise_matches_oracle():
    """VAEB_EST_FVS in Philox mode at 37-19-3 (P = 1658, P % 4 = 2: a partial last group): one
    update() (the weight sample drawn by fvs_sample_kernel) and one update_many() of two steps
    (the second reads the sample the first step's update wrote: zeta(step + 1)), against
    O.fvs_step with fvs_zeta and train_eps; tolerances and setup (sigma = 1e-3, three steps) of
    test_fv_weight_sampling_step.  At sigma = 1e-3 the ELBO hardly feels zeta; mu' and sigma' do
    (test_philox_oracle.py::test_fvs_case_tells_a_wrong_weight_noise_apart)."""
    c = FVS_CASE
    cfg = O.Config(**c.kw)
    assert O.num_params(cfg) % 4 != 0
    x = data_for(cfg, 8 * c.B)
    rng = np.random.default_rng(21)
    theta = [(t + 0.05 * rng.standard_normal(t.shape)).astype(np.float32) for t in O.init_params(cfg)]
    mu = [t.copy() for t in theta]
    sig = [np.full_like(t, 1e-3) for t in theta]
    zero = [np.zeros_like(t) for t in theta]
    ctx = make_ctx(c, keep_grads=False)
    ctx.set_data(x)
    ctx.set_params(O.flatten(theta))
    ctx.set_fv_state(O.flatten(mu), O.flatten(sig), O.flatten(zero), O.flatten(zero))
    ctx.set_eps_mode(0, c.seed)
    ctx.set_step(STEP)
    m64, s64 = [q.astype(np.float64) for q in mu], [q.astype(np.float64) for q in sig]
    am64, as64 = [q.astype(np.float64) for q in zero], [q.astype(np.float64) for q in zero]

    def oracle(step, b, m64, s64, am64, as64):
        zeta = O.unflatten(P.fvs_zeta(c.seed, step, ctx.P), cfg)
        eps = P.train_eps(c.seed, step, b, c.B, c.B, 0, 1, cfg.Z)
        return O.fvs_step(m64, s64, am64, as64, x[b * c.B:(b + 1) * c.B].astype(np.float64), eps, zeta, cfg)

    step = ctx.get_step()
    e = ctx.update(IDX)
    ref, m64, s64, am64, as64, _ = oracle(step, IDX, m64, s64, am64, as64)
    assert abs(e - ref) <= 1e-4 * abs(ref), (e, ref)
    ctx.epoch_elbo()
    step = ctx.get_step()
    ctx.update_many(np.array([5, 1], np.int32))
    tot, nst = ctx.epoch_elbo()
    assert nst == 2 and ctx.get_step() == step + 2
    refs = []
    for t, b in enumerate((5, 1)):
        ref, m64, s64, am64, as64, _ = oracle(step + t, b, m64, s64, am64, as64)
        refs.append(ref)
    assert abs(tot - sum(refs)) <= 1e-4 * abs(sum(refs)), (tot, refs)
    gm, gs, _, _ = ctx.get_fv_state()
    for got, want, first in ((gm, O.flatten(m64), O.flatten(mu)), (gs, O.flatten(s64), O.flatten(sig))):
        d = np.abs(got - want)
        assert d.max() <= 2 * cfg.lr + 1e-7, d.max()
        assert float((d > 1e-3 * cfg.lr).mean()) <= 1e-3
        assert rel(got - first, want - first) <= 1e-2
    assert np.array_equal(ctx.get_params(), O.flatten(theta))
    ctx.close()


# -------------------------------------------------------------------- (f) 16-bit engines
H16 = {"bf16": (1, O.bf16_round, 1e-2, 8e-2), "fp16": (2, O.fp16_round, 2e-3, 2e-2)}


@pytest.mark.parametrize("engine", list(H16))
@pytest.mark.parametrize("c", H16_CASES, ids=[c.name for c in H16_CASES])
def test_h16_philox_step_matches_rounded_oracle(c, engine):
    """One Philox-mode step of the bf16 / fp16 engine (the per-row, the 4-wide and the thin
    kernels' draw sites) against the oracle rounding where the engine rounds, on the oracle's
    draw; tolerances of test_bf16_step_parity / test_fp16_step_parity."""
    dtype, q, elbo_f, grad_f = H16[engine]
    ctx = make_ctx(c, dtype=dtype, max_eval_rows=512)
    cfg = start(c, ctx, idx=H16_IDX, acc0=1e-3, rng_seed=5)
    _, _, params, acc, _ = inputs(c, H16_IDX, 1e-3, 5)
    step = ctx.get_step()
    elbo = ctx.update(H16_IDX)
    g, newa, newp = ctx.get_grads(), ctx.get_adagrad_state(), ctx.get_params()
    ctx.close()
    _, (q_elbo, _, q_a, q_aux) = step_reference(c, step, H16_IDX, q, 1e-3, 5)
    _, (f_elbo, _, _, f_aux) = step_reference(c, step, H16_IDX, None, 1e-3, 5)
    assert abs(elbo - q_elbo) <= 1e-4 * abs(q_elbo), (elbo, q_elbo)
    assert abs(elbo - f_elbo) <= elbo_f * abs(f_elbo), (elbo, f_elbo)
    for (n, s), gg, rq, rf in zip(O.param_shapes(cfg), O.unflatten(g, cfg), q_aux["data_grads"], f_aux["data_grads"]):
        assert rel(gg.reshape(s), rq) <= 2e-3, (n, rel(gg.reshape(s), rq))
        assert rel(gg.reshape(s), rf) <= grad_f, (n, rel(gg.reshape(s), rf))
    assert rel(newa, O.flatten(q_a)) <= 4e-3
    # theta' is the fp32 Adagrad rule on the engine's own gradient
    th = O.flatten(params).astype(np.float64)
    gt = g.astype(np.float64) - th
    want = th + cfg.lr * gt / (np.sqrt(O.flatten(acc).astype(np.float64) + gt * gt) + cfg.eps)
    assert np.abs(newp - want).max() <= 1e-6 + 1e-5 * np.abs(want).max()


@pytest.mark.parametrize("engine", list(H16))
def test_h16_philox_validate_two_chunks(engine):
    """validate over two device chunks (300 rows, 160 per chunk) on the 16-bit engines: stream 0
    keyed by the row of the call; tolerance of test_bf16_validate_and_reconstruct."""
    from vaeb_amd import _lib
    dtype, q, _, _ = H16[engine]
    cfg = O.Config(D=256, H=128, Z=32)
    seed, n = (35 << 32) | 0x89ABCDE, 300
    x = data_for(cfg, n, seed=4)
    params = O.init_params(cfg)
    ctx = _lib.Context(cfg.D, cfg.H, cfg.Z, 128, max_eval_rows=160, dtype=dtype)
    ctx.set_data(x)
    ctx.set_params(O.flatten(params))
    ctx.set_eps_mode(_lib.EPS_PHILOX, seed)
    ctx.set_step(STEP)
    step = ctx.get_step()
    got = ctx.validate(x)
    ctx.close()
    ref = O.validate([p.astype(np.float64) for p in params], x.astype(np.float64),
                     P.eval_eps(seed, step, n, cfg.Z, 0)[None], cfg, q=q)
    assert abs(got - ref) <= 1e-4 * abs(ref), (got, ref)
