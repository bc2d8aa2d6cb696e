"""The 16-bit step engine per stage, from its own stored operands, off theta_0 (bf16 and fp16).

Case table, stage functions and criterion: tests/h16_stage_cases.py; what the criterion lets through
and what it rejects: tests/test_h16_stage_host.py.  Per case and dtype: ONE update() with host eps and
keep_grads, one read of every buffer of the step (vaeb_get_h16, include/vaeb_diag.h), every stage judged
against its float64 value computed from the inputs the kernel itself read:
  * the shadow is Q(theta) before the step and Q(theta') after it, bit for bit; the eps buffer is the
    pushed noise, bit for bit;
  * h, z, hd, dA2 (| dA6), dA1, [dMu | dLv], dA3: |v - t| <= ulp16(t) / 2 + tau per element; tau is raised
    for h / hd at theta_0 only (h16_stage_cases.RAISED: 16 x the error of the float32 NumPy restatement of
    the epilogue's tanh), and a listed stage that does not exceed its unraised tau on the device, or an
    unlisted one that does, fails the test;
  * mu, lv and every weight gradient: |C - ref| <= 1e-5 (|A| |B|) per element; every bias gradient within
    sum ulp16(stored) / 2 + 2^-23 sum |stored| of its stored operand's column sum;
  * rows of a buffer past the step's L B (B) rows are what the step found there: the operand views of
    engine_bf16.inc bf_mats end at row L B (B), so no GEMM reads them and nothing may write them (the
    contexts are created with 16 rows of spare capacity);
  * the step's value within 1e-4 of the rounded float64 oracle; theta' - theta and acc' - acc per block by
    f32_parity_cases.optimizer_check on the gradient the device reports.
Each test prints the stage nearest to its bound (device / restatement / bound) and, per 16-bit stage, the
share of elements that are not Q(t).  A failure names the stage, the element's (row, column), its 16-tile
and 64-block and the three numbers.
"""
import numpy as np
import pytest

from oracle import vaeb_oracle as O
from tests import f32_parity_cases as F
from tests import h16_stage_cases as C

pytestmark = pytest.mark.gpu

EST = {"LB": 0, "LA": 1}
OBJ = {"sum_prior": 0, "mean_map": 1}
SPARE = 16                 # rows of capacity past B: the pad rows a step must leave alone
BUFFERS = ("h", "z", "hd", "dA", "dA1", "dml", "dA3")


def capacity(c):
    """{buffer: elements} of a context created with max_eval_rows = B + SPARE (vaeb_diag.h)."""
    cfg = c.cfg
    R = F.r16(c.B + SPARE)
    RL, Dn = R * cfg.L, cfg.D * (2 if cfg.continuous else 1)
    return {"h": R * cfg.H, "z": RL * cfg.Z, "hd": RL * cfg.H, "dA": RL * Dn, "dA1": RL * cfg.H, "dml": R * 2 * cfg.Z,
            "dA3": R * cfg.H}


def valid(c):
    cfg, B, LB = c.cfg, c.B, c.cfg.L * c.B
    Dn = cfg.D * (2 if cfg.continuous else 1)
    return {"h": B * cfg.H, "z": LB * cfg.Z, "hd": LB * cfg.H, "dA": LB * Dn, "dA1": LB * cfg.H, "dml": B * 2 * cfg.Z,
            "dA3": B * cfg.H}


def run_case(name, state, dtype):
    """(table line, flipped shares, failures) of one device step of a table case."""
    from vaeb_amd import _lib
    c = C.case(name, state)
    cfg, B = c.cfg, c.B
    nw = sum(int(np.prod(s)) for n, s in O.param_shapes(cfg) if n.startswith("W"))
    ctx = _lib.Context(cfg.D, cfg.H, cfg.Z, B, L=cfg.L, decoder=int(cfg.continuous), estimator=EST[cfg.estimator],
                       objective=OBJ[cfg.objective], lr=cfg.lr, keep_grads=True, max_eval_rows=B + SPARE,
                       dtype=_lib.DTYPE_BF16 if dtype == "bf16" else _lib.DTYPE_F16)
    try:
        ctx.set_data(c.x)
        ctx.set_params(c.theta())
        ctx.set_adagrad_state(c.acc_flat())
        ctx.set_eps_mode(_lib.EPS_HOST)
        ctx.push_eps(c.eps)
        shadow0 = ctx.get_shadow(nw)
        cap, val = capacity(c), valid(c)
        before = {k: ctx.get_h16(k, cap[k]) for k in BUFFERS}
        value = ctx.update(C.IDX)
        dev, grads, g = C.read_step(ctx, c, dtype)
        after = {k: ctx.get_h16(k, cap[k]) for k in BUFFERS}
        theta1, acc1 = ctx.get_params(), ctx.get_adagrad_state()
        shadow1 = ctx.get_shadow(nw)
    finally:
        ctx.close()
    bad = []
    if not np.array_equal(shadow0, C.to_bits(c.theta()[:nw], dtype)):
        bad.append("shadow before the step is not Q(theta)")
    if not np.array_equal(shadow1, C.to_bits(theta1[:nw], dtype)):
        bad.append("shadow after the step is not Q(theta')")
    if not np.array_equal(dev["eps"].astype(np.float32), c.eps):
        bad.append("the eps buffer is not the pushed noise")
    for k in BUFFERS:
        if not np.array_equal(before[k][val[k]:], after[k][val[k]:]):
            bad.append(f"rows of {k} past the step's were written")
    f = C.judge(c, dtype, dev, grads)
    bad += [x.line() for x in C.rejected(f)]
    # a raised tau (h16_stage_cases.RAISED) is one the device does exceed unraised, and no other stage does
    over = {x.stage for x in C.rejected(C.judge(c, dtype, dev, grads, raised=False))}
    want = {k[3] for k in C.RAISED if k[:3] == (name, state, dtype)}
    if over - {x.stage for x in C.rejected(f)} != want:
        bad.append(f"stages past their unraised tau {sorted(over)}, RAISED lists {sorted(want)}")
    oe, orst, obound = F.optimizer_check(cfg, c.theta(), c.acc_flat(), g, theta1, acc1)
    bad += F.rejected(oe, obound)
    _, v64 = C.oracle_grads(c, dtype)
    vrel = abs(value - v64) / abs(v64)
    if not vrel <= C.VALUE_RTOL:
        bad.append(f"value {value} against {v64}")
    label = f"{name}-{state}-{dtype}"
    line = (C.table_line(label, f) + "  |  " + F.table_line("", oe, orst, obound).strip() + f"  |  value {vrel:.1e}")
    stages = "  ".join(f"{x.stage} {x.ratio:.2g}" + (f" ({x.flipped:.1e})" if x.kind == "stored" else "") for x in f)
    return line, f"    error / bound (share not Q(t)): {stages}", bad


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("name,state", C.CASES, ids=C.CASE_IDS)
def test_h16_step_stages(name, state, dtype):
    line, stages, bad = run_case(name, state, dtype)
    print(line)
    print(stages)
    assert not bad, "\n".join([line] + bad)


# the alternative forms of the step, as the tests of tests/test_gpu_bf16.py that compare them with each
# other at theta_0 select them: test_bf16_tile_form_switches_agree, test_bf16_gemm8_step_matches_ring_step,
# test_bf16_forked_and_single_stream_steps_agree
SETTINGS = [{"VAEB_BF_DTT": "0"}, {"VAEB_BF_DZFUSE": "0"}, {"VAEB_BF_FORK": "0"}, {"VAEB_BF_GEMM8": "15"},
            {"VAEB_BF_GEMM8": "0"}, {"VAEB_BF_DTT": "0", "VAEB_BF_FORK": "0"}]


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("name", ["bern_LB_tails", "gauss_LB"])
@pytest.mark.parametrize("env", SETTINGS, ids=["-".join(f"{k[8:]}{v}" for k, v in e.items()) for e in SETTINGS])
def test_h16_step_stages_alternative_forms(monkeypatch, env, name, dtype):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    line, stages, bad = run_case(name, "x30", dtype)
    print(" ".join(f"{k}={v}" for k, v in env.items()) + "  " + line)
    print(stages)
    assert not bad, "\n".join([line] + bad)


def test_get_h16_errors():
    """vaeb_get_h16: an unknown name or n past the capacity is VAEB_ERR_ARG (-1), an fp32 context
    VAEB_ERR_STATE (-3)."""
    from vaeb_amd import _lib
    ctx = _lib.Context(64, 32, 8, 16, max_eval_rows=16, dtype=_lib.DTYPE_BF16)
    try:
        assert ctx.get_h16("h", 16 * 32).shape == (16 * 32,) and ctx.get_h16("mu", 16 * 8).dtype == np.float32
        for name, n in (("nope", 1), ("h", 16 * 32 + 1), ("mu", 16 * 8 + 1), ("eps", 16 * 8 + 1), ("dA", 16 * 64 + 1)):
            with pytest.raises(_lib.VaebError, match=r"error -1: vaeb_get_h16"):
                ctx.get_h16(name, n)
    finally:
        ctx.close()
    ctx = _lib.Context(64, 32, 8, 16, max_eval_rows=16)
    try:
        for name in ("h", "mu"):
            with pytest.raises(_lib.VaebError, match=r"error -3: vaeb_get_h16"):
                ctx.get_h16(name, 1)
    finally:
        ctx.close()
