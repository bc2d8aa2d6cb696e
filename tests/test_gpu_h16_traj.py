"""16-bit engine steps at the state a training run actually starts from: theta_0, ZERO Adagrad
accumulators, device Philox noise, then a few Adagrad steps (tests/h16_traj_cases.py holds the
cases, tests/test_h16_traj_host.py the proof of what their inputs do on the oracle).

Teacher-forced per-step parity: before every step the device's own theta, accumulators and step
counter are read back, the step runs (vaeb_update), and the rounded oracle runs ONE step from
exactly that state on its own draw of that step's Philox noise.  Bounds: the 16-bit modules'
single-step tolerances (ELBO 1e-4 relative to the rounded oracle, data gradients 2e-3 norm-wise
per tensor, Adagrad accumulator 4e-3; theta' = the fp32 Adagrad rule on the engine's own gradient
within 1e-6 + 1e-5 max), raised per (case, dtype, step, quantity) only by h16_traj_cases.RAISED.

fp16 leaves its range (+-65504) at step index 2 of the wide cases and in the Gaussian decoder at
b6 = -14: the step must report VAEB_ERR_NUMERIC naming the fp16 range, through vaeb_update and
through vaeb_update_many + vaeb_epoch_elbo, and the context must step again once its state is
restored."""
import functools

import numpy as np
import pytest

from oracle import vaeb_oracle as O
from tests import h16_traj_cases as C

pytestmark = pytest.mark.gpu

QS = {"bf16": O.bf16_round, "fp16": O.fp16_round}


def make_ctx(case, dt, use_graph=True, keep_grads=True):
    from vaeb_amd import _lib
    cfg = C.cfg_of(case)
    ctx = _lib.Context(cfg.D, cfg.H, cfg.Z, case.B, decoder=int(cfg.continuous), keep_grads=keep_grads,
                       max_eval_rows=case.B, use_graph=use_graph,
                       dtype=_lib.DTYPE_F16 if dt == "fp16" else _lib.DTYPE_BF16)
    ctx.set_data(C.data_of(case))
    reset(ctx, case)
    return ctx


def reset(ctx, case):
    from vaeb_amd import _lib
    ctx.set_params(O.flatten(C.theta0(case, np.float32)))
    ctx.set_adagrad_state(O.flatten(C.acc0(case, np.float32)))
    ctx.set_eps_mode(_lib.EPS_PHILOX, C.seed_of(case))
    ctx.set_step(C.STEP0)


def forced_step(ctx, case, dt, t, idx, x):
    """One teacher-forced step: the device's step from its own state against the rounded oracle's
    step from that state.  Returns the figures (printed before anything is asserted) or, when
    vaeb_update raised, {"raised": message, "oracle_in_range": ...}."""
    from vaeb_amd import _lib
    cfg = C.cfg_of(case)
    th, ac, st = ctx.get_params(), ctx.get_adagrad_state(), ctx.get_step()
    assert st == C.STEP0 + t
    q_elbo, _, q_a, aux = C.oracle_step(case, O.unflatten(th, cfg), O.unflatten(ac, cfg), x, idx, st, QS[dt])
    rec = {"t": t, "oracle_in_range": C.in_f16_range(aux), "store_max": C.store_max(aux), "q_elbo": float(q_elbo)}
    try:
        elbo = ctx.update(idx)
    except _lib.VaebError as e:
        rec["raised"] = str(e)
        print(case.name, dt, "step", t, "raised:", rec["raised"], "oracle stores", rec["store_max"])
        return rec
    g, newa, newp = ctx.get_grads(), ctx.get_adagrad_state(), ctx.get_params()
    rec["elbo"] = elbo
    rec["finite"] = bool(np.isfinite(elbo) and np.isfinite(newp).all() and np.isfinite(newa).all())
    with np.errstate(all="ignore"):
        rec["err"] = {"elbo": abs(elbo - q_elbo) / abs(q_elbo), "acc": C.rel(newa, O.flatten(q_a))}
        for (n, s), gg, rq in zip(O.param_shapes(cfg), O.unflatten(g, cfg), aux["data_grads"]):
            rec["err"][n] = C.rel(gg.reshape(s), rq)
        # theta' is the fp32 Adagrad rule applied to the engine's own gradient
        th64 = th.astype(np.float64)
        gt = g.astype(np.float64) - th64
        want = th64 + cfg.lr * gt / (np.sqrt(ac.astype(np.float64) + gt * gt) + cfg.eps)
        rec["theta_err"] = float(np.abs(newp - want).max())
        rec["theta_tol"] = float(1e-6 + 1e-5 * np.abs(want).max())
    for k, v in rec["err"].items():
        print(f"{case.name} {dt} step {t} {k}: err {v:.3e} bound {C.bound(case.name, dt, t, k):.1e}")
    print(f"{case.name} {dt} step {t} theta': err {rec['theta_err']:.3e} tol {rec['theta_tol']:.3e}; "
          f"elbo {elbo:.6g} oracle {q_elbo:.6g}; max|lv| {np.abs(aux['lv']).max():.3g}")
    return rec


def check_step(case, dt, rec):
    t = rec["t"]
    assert "raised" not in rec, (case.name, dt, t, rec["raised"])
    assert rec["finite"], (case.name, dt, t)
    for k, v in rec["err"].items():
        assert v <= C.bound(case.name, dt, t, k), (case.name, dt, t, k, v)
    assert rec["theta_err"] <= rec["theta_tol"], (case.name, dt, t, rec["theta_err"], rec["theta_tol"])


@functools.lru_cache(maxsize=None)
def forced_run(name, dt):
    """The per-step run of a trajectory case: its records (ending with the step that raised, if
    one did) and, when all 5 steps ran, the final theta, accumulators and epoch ELBO sum."""
    case = C.BY_NAME[name]
    x = C.data_of(case)
    ctx = make_ctx(case, dt)
    recs, final = [], None
    try:
        for t, idx in enumerate(C.ORDER):
            recs.append(forced_step(ctx, case, dt, t, idx, x))
            if "raised" in recs[-1]:
                break
        else:
            final = (ctx.get_params(), ctx.get_adagrad_state(), ctx.epoch_elbo())
    finally:
        ctx.close()
    return recs, final


@pytest.mark.parametrize("case", C.TRAJ_CASES, ids=lambda c: c.name)
def test_bf16_per_step_parity(case):
    recs, final = forced_run(case.name, "bf16")
    assert len(recs) == len(C.ORDER) and final is not None
    for rec in recs:
        check_step(case, "bf16", rec)
    if case.name.startswith("wide_"):
        # the device's own trajectory reaches the state the host proof describes
        assert not recs[2]["oracle_in_range"], recs[2]["store_max"]


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("case", C.TRAJ_CASES, ids=lambda c: c.name)
def test_bf16_update_many_is_the_per_step_run(case, use_graph):
    """One vaeb_update_many(order) on a fresh context == the per-step vaeb_update run, bit for bit
    in theta, accumulators and the epoch ELBO sum, as a graph replay and as eager launches."""
    _, final = forced_run(case.name, "bf16")
    assert final is not None
    ctx = make_ctx(case, "bf16", use_graph=use_graph)
    ctx.update_many(np.array(C.ORDER, np.int32))
    got = (ctx.get_params(), ctx.get_adagrad_state(), ctx.epoch_elbo())
    ctx.close()
    assert got[2] == final[2], (got[2], final[2])
    assert np.array_equal(got[0], final[0])
    assert np.array_equal(got[1], final[1])


def test_fp16_narrow_per_step_parity():
    case = C.BY_NAME["narrow_thin"]
    recs, final = forced_run(case.name, "fp16")
    assert len(recs) == len(C.ORDER) and final is not None
    for rec in recs:
        assert rec["oracle_in_range"], rec["store_max"]
        check_step(case, "fp16", rec)


def assert_fp16_range_error(msg):
    assert "error -6:" in msg, msg                      # VAEB_ERR_NUMERIC
    assert "fp16 range" in msg and "fixed-point" not in msg, msg


WIDE = [c for c in C.TRAJ_CASES if c.name.startswith("wide_")]


@pytest.mark.parametrize("case", WIDE, ids=lambda c: c.name)
def test_fp16_wide_reports_the_step_that_leaves_its_range(case):
    recs, _ = forced_run(case.name, "fp16")
    assert len(recs) == 3, [r.get("raised") for r in recs]
    for rec in recs[:2]:
        assert rec["oracle_in_range"], rec["store_max"]
        check_step(case, "fp16", rec)
    assert not recs[2]["oracle_in_range"], recs[2]["store_max"]
    assert "raised" in recs[2]
    assert_fp16_range_error(recs[2]["raised"])


@pytest.mark.parametrize("case", WIDE, ids=lambda c: c.name)
def test_fp16_wide_update_many_reports_and_recovers(case):
    """vaeb_update_many(order) + vaeb_epoch_elbo reports the same error; after theta_0 and zero
    accumulators are restored the context steps again and its step-0 ELBO is the first run's."""
    from vaeb_amd import _lib
    recs, _ = forced_run(case.name, "fp16")
    ctx = make_ctx(case, "fp16")
    ctx.update_many(np.array(C.ORDER, np.int32))
    with pytest.raises(_lib.VaebError) as ei:
        ctx.epoch_elbo()
    assert_fp16_range_error(str(ei.value))
    reset(ctx, case)
    e0 = ctx.update(C.ORDER[0])
    e1 = ctx.update(C.ORDER[1])
    with pytest.raises(_lib.VaebError) as ei:          # and the per-step form on the same context
        ctx.update(C.ORDER[2])
    assert_fp16_range_error(str(ei.value))
    reset(ctx, case)
    e0b = ctx.update(C.ORDER[0])
    ctx.close()
    assert e0 == recs[0]["elbo"] and e1 == recs[1]["elbo"], (e0, e1, recs[0]["elbo"], recs[1]["elbo"])
    assert e0b == recs[0]["elbo"]


# The engine's other launch forms of the guarded stores (switches read at context creation):
# unforked -- dhd shares a grid with dW2 (EpiDTanh) and dz is its own split-K / thin launch;
# dA1 / dA3 on the untransposed product (EpiDTanh); dhd transposed without the fused dz; the
# latent block on the 16-byte latent kernels instead of the thin launches.
FORMS = [("wide_thin", "VAEB_BF_FORK", "0"), ("wide_split", "VAEB_BF_FORK", "0"),
         ("wide_thin", "VAEB_BF_DTT", "0"), ("wide_split", "VAEB_BF_DTT", "0"),
         ("wide_thin", "VAEB_BF_DZFUSE", "0"), ("wide_split", "VAEB_BF_DZFUSE", "0"),
         ("wide_thin", "VAEB_BF_THIN", "0")]


@pytest.mark.parametrize("name,var,val", FORMS, ids=[f"{n}-{v}={x}" for n, v, x in FORMS])
def test_fp16_wide_other_launch_forms_report_too(name, var, val, monkeypatch):
    from vaeb_amd import _lib
    case = C.BY_NAME[name]
    recs, _ = forced_run(name, "fp16")      # (the default forms: before the switch is set)
    monkeypatch.setenv(var, val)
    ctx = make_ctx(case, "fp16", keep_grads=False)
    try:
        e0 = ctx.update(C.ORDER[0])
        assert abs(e0 - recs[0]["q_elbo"]) <= C.TOL["elbo"] * abs(recs[0]["q_elbo"]), (e0, recs[0]["q_elbo"])
        assert np.isfinite(ctx.update(C.ORDER[1]))
        with pytest.raises(_lib.VaebError) as ei:
            ctx.update(C.ORDER[2])
        assert_fp16_range_error(str(ei.value))
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def gauss_run(name, dt):
    case = C.BY_NAME[name]
    ctx = make_ctx(case, dt)
    try:
        return forced_step(ctx, case, dt, 0, case.idx, C.data_of(case))
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["gauss_lowvar_in", "gauss_lowvar_out"])
def test_bf16_gaussian_low_variance_parity(name):
    check_step(C.BY_NAME[name], "bf16", gauss_run(name, "bf16"))


def test_fp16_gaussian_low_variance_inside_range():
    rec = gauss_run("gauss_lowvar_in", "fp16")
    assert rec["oracle_in_range"], rec["store_max"]
    check_step(C.BY_NAME["gauss_lowvar_in"], "fp16", rec)


def test_fp16_gaussian_low_variance_outside_range_is_reported():
    """b6 = -14: dA2 | dA6 leave fp16's range while the step's ELBO is finite -- the step raises."""
    rec = gauss_run("gauss_lowvar_out", "fp16")
    assert not rec["oracle_in_range"] and np.isfinite(rec["q_elbo"]), rec
    assert "raised" in rec
    assert_fp16_range_error(rec["raised"])
