"""The conditions the inputs of tests/test_gpu_h16_traj.py meet, proved on the host oracle alone
(tests/h16_traj_cases.py holds the table): free-running oracle trajectories on the device's Philox
noise, in plain float64 and with the 16-bit engines' storage rounding."""
import functools

import numpy as np
import pytest

from oracle import vaeb_oracle as O
from tests import h16_traj_cases as C

QS = {"f64": None, "bf16": O.bf16_round, "fp16": O.fp16_round}


@functools.lru_cache(maxsize=None)
def run(name, qname):
    return C.free_run(C.BY_NAME[name], QS[qname])


@pytest.mark.parametrize("qname", ["f64", "bf16"])
@pytest.mark.parametrize("case", C.TRAJ_CASES, ids=lambda c: c.name)
def test_a_float64_and_bf16_stay_finite(case, qname):
    """(a) plain float64 and q = bf16_round: a finite ELBO and a finite theta' at every step."""
    for t, s in enumerate(run(case.name, qname)):
        assert np.isfinite(s.elbo) and s.finite, (t, s)


@pytest.mark.parametrize("case", [c for c in C.TRAJ_CASES if c.name.startswith("wide_")], ids=lambda c: c.name)
def test_b_wide_cases_leave_fp16_range_at_step_2(case):
    """(b) q = fp16_round: steps 0 and 1 keep z, dA2, dA1, [dMu | dLv] and dA3 within +-65504, step
    2 is the first with one outside, and theta is non-finite after it."""
    steps = run(case.name, "fp16")
    for t in (0, 1):
        assert steps[t].in_range and steps[t].finite and np.isfinite(steps[t].elbo), (t, steps[t])
    assert not steps[2].in_range, steps[2]
    assert not steps[2].finite
    # the float64 run is off theta_0 there too, and huge where fp16 overflows
    f = run(case.name, "f64")[2]
    assert f.lv_max > 15 and max(f.store_max["dLv"], f.store_max["dMu"]) > 1e6 and f.store_max["dA3"] > 1e5, f


def test_c_narrow_case_stays_in_fp16_range():
    """(c) narrow_thin with q = fp16_round: within +-65504 with a finite theta for all 5 steps, and
    max |lv| at step 2 above 5 -- the state really is off theta_0 (where |lv| < 0.5)."""
    steps = run("narrow_thin", "fp16")
    assert len(steps) == len(C.ORDER) == 5
    for t, s in enumerate(steps):
        assert s.in_range and s.finite and np.isfinite(s.elbo), (t, s)
    assert steps[2].lv_max > 5, steps[2]
    assert steps[0].lv_max < 0.5, steps[0]


def gauss_step(case, q):
    x = C.data_of(case)
    return C.oracle_step(case, C.theta0(case), C.acc0(case), x, case.idx, C.STEP0, q)


def test_d_gaussian_pair_straddles_fp16_range():
    """(d) gauss_lowvar_out: max |dA2| or max |dA6| above 65504 with a finite float64 ELBO (and a
    finite fp16-rounded ELBO beside a non-finite theta': the silent failure); gauss_lowvar_in: both
    below 32768, every rounding finite."""
    out, inn = C.BY_NAME["gauss_lowvar_out"], C.BY_NAME["gauss_lowvar_in"]
    e, p, _, aux = gauss_step(out, None)
    m = C.store_max(aux)
    assert np.isfinite(e) and all(np.isfinite(v).all() for v in p)
    assert max(m["dA2"], m["dA6"]) > C.F16_MAX, m
    assert all(m[k] <= C.F16_MAX for k in ("z", "dA1", "dMu", "dLv", "dA3")), m   # the decoder's stores alone
    eh, ph, _, auxh = gauss_step(out, O.fp16_round)
    assert np.isfinite(eh) and not all(np.isfinite(v).all() for v in ph)
    assert not C.in_f16_range(auxh)
    eb, pb, _, _ = gauss_step(out, O.bf16_round)
    assert np.isfinite(eb) and all(np.isfinite(v).all() for v in pb)
    for q in (None, O.fp16_round, O.bf16_round):
        e, p, _, aux = gauss_step(inn, q)
        m = C.store_max(aux)
        assert np.isfinite(e) and all(np.isfinite(v).all() for v in p)
        assert max(m["dA2"], m["dA6"]) < 32768 and C.in_f16_range(aux), m


def test_raised_bounds_carry_their_host_evidence():
    """Every raised per-step bound names a case, dtype, step and quantity of the table, exceeds the
    module tolerance it replaces and is at most 4 x the recorded float32-vs-float64 difference."""
    for (case, dtype, step, quantity), (b, diff) in C.RAISED.items():
        assert case in C.BY_NAME and dtype in ("bf16", "fp16") and 0 <= step < len(C.ORDER)
        kind = quantity if quantity in ("elbo", "acc") else "grad"
        assert quantity in ("elbo", "acc") or quantity in C.cfg_of(C.BY_NAME[case]).names
        assert C.TOL[kind] < b <= 4 * diff, (case, dtype, step, quantity)
