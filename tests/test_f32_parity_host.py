"""Host checks (no GPU) of the fp32 step engine's per-element parity test
(tests/f32_parity_cases.py, tests/test_gpu_f32_parity.py): that its inputs are fair and that it can
fail where today's criteria cannot.

Inputs (test_inputs_are_fair, test_theta0_is_where_todays_tests_sit).  Every x30 and start-up case
meets fair()'s conditions at seed 3 and every gradient bound is <= 1e-4.  At theta_0, where every
other oracle comparison of this engine's step runs, the same statistics read: no |h| above 0.45
(below 0.3 at the nine shapes with D < 560; 0.41-0.45 at mnist20, frey2_gauss and mean_map_frey10),
|y - 1/2| < 0.02, |lv| < 0.09.

Mutants (test_new_criterion_rejects_what_todays_accepts).  Wrong gradients built on the oracle
side, in a copied backward (backward() below, pinned against the oracle's) or from its gradient:
  corner  in W3, W2 and W1 the element [15, 16] -- the last row of one 16-tile, the first column of
          the next -- displaced by 1e-3 of the block's max|g|;
  tanh    tanh' = 1 - |h| where |h| > 0.95 (1 - h^2 elsewhere);
  explv   exp(lv) in dLv replaced by 1 + lv + lv^2 / 2.
Each is accepted by rel <= 1e-4 norm-wise per tensor at theta_0 and rejected by the per-element
criterion at x30, at the shapes of MUTANT_SHAPES.  Measured (norm-wise at theta_0 / largest err at
x30): corner 7.1e-5 / 1.0e-3 (mnist20 W1), 8.4e-5 / 1.0e-3 (slab_partial_k W3); tanh 0 / 3.0e-2
(mnist20; at theta_0 no |h| reaches 0.95, the mutant is the oracle); explv 5.3e-6 / 4.0e-2
(odd_shapes), 3.9e-5 / 5.5e-1 (slab_partial_k), 7.0e-6 / 3.3e-1 (gauss_cap).  Not counted as
evidence: explv at mnist20 is caught at theta_0 already (3.1e-4 norm-wise in W5), and the corner
mutant in a block of fewer than ~1e4 elements (odd_shapes, gauss_cap: 1.2e-4 to 3.8e-4 norm-wise).

Optimizer (test_optimizer_check_*).  The check accepts the float32 adagrad_update and rejects an
update that adds the prior twice.  It does NOT resolve a dropped mean_map decay, and no
per-element check of a float32 theta' can: the decay is lr eps theta^2 = 1e-8 theta^2, between 0.08
and 0.17 |theta| of theta's float32 spacing, so the rounding of theta' itself is larger.
Measured at mean_map_frey10 x30: the decay is at most 1.1e-8 (0.16 spacings of its theta), 1.1e-6
of max|step|; the float32 restatement of the rule is off by 3.4e-6 and the bound is 5.5e-5 (start-up
state: 5.7e-11, 0.01 spacings).  test_mean_map_decay_is_below_float32_spacing
keeps these figures on record instead of asserting a rejection that cannot happen; the decay
stays covered by tests/test_oracle_pins.py and the mean_map rows of tests/test_gpu_step.py.
"""
import dataclasses

import numpy as np
import pytest

from oracle import vaeb_oracle as O
from tests import f32_parity_cases as C

CASE_PARAMS = pytest.mark.parametrize("name,state", C.CASES, ids=C.CASE_IDS)
H_THETA0_WIDE = ("mnist20", "frey2_gauss", "mean_map_frey10")     # D >= 560: max|h| 0.41-0.45 at theta_0


def rel(a, b):
    """The norm-wise measure of tests/test_gpu_step.py."""
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.fixture(scope="module")
def theta0_step():
    cache = {}

    def get(name):
        if name not in cache:
            x, params, acc, eps = C.draw(name, "theta0", C.SEED0)
            cache[name] = C.make_step(name, "theta0", C.config(name), C.batch(name), x, C.IDX, params, acc, eps, C.SEED0)
        return cache[name]
    return get


# ------------------------------------------------------------------ 1. the inputs
@CASE_PARAMS
def test_inputs_are_fair(name, state):
    st = C.case(name, state)
    s = st.stats
    print(f"{name}-{state} (seed {st.seed}): " + " ".join(f"{k} {v:.3g}" for k, v in s.items()))
    gk = C.grad_keys(st.cfg)
    worst = max(gk, key=lambda k: st.bound[k])
    print(f"    gradient restatement {min(st.restate[k] for k in gk):.1e} .. {max(st.restate[k] for k in gk):.1e}; "
          f"largest gradient bound {worst} {st.bound[worst]:.1e}; value {st.restate_value:.1e}")
    assert st.seed == C.SEED0                      # the seed the tables of the GPU test were recorded at
    assert C.fair_reasons(st.cfg, state, s) == []
    assert set(gk) <= set(st.bound) and set(C.ACTS) <= set(st.bound)
    for k in gk:
        assert st.bound[k] <= C.GRAD_CAP, (k, st.bound[k])
        assert st.restate[k] > 0, k                # a zero restatement error would ask for bit equality
    assert st.restate_value <= C.VALUE_RTOL / C.MARGIN
    # the conditions spelled out, so that a change to fair_reasons cannot empty them
    if state == "x30":
        assert s["h_sat"] >= 0.05 and s["hd_sat"] >= 0.05 and s["hd_open"] >= 0.4
        assert 1.0 <= s["lv_max"] <= 8.0
        assert s["y_min"] < 0.2 and s["y_max"] > 0.8
        if st.cfg.continuous:
            assert s["a6_min"] < -1.0 and s["a6_max"] > 1.0 and max(-s["a6_min"], s["a6_max"]) <= 12.0
        assert all(np.all(a == np.float32(C.ACC0)) for a in st.acc)
    else:
        assert s["h_sat"] >= 0.1 or s["lv_max"] >= 1.0
        assert all(a.min() >= 0 and a.max() > 0 for a in st.acc)


@pytest.mark.parametrize("name", C.X30)
def test_theta0_is_where_todays_tests_sit(name, theta0_step):
    s = theta0_step(name).stats
    print(f"{name} theta_0: max|h| {s['h_max']:.3f} max|y - 1/2| {s['y_off']:.3f} max|lv| {s['lv_max']:.3f}")
    assert s["h_max"] < (0.5 if name in H_THETA0_WIDE else 0.3)
    assert s["h_sat"] == 0 and s["hd_sat"] == 0
    assert s["y_off"] < 0.05 and s["lv_max"] < 0.1
    if C.config(name).continuous:
        assert max(-s["a6_min"], s["a6_max"]) < 0.1


def test_x30_scale_rule():
    cfg = C.config("frey2_gauss")
    kin = C.layer_inputs(cfg)
    assert kin == {"W3": 560, "b3": 560, "W4": 200, "W5": 200, "b4": 200, "b5": 200, "W1": 2, "b1": 2,
                   "W2": 200, "W6": 200, "b2": 200, "b6": 200}
    p0, _ = C.theta0(cfg, 100, 3)
    for n, a, b in zip(cfg.names, p0, C.scale_params(cfg, p0)):
        f = 30.0 * min(1.0, (64.0 / kin[n]) ** 0.5)
        assert np.allclose(b, a * f, rtol=1e-6, atol=0), n


# ------------------------------------------------------------------ 2. mutants
def backward(cfg, params, x, eps, out, dtanh=None, exp_lv=None):
    """oracle.forward_backward's reverse mode in float64 from its stored forward `out`, with the
    two functions a mutant replaces; {"gW3": ...} data gradients."""
    p = dict(zip(cfg.names, params))
    B, L, Z = x.shape[0], eps.shape[0], cfg.Z
    dtanh = dtanh or (lambda h: 1 - h * h)
    exp_lv = exp_lv or np.exp
    s = 1.0 / B if cfg.objective == "mean_map" else 1.0
    sl = s / L
    h, mu, lv, z, hd, y = (out[k] for k in ("h", "mu", "lv", "z", "hd", "y"))
    std = np.exp(0.5 * lv)
    xr = np.tile(x, (L, 1))
    zf = z.reshape(L * B, Z)
    g = {}
    if cfg.continuous:
        r, e = xr - y, np.exp(-out["a6"])
        dA2 = r * e * y * (1 - y) * sl
        dA6 = (-0.5 + 0.5 * r * r * e) * sl
        g["W6"], g["b6"] = hd.T @ dA6, dA6.sum(0)
    else:
        dA2 = (xr - y) * sl
    g["W2"], g["b2"] = hd.T @ dA2, dA2.sum(0)
    dHd = dA2 @ p["W2"].T + (dA6 @ p["W6"].T if cfg.continuous else 0.0)
    dA1 = dHd * dtanh(hd)
    g["W1"], g["b1"] = zf.T @ dA1, dA1.sum(0)
    dZ = (dA1 @ p["W1"].T).reshape(L, B, Z)
    if cfg.estimator == "LA":
        dMu = dZ.sum(0) + sl * (-z).sum(0)
        dLv = (dZ * 0.5 * std[None] * eps).sum(0) + sl * (0.5 - 0.5 * z * std[None] * eps).sum(0)
    else:
        dMu = dZ.sum(0) - s * mu
        dLv = (dZ * 0.5 * std[None] * eps).sum(0) + s * 0.5 * (1 - exp_lv(lv))
    g["W4"], g["b4"], g["W5"], g["b5"] = h.T @ dMu, dMu.sum(0), h.T @ dLv, dLv.sum(0)
    dA3 = (dMu @ p["W4"].T + dLv @ p["W5"].T) * dtanh(h)
    g["W3"], g["b3"] = x.T @ dA3, dA3.sum(0)
    return {"g" + n: g[n] for n in cfg.names}


def run_backward(st, **kw):
    B = st.B
    return backward(st.cfg, C.f64(st.params), st.x[st.idx * B:(st.idx + 1) * B].astype(np.float64),
                    st.eps.astype(np.float64), st.out64, **kw)


def corner(st):
    g = {k: st.q64[k].copy() for k in C.grad_keys(st.cfg)}
    for k in ("gW3", "gW2", "gW1"):
        i, j = min(15, g[k].shape[0] - 1), min(16, g[k].shape[1] - 1)
        g[k][i, j] += 1e-3 * np.abs(g[k]).max()
    return g


MUTANTS = {
    "corner": corner,
    "tanh": lambda st: run_backward(st, dtanh=lambda h: np.where(np.abs(h) > 0.95, 1 - np.abs(h), 1 - h * h)),
    "explv": lambda st: run_backward(st, exp_lv=lambda lv: 1 + lv + lv * lv / 2),
}
MUTANT_SHAPES = {"corner": ("mnist20", "slab_partial_k"), "tanh": ("mnist20", "frey2_gauss", "odd_shapes"),
                 "explv": ("odd_shapes", "slab_partial_k", "gauss_cap")}
MUTANT_CASES = [(m, n) for m, ns in MUTANT_SHAPES.items() for n in ns]


@pytest.mark.parametrize("name", ["mnist20", "frey2_gauss", "atomic_LA_L2", "mean_map_frey10"])
def test_copied_backward_is_the_oracles(name, theta0_step):
    for st in (theta0_step(name), C.case(name, "x30")):
        g = run_backward(st)
        for k in g:
            assert np.allclose(g[k], st.q64[k], rtol=1e-12, atol=1e-15 * np.abs(st.q64[k]).max()), (name, st.state, k)


@pytest.mark.parametrize("mutant,name", MUTANT_CASES, ids=[f"{m}-{n}" for m, n in MUTANT_CASES])
def test_new_criterion_rejects_what_todays_accepts(mutant, name, theta0_step):
    t0, st = theta0_step(name), C.case(name, "x30")
    g0 = MUTANTS[mutant](t0)
    today = {k: rel(g0[k], t0.q64[k]) for k in g0}
    e = C.errors(MUTANTS[mutant](st), st.q64)
    bad = C.rejected(e, st.bound)
    print(f"{mutant} {name}: norm-wise at theta_0 {max(today.values()):.1e} (accepted <= 1e-4); per element at "
          f"x30 rejects {bad}, largest err {max(e.values()):.1e}")
    assert max(today.values()) <= 1e-4, today          # today's criterion, where today's tests run
    assert bad, e
    if mutant == "corner":
        assert set(bad) == {"gW3", "gW2", "gW1"}
        assert all(rel(MUTANTS[mutant](st)[k], st.q64[k]) <= 1e-4 for k in bad)   # norm-wise blind at x30 too
    # the unmutated oracle passes its own criterion
    assert C.rejected(C.errors({k: st.q64[k] for k in e}, st.q64), st.bound) == []


# ------------------------------------------------------------------ 3. the optimizer check
def float32_update(cfg, st, g, twice=False):
    th, ac = st.theta(), st.acc_flat()
    gt = g - np.float32((2.0 if twice else 1.0) * C.prior_coef(cfg)) * th
    (p1,), (a1,) = O.adagrad_update([th], [ac], [gt.astype(np.float32)], cfg)
    return p1, a1


@pytest.mark.parametrize("name,state", [("mnist20", "x30"), ("mnist20", "startup"), ("mean_map_frey10", "x30"),
                                        ("mean_map_frey10", "startup"), ("odd_shapes", "x30")])
def test_optimizer_check_accepts_the_float32_rule(name, state):
    st = C.case(name, state)
    g = O.flatten(st.out64["data_grads"]).astype(np.float32)
    e, restate, bound = C.optimizer_check(st.cfg, st.theta(), st.acc_flat(), g, *float32_update(st.cfg, st, g))
    print(C.table_line(f"{name}-{state} float32 rule", e, restate, bound))
    assert C.rejected(e, bound) == []
    assert all(e[k] == restate[k] for k in e)


@pytest.mark.parametrize("name,state", [("mnist20", "x30"), ("mnist20", "startup"), ("odd_shapes", "x30")])
def test_optimizer_check_rejects_the_prior_added_twice(name, state):
    st = C.case(name, state)
    g = O.flatten(st.out64["data_grads"]).astype(np.float32)
    e, _, bound = C.optimizer_check(st.cfg, st.theta(), st.acc_flat(), g, *float32_update(st.cfg, st, g, twice=True))
    bad = C.rejected(e, bound)
    print(f"{name}-{state} prior twice: rejects {len(bad)} of {len(e)} blocks, largest err {max(e.values()):.1e}")
    assert any(k.startswith("dth.W") for k in bad) and any(k.startswith("dac.W") for k in bad)


def test_optimizer_check_rejects_a_stale_accumulator():
    """An update that divides by sqrt(g^2) instead of sqrt(acc + g^2) (the accumulator read as zero)."""
    st = C.case("mnist20", "startup")
    g = O.flatten(st.out64["data_grads"]).astype(np.float32)
    th, gt = st.theta(), g - st.theta()
    (p1,), _ = O.adagrad_update([th], [np.zeros_like(th)], [gt], st.cfg)
    _, a1 = float32_update(st.cfg, st, g)
    e, _, bound = C.optimizer_check(st.cfg, th, st.acc_flat(), g, p1, a1)
    bad = C.rejected(e, bound)
    assert any(k.startswith("dth.") for k in bad) and not any(k.startswith("dac.") for k in bad)


@pytest.mark.parametrize("state", ["x30", "startup"])
def test_mean_map_decay_is_below_float32_spacing(state):
    """The figures behind the module docstring's last paragraph: an update without the mean_map
    decay differs from the rule by less than the float32 restatement of the rule does, so the
    per-element check accepts it -- and so would any other reading of a float32 theta'."""
    st = C.case("mean_map_frey10", state)
    cfg = st.cfg
    g = O.flatten(st.out64["data_grads"]).astype(np.float32)
    th, ac = st.theta(), st.acc_flat()
    (p1,), (a1,) = O.adagrad_update([th], [ac], [g], dataclasses.replace(cfg, objective="sum_prior"))
    e, restate, bound = C.optimizer_check(cfg, th, ac, g, p1, a1)
    decay = cfg.lr * cfg.eps * th.astype(np.float64) ** 2
    spacing = np.spacing(np.abs(th)).astype(np.float64)
    d64, _ = C.adagrad_deltas(cfg, th, ac, g, np.float64)
    k = max((k for k in e if k.startswith("dth.")), key=lambda k: e[k])
    print(f"mean_map_frey10-{state}: decay <= {decay.max():.1e} = {np.max(decay / spacing):.2f} spacings of theta, "
          f"{decay.max() / np.abs(d64).max():.1e} of max|step|; without it {k} err {e[k]:.1e}, restatement "
          f"{restate[k]:.1e}, bound {bound[k]:.1e}")
    assert np.max(decay / spacing) < 0.5          # below half a spacing: theta' cannot carry it
    assert C.rejected(e, bound) == []
