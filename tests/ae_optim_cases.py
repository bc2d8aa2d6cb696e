"""The layer-stack engine's update rules against tests/optim_oracle.py -- TEST HELPER ONLY: the
hyper-parameters, the conditioned states, the per-block error and the bounds shared by
tests/test_ae_optim_host.py (no GPU) and tests/test_gpu_ae_optim.py.

Inputs are the Steps of tests/ae_grad_cases.py (shapes, theta, rows, eps, the float64 gradient
g64).  A rule step starts from float32 (theta, s0, s1) and is run three ways: the float64 oracle
(float64 gradient, float64 rule), the float32 restatement (float32 gradient from the float32-fed
forward_backward, float32 rule) and the device.

Error of a parameter block and an array X of (dtheta = theta' - theta, slot 0', slot 1'):
max|X - X64| / max|X64|.  Bound: MARGIN (16) x the restatement's error in the same measure.  No
bound comes from the device.  Conditions on the inputs (asserted by the host test): every state
bound <= STATE_CAP = 1e-4, every dtheta bound <= DTHETA_CAP = 1e-2 (dtheta is dominated by the
float32 rounding of theta' beside a small step: ulp(theta) / (eta |update|)).

Conditioned state, per block with gm = max|g64| (float32, seeded): second moments
(0.5 gm)^2 U[0.25, 1], first moments and velocities 0.3 gm N(0, 1), AdaDelta's dx_ac
1e-6 U[0.25, 1] -- g / sqrt(state) stays of order 1, as acc = 1e-4 keeps it in tests/test_gpu_ae.py.
"""
import dataclasses
import functools

import numpy as np

from oracle import ae_oracle as A
from tests import ae_grad_cases as G
from tests import optim_oracle as O

STATE_CAP = G.GRAD_CAP
DTHETA_CAP = 1e-2
T0 = 9                       # the conditioned step runs at t = 10
ARRAYS = ("dtheta", "s0", "s1")

HYPERS = {
    "sga0": O.Hyper("sga", 1e-3),
    "sga": O.Hyper("sga", 1e-3, 0.9),
    "adadelta": O.Hyper("adadelta", 1.0, 0.95, eps=1e-6),
    "adam": O.Hyper("adam", 1e-3, 0.9, 0.999, 1e-8),
}
STEP_RULES = ("sga", "adadelta", "adam")


def conditioned(rule, g64, seed=0):
    """(S0, S1) float32 lists for the blocks whose float64 gradients are g64 (S1: Nones on a
    one-slot rule)."""
    rng = np.random.default_rng(20240 + seed)
    S0, S1 = [], []
    for g in g64:
        gm = float(np.abs(g).max())
        second = ((0.5 * gm) ** 2 * rng.uniform(0.25, 1.0, g.shape)).astype(np.float32)
        first = (0.3 * gm * rng.standard_normal(g.shape)).astype(np.float32)
        dx = (1e-6 * rng.uniform(0.25, 1.0, g.shape)).astype(np.float32)
        S0.append(second if rule == "adadelta" else first)
        S1.append({"sga": None, "adadelta": dx, "adam": second}[rule])
    return S0, S1


def zero_state(rule, params):
    S0 = [np.zeros_like(p) for p in params]
    return S0, [np.zeros_like(p) if O.SLOTS[rule] == 2 else None for p in params]


def rel_err(x, x64):
    return float(np.abs(np.asarray(x, np.float64) - x64).max() / np.abs(x64).max())


def step_arrays(params0, new_p, new_s0, new_s1):
    """{array: [per block float64]} of one step's results (s1: absent on a one-slot rule)."""
    out = {"dtheta": [np.asarray(q, np.float64) - np.asarray(p, np.float64) for p, q in zip(params0, new_p)],
           "s0": [np.asarray(s, np.float64) for s in new_s0]}
    if new_s1[0] is not None:
        out["s1"] = [np.asarray(s, np.float64) for s in new_s1]
    return out


def errors(got, ref, names):
    """{array: {block: error}} of two step_arrays results."""
    return {k: {n: rel_err(x, r) for n, x, r in zip(names, got[k], ref[k])} for k in ref}


def over(err, bound):
    """{(array, block): (error, bound)} past the bound: the criterion of the GPU tests."""
    return {(k, n): (err[k][n], bound[k][n]) for k in bound for n in bound[k] if not err[k][n] <= bound[k][n]}


def unflatten(flat, shapes):
    out, o = [], 0
    for _, s in shapes:
        k = int(np.prod(s))
        out.append(np.asarray(flat[o:o + k]).reshape(s))
        o += k
    assert o == len(flat)
    return out


@functools.lru_cache(maxsize=None)
def grads32(name, latent, scaled):
    """The float32 gradient of a table case: the float32-fed oracle."""
    st = G.case(name, latent, scaled)
    out = G.forward_backward(st.cfg, latent, st.params, st.Xtr[st.idx].astype(np.float32),
                             None if st.eps is None else st.eps.astype(np.float32))
    assert out["grads"][0].dtype == np.float32
    return out["grads"]


@dataclasses.dataclass
class RuleStep:
    """One rule step of a table case: inputs, the float64 oracle's arrays and the bounds."""
    st: object
    h: O.Hyper
    t0: int                  # optimiser steps taken before this one
    S0: list
    S1: list
    names: list
    ref: dict                # {array: [per block float64]}
    restate: dict            # {array: {block: error of the float32 restatement}}
    bound: dict              # MARGIN x restate

    def device(self, theta1, s0_1, s1_1=None):
        """{array: {block: error}} of the device's flat theta', slot 0' (and slot 1')."""
        sh = self.st.shapes
        got = step_arrays(self.st.params, unflatten(theta1, sh), unflatten(s0_1, sh),
                          unflatten(s1_1, sh) if s1_1 is not None else [None] * len(sh))
        return errors(got, self.ref, self.names)

    def flat(self, S):
        return A.flatten(S)


def run_both(params, S0, S1, g64, g32, h, t, fn=None):
    """(float64 arrays, float32-restated arrays) of one step at step number t."""
    p64, s064, s164 = (O.as_dtype(x, np.float64) for x in (params, S0, S1))
    ref = step_arrays(params, *O.apply(p64, s064, s164, g64, h, t, fn))
    low = step_arrays(params, *O.apply(params, S0, S1, g32, h, t, fn))
    return ref, low


@functools.lru_cache(maxsize=None)
def rule_step(name, latent, scaled, key, zero=False):
    """The RuleStep of a table case under HYPERS[key]: from the conditioned state at t0 = T0, or
    (zero) from zero state at t0 = 0."""
    st = G.case(name, latent, scaled)
    h = HYPERS[key]
    names = [n for n, _ in st.shapes]
    g64 = [st.g64[n] for n in names]
    t0 = 0 if zero else T0
    for seed in range(1 if zero else MAX_STATE_SEEDS):
        S0, S1 = zero_state(h.rule, st.params) if zero else conditioned(h.rule, g64, seed)
        ref, low = run_both(st.params, S0, S1, g64, grads32(name, latent, scaled), h, t0 + 1)
        restate = errors(low, ref, names)
        bound = {k: {n: G.MARGIN * e for n, e in v.items()} for k, v in restate.items()}
        if zero or (caps_hold(bound) and no_cancellation(h, g64, ref["s0"]) and no_accident(h, g64, grads32(name, latent, scaled), ref["s0"], restate, names)):
            return RuleStep(st, h, t0, S0, S1, names, ref, restate, bound)
    raise AssertionError(f"{name}-{latent}-{scaled}-{key}: no conditioned state below seed {MAX_STATE_SEEDS} meets the conditions")


# The conditioned state of a case is the first seed that meets three conditions on the inputs (the rule
# of ae_grad_cases.case's fair seeds), both judged on the float64 oracle and the restatement alone:
#  * the bounds meet the caps;
#  * in no block does the drawn first moment or velocity cancel the gradient's share of the new one:
#    max|s0'| >= c max|g| per block, c = 1 (sga) or 1 - beta1 (adam).  s0' = beta s0 + c g, and the
#    step is proportional to it, so where beta s0 all but cancels c g the gradient's own float32 error
#    (tests/ae_grad_cases.py bounds it per block relative to max|g|) is magnified by c max|g| / max|s0'|
#    in s0' and in dtheta, and the test would measure that cancellation, not the rule.  It matters in
#    the blocks of one element (bzmu, bzlv at Dz = 1), where it is a coin toss on the sign of the draw;
#    the first device run showed it there (sga, bzlv of edge_bin_tanh-gauss-theta0: dtheta 7.8e-6
#    against a bound of 7.1e-6, the gradient itself being 4.9e-6 off at that element,
#    tests/test_gpu_ae_grads.py) and the condition was written down then.  AdaDelta has no such term.
#  * in a block of ONE element (bz, bzmu, bzlv at Dz = 1) the restated s0' and dtheta of sga and adam are
#    no nearer to the oracle than the restatement's own gradient error puts them:
#    restate_X >= share x restate_g, share = c |g| / |s0'| (<= 1 by the condition above), restate_g the
#    error of the float32 gradient at that element.  The restatement is one sample of float32 rounding;
#    over a block of many elements its maximum is stable, but with one element the rule's own roundings
#    can cancel the gradient's error by accident (the second device run: s0' of bzlv restated to
#    2.7e-11, i.e. a bound of 4e-10 on a float32 value whose gradient is 4e-8 off in the restatement
#    itself), and 16 x an accident is no bound for another float32 gradient.
# The zero-state steps have no draw to choose; first_step_cases leaves the cases with a one-element
# block out instead.
MAX_STATE_SEEDS = 64


def no_accident(h, g64, g32, s0_new, restate, names):
    c = {"sga": 1.0, "adam": 1.0 - h.beta1}.get(h.rule)
    for n, g, q, s in zip(names, g64, g32, s0_new):
        if c is not None and g.size == 1:
            floor = c * np.abs(g).max() / np.abs(s).max() * rel_err(q, g)
            if restate["s0"][n] < floor or restate["dtheta"][n] < floor:
                return False
    return True


def no_cancellation(h, g64, s0_new):
    c = {"sga": 1.0, "adam": 1.0 - h.beta1}.get(h.rule)
    return c is None or all(np.abs(s).max() >= c * np.abs(g).max() for s, g in zip(s0_new, g64))


def caps_hold(bound, arrays=ARRAYS):
    """The conditions on the inputs: state bounds <= STATE_CAP, dtheta bounds <= DTHETA_CAP."""
    return all(b <= (DTHETA_CAP if k == "dtheta" else STATE_CAP)
               for k, v in bound.items() if k in arrays for b in v.values())


# The first step from zero state checks the slots alone (the step itself by size and sign).  There a
# second-moment slot is (1 - beta) g^2 and carries twice the gradient's relative error, which in
# the two batch_51x-point-theta0 cases (gradient bounds of 8e-5, the largest of the table) puts its
# bound past STATE_CAP; the first-step tests run on the cases whose slot bounds meet the cap.
def first_step_case(name, latent, scaled):
    if any(int(np.prod(shp)) == 1 for _, shp in G.case(name, latent, scaled).shapes):
        return False   # one-sample restatement of a one-element block: see the conditions above
    return all(caps_hold(rule_step(name, latent, scaled, key, True).bound, ("s0", "s1") if key == "adam" else ("s0",))
               for key in ("adadelta", "adam"))


def first_step_cases():
    sel = [(c, i) for c, i in zip(G.CASES, G.CASE_IDS) if first_step_case(*c)]
    return [c for c, _ in sel], [i for _, i in sel]


def worst(err, bound, restate):
    """'array/block device / restatement / bound' of the entry nearest to its bound."""
    k, n = max(((k, n) for k in bound for n in bound[k]),
               key=lambda kn: err[kn[0]][kn[1]] / bound[kn[0]][kn[1]] if bound[kn[0]][kn[1]] > 0 else np.inf)
    return f"{k}/{n} {err[k][n]:.1e} / {restate[k][n]:.1e} / {bound[k][n]:.1e}"


# ------------------------------------------------------------------ trajectories
@dataclasses.dataclass(frozen=True)
class Model:
    name: str
    kw: tuple
    latent: str              # the oracle's latent
    B: int
    K: int = 1               # iw_samples

    def cfg(self):
        return A.AEConfig(**dict(self.kw))


def _model(name, latent, B, K=1, **kw):
    return Model(name, tuple(sorted(kw.items())), latent, B, K)


STEPS = 4
MODELS = [
    _model("point", "point", 17, Dobs=37, Denc=(17, 33), Dz=3, Ddec=(15, 31), otype="binary", act="tanh", s2=2.0),
    _model("gauss_elbo", "gauss", 15, Dobs=37, Denc=(32,), Dz=17, Ddec=(16,), otype="cont", act="sigmoid"),
    _model("gauss_iw3", "gauss", 17, K=3, Dobs=24, Denc=(20,), Dz=4, Ddec=(18,), otype="binary", act="tanh"),
    _model("vanilla_se", "act", 17, Dobs=33, Denc=(31,), Dz=5, Ddec=(17,), otype="se", act="tanh"),
]
MODEL = {m.name: m for m in MODELS}


@dataclasses.dataclass
class Trajectory:
    model: Model
    cfg: A.AEConfig
    h: O.Hyper
    params: list
    shapes: list
    names: list
    Xtr: np.ndarray
    idx: np.ndarray          # the train_many list: STEPS batches, the last one partial
    eps: object              # None, [n x Dz] or [K x n x Dz] float32
    S0: list
    S1: list
    values64: list
    ref: dict
    restate: dict
    bound: dict

    def host_eps(self):
        """eps as vaeb_ae_push_eps takes it: sample k of list position i at row k n + i."""
        return None if self.eps is None else self.eps.reshape(-1, self.cfg.Dz)

    def device(self, theta1, s0_1, s1_1=None):
        got = step_arrays(self.params, unflatten(theta1, self.shapes), unflatten(s0_1, self.shapes),
                          unflatten(s1_1, self.shapes) if s1_1 is not None else [None] * len(self.shapes))
        return errors(got, self.ref, self.names)


@functools.lru_cache(maxsize=None)
def trajectory(model_name, key):
    """STEPS steps of train_many (batch B not dividing n, host eps) under HYPERS[key] from the
    conditioned state at T0, on theta_0 x 30 (ae_grad_cases.scale_params)."""
    m = MODEL[model_name]
    cfg, h = m.cfg(), HYPERS[key]
    lat_layout = "gauss" if m.latent == "gauss" else "point"
    shapes = A.param_shapes(cfg, m.latent)
    names = [n for n, _ in shapes]
    params = G.scale_params(cfg, A.init_params(cfg, seed=15485863 + 11, latent=m.latent), lat_layout)
    n = (STEPS - 1) * m.B + 5
    Xtr = G.data_for(cfg, n + 9, 3)
    rng = np.random.default_rng(77)
    idx = rng.choice(Xtr.shape[0], size=n, replace=False).astype(np.int32)
    batches = [idx[lb:lb + m.B] for lb in range(0, n, m.B)]
    assert len(batches) == STEPS and len(batches[-1]) == 5
    eps = None
    if m.latent == "gauss":
        eps = rng.standard_normal((m.K, n, cfg.Dz) if m.K > 1 else (n, cfg.Dz)).astype(np.float32)
    kw = dict(latent=m.latent)
    p64 = [p.astype(np.float64) for p in params]
    e0 = None if eps is None else eps[..., :m.B, :].astype(np.float64)
    first = A.forward_backward(p64, Xtr[batches[0]].astype(np.float64), cfg, **kw, **({} if e0 is None else {"eps": e0}))
    for seed in range(MAX_STATE_SEEDS):   # rule_step's two conditions, the second at the first step
        S0, S1 = conditioned(h.rule, first["grads"], seed)
        one = O.apply(p64, O.as_dtype(S0, np.float64), O.as_dtype(S1, np.float64), first["grads"], h, T0 + 1)
        if not no_cancellation(h, first["grads"], one[1]):
            continue
        v64, p, s0, s1 = O.trajectory(cfg, params, S0, S1, Xtr, batches, h, T0, np.float64, eps=eps, **kw)
        _, q, r0, r1 = O.trajectory(cfg, params, S0, S1, Xtr, batches, h, T0, np.float32, eps=eps, **kw)
        assert q[0].dtype == np.float32 and r0[0].dtype == np.float32
        ref, low = step_arrays(params, p, s0, s1), step_arrays(params, q, r0, r1)
        restate = errors(low, ref, names)
        bound = {k: {b: G.MARGIN * e for b, e in v.items()} for k, v in restate.items()}
        if caps_hold(bound):
            return Trajectory(m, cfg, h, params, shapes, names, Xtr, idx, eps, S0, S1, v64, ref, restate, bound)
    raise AssertionError(f"{model_name}-{key}: no conditioned state below seed {MAX_STATE_SEEDS} meets the conditions")
