"""Per-element parity of the fp32 step engine (vaeb_amd/csrc/engine_f32.inc, latent.hpp,
latent_bwd.hpp, fused.hpp, phases.hpp, kernels_aux.hpp) away from theta_0 -- TEST HELPER ONLY: the
case table, the two states, the float64 oracle step, its float32 restatement, the bounds and
fair(), shared by tests/test_f32_parity_host.py (no GPU) and tests/test_gpu_f32_parity.py.

Why.  Every other oracle comparison of this engine's training step starts from init_params
(W ~ N(0, 0.01)).  There no hidden unit leaves |h| < 0.3, lv stays within +-0.1, every decoder mean
within 0.05 of 1/2 and the Gaussian head at a6 ~ 0: tanh is linear, 1 - h^2 ~ 1, exp(lv) ~ 1,
sigmoid ~ 1/2, exp(-a6) ~ 1, and the gradients are compared norm-wise per tensor.

States.
  x30      theta_0 (biases 0.01 N(0, 1), as tests/test_gpu_step.py::test_single_step_parity) with
           every layer's W and b times 30 min(1, sqrt(64 / Kin)), Kin the width of the layer's
           input (the rule of tests/ae_grad_cases.py scale_params); Adagrad accumulator 1e-3
           everywhere (as the 16-bit single-step tests).
  startup  theta and the accumulators after STARTUP_STEPS float64 oracle steps from theta_0 with
           zero accumulators on fixed minibatches and noise, cast to float32: the state in which
           tests/test_gpu_h16_traj.py found a silent NaN in the 16-bit engines.
The step under test then runs minibatch IDX = 2 with host eps; data, theta_0's biases and eps are
drawn as test_single_step_parity draws them, from default_rng(seed).  The seed of a case is the
first of SEED0, SEED0 + 1, ... (MAX_SEEDS tries) that is fair (fair()).

Criterion.  For a quantity Q:  err(Q) = max|Q - Q64| / max|Q64|, Q64 the float64 oracle's value
(oracle/vaeb_oracle.py).  Bound = MARGIN x max(err of the float32 restatement, 2^-23): the
restatement is the same oracle functions fed float32 arrays (forward_backward follows the dtype of
W3), 16 x is the margin of tests/test_gpu_eval_path.py and tests/ae_grad_cases.py, 2^-23 is
float32's spacing.  No bound comes from the device.  Q runs over each data-gradient block
(vaeb_get_grads, reference order), the activations h, mu, lv, z, hd over all L planes (valid rows)
and the stored backward operands dA2, dA6, dA1, [dMu | dLv], dA3.  (The decoder means y are not
stored by a training launch -- phases.hpp PDecOut::epilogue_row stores dA2 (| dA6) in MODE_TRAIN
and y only in MODE_RECON -- so the step sees them through dA2; tests/test_gpu_f32_parity.py
compares y itself on the evaluation path.)

Optimizer.  theta' is not compared with the oracle's theta': an Adagrad step divides by sqrt(acc),
so a gradient error of 1e-6 max|g| is percent-level in the step wherever |g| <~ sqrt(acc).
Instead adagrad_update runs in float64 on (theta, acc, g_dev - prior theta), g_dev the gradient the
device reports, and theta'_dev - theta, acc'_dev - acc are compared with it per parameter block in
units of the block's max|.|; the bound is MARGIN x max(error of the float32 adagrad_update on the
same inputs, 2^-23).
"""
import dataclasses
import functools
import math

import numpy as np

from oracle import vaeb_oracle as O

MARGIN = 16.0              # device bound = MARGIN x max(restatement error, ULP)
ULP = 2.0 ** -23           # float32's spacing
GRAD_CAP = 1e-4            # a condition on the inputs: every gradient bound <= today's tolerance
VALUE_RTOL = 1e-4          # the step's value: tests/test_gpu_step.py
SCALE = 30.0
WIDE = 64                  # a layer with more inputs than this gets SCALE sqrt(WIDE / Kin)
ACC0 = 1e-3                # the x30 state's accumulator
IDX = 2                    # the minibatch of the step under test
SEED0 = 3
MAX_SEEDS = 64
STARTUP_STEPS = 5
STARTUP_ORDER = (0, 1, 3, 0, 1)     # minibatches of the start-up steps (IDX is not among them)
STARTUP_EPS_SEED = 11

SHAPES = {
    # name: (config, B): each from an existing table, where the kernels it selects are documented
    "mnist20": (dict(D=784, H=500, Z=20), 100),                                    # slab encoder, deferred dW2, decout_z2
    "frey2_gauss": (dict(D=560, H=200, Z=2, continuous=True), 100),                # counted atomics both ways, Gaussian
    "odd_shapes": (dict(D=37, H=19, Z=3), 13),                                     # scalar loads, partial tiles everywhere
    "atomic_LA_L2": (dict(D=40, H=72, Z=20, estimator="LA", L=2), 20),             # LA, second z plane, idle epilogue waves
    "gauss_latent28_slab_odd_H": (dict(D=45, H=274, Z=28, continuous=True), 20),   # slab, NCT = 2, H % 4 != 0
    "mean_map_frey10": (dict(D=560, H=200, Z=10, continuous=True, objective="mean_map"), 100),   # sc = 1/B, decay
    "bern_latent18_odd_H_deep": (dict(D=530, H=30, Z=18), 17),                     # dhd K > 512 with scalar loads
    "wide_latent_generic": (dict(D=64, H=40, Z=40, L=2), 20),                      # Z > 32: the generic phases
    "L6_LA_deferred": (dict(D=200, H=96, Z=28, estimator="LA", L=6), 50),          # l >= 4 re-reads, deferred reducer
    "H1040_gauss_L5": (dict(D=36, H=1040, Z=20, continuous=True, L=5), 19),        # ticket encoder, GCH = 8
    "slab_partial_k": (dict(D=33, H=500, Z=20), 100),                              # partial last K block, column tile past D
    "gauss_cap": (dict(D=24, H=40, Z=2, continuous=True), 17),                     # the 128-VGPR form
    "mnist_LA_L2": (dict(D=784, H=500, Z=20, estimator="LA", L=2), 100),           # start-up state only
}
X30 = [n for n in SHAPES if n != "mnist_LA_L2"]
STARTUP = ["mnist20", "frey2_gauss", "mean_map_frey10", "bern_latent18_odd_H_deep", "mnist_LA_L2"]
CASES = [(n, "x30") for n in X30] + [(n, "startup") for n in STARTUP]
CASE_IDS = [f"{n}-{s}" for n, s in CASES]

ACTS = ("h", "mu", "lv", "z", "hd")                       # forward order
BWD = ("dA2", "dA6", "dA1", "dMuLv", "dA3")               # backward order


def config(name):
    return O.Config(**SHAPES[name][0])


def batch(name):
    return SHAPES[name][1]


def r16(n):
    return (n + 15) // 16 * 16


def data_for(cfg, n, seed=0):
    """tests/test_gpu_step.py data_for."""
    if cfg.continuous:
        return O.synthetic_frey(n=n, D=cfg.D, seed=seed)
    return O.synthetic_mnist(n=n, D=cfg.D, seed=seed)


def layer_inputs(cfg):
    """{parameter name: width of its layer's input}."""
    kin = {"W3": cfg.D, "W4": cfg.H, "W5": cfg.H, "W1": cfg.Z, "W2": cfg.H, "W6": cfg.H}
    kin.update({"b" + n[1:]: k for n, k in list(kin.items())})
    return {n: kin[n] for n in cfg.names}


def scale_params(cfg, params):
    """Every layer x 30, a layer wider than WIDE at its input x 30 sqrt(WIDE / Kin)."""
    kin = layer_inputs(cfg)
    return [(p * (SCALE * min(1.0, math.sqrt(WIDE / kin[n])))).astype(np.float32) for n, p in zip(cfg.names, params)]


def theta0(cfg, B, seed):
    """(params, eps) as test_single_step_parity draws them: init_params, biases 0.01 N(0, 1), then eps."""
    rng = np.random.default_rng(seed)
    params = [p if p.ndim == 2 else (0.01 * rng.standard_normal(p.shape)).astype(np.float32)
              for p in O.init_params(cfg)]
    eps = rng.standard_normal((cfg.L, B, cfg.Z)).astype(np.float32)
    return params, eps


def f64(arrs):
    return [np.asarray(a, np.float64) for a in arrs]


def prior_coef(cfg):
    return 1.0 if cfg.objective == "sum_prior" else 0.0


@functools.lru_cache(maxsize=None)
def startup_state(name, seed):
    """(theta, acc) float32 after STARTUP_STEPS float64 oracle steps from theta_0 and zero accumulators."""
    cfg, B = config(name), batch(name)
    x = data_for(cfg, 4 * B)
    params, _ = theta0(cfg, B, seed)
    rng = np.random.default_rng(STARTUP_EPS_SEED)
    p, a = f64(params), [np.zeros(q.shape) for q in params]
    for b in STARTUP_ORDER[:STARTUP_STEPS]:
        eps = rng.standard_normal((cfg.L, B, cfg.Z)).astype(np.float32)
        _, p, a, _ = O.step(p, a, x[b * B:(b + 1) * B].astype(np.float64), eps.astype(np.float64), cfg)
    return [q.astype(np.float32) for q in p], [q.astype(np.float32) for q in a]


def draw(name, state, seed):
    """x, params, acc, eps of one seed in one state ("theta0" too: what today's tests cover)."""
    cfg, B = config(name), batch(name)
    x = data_for(cfg, 4 * B)
    params, eps = theta0(cfg, B, seed)
    if state == "x30":
        params = scale_params(cfg, params)
        acc = [np.full_like(p, ACC0) for p in params]
    elif state == "startup":
        params, acc = startup_state(name, seed)
    else:
        assert state == "theta0"
        acc = [np.zeros_like(p) for p in params]
    return x, params, acc, eps


# ------------------------------------------------------------------ quantities and the criterion
def quantities(cfg, out, B):
    """{name: array} of one oracle forward / backward, in the order a failure is read: forward
    activations, backward operands, then the data-gradient blocks in reference order."""
    L, H, D = cfg.L, cfg.H, cfg.D
    q = {"h": out["h"], "mu": out["mu"], "lv": out["lv"], "z": out["z"], "hd": out["hd"].reshape(L, B, H),
         "y": out["y"].reshape(L, B, D), "dA2": out["dA2"].reshape(L, B, D)}
    if cfg.continuous:
        q["dA6"] = out["dA6"].reshape(L, B, D)
    q["dA1"] = out["dA1"].reshape(L, B, H)
    q["dMuLv"] = np.concatenate([out["dMu"], out["dLv"]], axis=1)
    q["dA3"] = out["dA3"]
    for n, g in zip(cfg.names, out["data_grads"]):
        q["g" + n] = g
    return q


def grad_keys(cfg):
    return ["g" + n for n in cfg.names]


def err(a, a64):
    """max|a - a64| / max|a64|."""
    a64 = np.asarray(a64, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - a64).max() / np.abs(a64).max())


def errors(got, q64):
    """{name: err} over the quantities of `got` (shapes as quantities())."""
    for k in got:
        assert np.shape(got[k]) == q64[k].shape, (k, np.shape(got[k]), q64[k].shape)
    return {k: err(got[k], q64[k]) for k in got}


def bound_of(restate):
    return {k: MARGIN * max(e, ULP) for k, e in restate.items()}


def rejected(e, bound):
    """Quantities of e above their bound (NaN included), in the order of e."""
    return [k for k in e if not e[k] <= bound[k]]


def stats(cfg, out):
    """Where the float64 forward sits: the figures of fair()."""
    s = {"h_sat": float((np.abs(out["h"]) > 0.9).mean()), "hd_sat": float((np.abs(out["hd"]) > 0.9).mean()),
         "hd_open": float((np.abs(out["hd"]) < 0.99).mean()), "h_max": float(np.abs(out["h"]).max()),
         "lv_max": float(np.abs(out["lv"]).max()), "y_min": float(out["y"].min()), "y_max": float(out["y"].max()),
         "y_off": float(np.abs(out["y"] - 0.5).max())}
    if cfg.continuous:
        s.update(a6_min=float(out["a6"].min()), a6_max=float(out["a6"].max()))
    return s


def fair_reasons(cfg, state, s):
    """The conditions of a state that the figures s miss (empty: fair)."""
    bad = []
    if state == "x30":
        if not (s["h_sat"] >= 0.05 and s["hd_sat"] >= 0.05):
            bad.append("saturated share of h / hd below 0.05")
        if not s["hd_open"] >= 0.4:
            bad.append("share of |hd| < 0.99 below 0.4")
        if not 1.0 <= s["lv_max"] <= 8.0:
            bad.append("max|lv| outside [1, 8]")
        if not (s["y_min"] < 0.2 and s["y_max"] > 0.8):
            bad.append("no y below 0.2 or none above 0.8")
        if cfg.continuous and not (s["a6_min"] < -1.0 and s["a6_max"] > 1.0 and max(-s["a6_min"], s["a6_max"]) <= 12.0):
            bad.append("a6 not on both sides of +-1 within +-12")
    elif state == "startup":
        if not (s["h_sat"] >= 0.1 or s["lv_max"] >= 1.0):
            bad.append("neither 10 % of |h| > 0.9 nor max|lv| >= 1")
    return bad


@dataclasses.dataclass
class Step:
    """One step's inputs, its float64 oracle and the float32 restatement's errors."""
    name: str
    state: str
    seed: int
    cfg: O.Config
    B: int
    x: np.ndarray               # the whole data set (4 B rows); the step runs rows [idx B, (idx + 1) B)
    idx: int
    eps: np.ndarray             # [L, B, Z] float32
    params: list                # float32
    acc: list                   # float32
    out64: dict
    value64: float              # SGVB / B
    q64: dict                   # quantities() of the float64 oracle
    restate: dict               # {quantity: err of the float32 restatement}
    bound: dict
    restate_value: float
    stats: dict

    def theta(self):
        return O.flatten(self.params)

    def acc_flat(self):
        return O.flatten(self.acc)


def make_step(name, state, cfg, B, x, idx, params, acc, eps, seed=0):
    """Oracle, restatement and bounds of one step on rows [idx B, (idx + 1) B) of x.  eps may be
    float64 (the Philox oracle's draw); the restatement and the device take it rounded to float32."""
    xb = x[idx * B:(idx + 1) * B]
    out64 = O.forward_backward(f64(params), xb.astype(np.float64), np.asarray(eps, np.float64), cfg)
    q64 = quantities(cfg, out64, B)
    assert all(p.dtype == np.float32 for p in params)
    out32 = O.forward_backward(params, xb.astype(np.float32), np.asarray(eps, np.float32), cfg)
    assert out32["data_grads"][0].dtype == np.float32 and out32["hd"].dtype == np.float32
    restate = errors(quantities(cfg, out32, B), q64)
    v64 = float(out64["sgvb"]) / B
    step = Step(name, state, seed, cfg, B, x, idx, np.asarray(eps), params, acc, out64, v64, q64, restate,
                bound_of(restate), abs(float(out32["sgvb"]) / B - v64) / abs(v64), stats(cfg, out64))
    for a in [x, step.eps] + list(params) + list(acc) + list(q64.values()):
        a.setflags(write=False)
    return step


def fair(name, state, seed):
    """The reasons seed `seed` is not fair for (name, state); empty when it is."""
    cfg, B = config(name), batch(name)
    x, params, _, eps = draw(name, state, seed)
    out = O.forward_backward(f64(params), x[IDX * B:(IDX + 1) * B].astype(np.float64), eps.astype(np.float64), cfg,
                             need_grad=False)
    return fair_reasons(cfg, state, stats(cfg, out))


@functools.lru_cache(maxsize=None)
def case(name, state):
    """The Step of one table case at its first fair seed."""
    for seed in range(SEED0, SEED0 + MAX_SEEDS):
        if not fair(name, state, seed):
            x, params, acc, eps = draw(name, state, seed)
            return make_step(name, state, config(name), batch(name), x, IDX, params, acc, eps, seed)
    raise AssertionError(f"{name}-{state}: no fair seed in {MAX_SEEDS} tries")


# ------------------------------------------------------------------ the optimizer
def adagrad_deltas(cfg, theta, acc, g, dtype):
    """(theta' - theta, acc' - acc) of oracle.adagrad_update in `dtype` on flat arrays; g is the
    data gradient, the prior's -theta (objective sum_prior) is added here in the same dtype."""
    th, a = np.asarray(theta, dtype), np.asarray(acc, dtype)
    gt = np.asarray(g, dtype) - dtype(prior_coef(cfg)) * th
    (p1,), (a1,) = O.adagrad_update([th], [a], [gt], cfg)
    assert p1.dtype == dtype and a1.dtype == dtype
    return p1.astype(np.float64) - th.astype(np.float64), a1.astype(np.float64) - a.astype(np.float64)


def block_errors(cfg, flat, flat64, tag):
    """{tag + block: max|flat - flat64| / max|flat64|} per parameter block."""
    out, o = {}, 0
    for n, s in O.param_shapes(cfg):
        k = int(np.prod(s))
        out[tag + n] = err(flat[o:o + k], flat64[o:o + k])
        o += k
    assert o == len(flat64)
    return out


def optimizer_check(cfg, theta, acc, g_dev, theta1, acc1):
    """(err, restate, bound) of an update (theta1, acc1) claimed for the float32 inputs theta, acc
    and the reported data gradient g_dev (all flat), per block: "dth.W3", ..., "dac.W3", ..."""
    theta, acc, g_dev = (np.asarray(a, np.float32) for a in (theta, acc, g_dev))
    dth64, dac64 = adagrad_deltas(cfg, theta, acc, g_dev, np.float64)
    dth32, dac32 = adagrad_deltas(cfg, theta, acc, g_dev, np.float32)
    restate = {**block_errors(cfg, dth32, dth64, "dth."), **block_errors(cfg, dac32, dac64, "dac.")}
    got_th = np.asarray(theta1, np.float64) - theta.astype(np.float64)
    got_ac = np.asarray(acc1, np.float64) - acc.astype(np.float64)
    e = {**block_errors(cfg, got_th, dth64, "dth."), **block_errors(cfg, got_ac, dac64, "dac.")}
    return e, restate, bound_of(restate)


# ------------------------------------------------------------------ reading a device step
def read_step(ctx, cfg, B):
    """{quantity: array} of the step a context has just taken (keep_grads), valid rows only, in
    quantities()' shapes, and the padding rows of z and hd.  Device layouts: h [Mp][H]; mu, lv
    [Mp][Z]; z, hd, dA2, dA6, dA1 [L][Mp][.]; dMuLv [Mp][2 Z] = [dMu | dLv]; dA3 [Mp][H]
    (Mp = B rounded up to 16)."""
    L, D, H, Z, Mp = cfg.L, cfg.D, cfg.H, cfg.Z, r16(B)
    rows = {k: ctx.activation(k, Mp * w).reshape(Mp, w) for k, w in (("h", H), ("mu", Z), ("lv", Z))}
    planes = {k: ctx.activation(k, L * Mp * w).reshape(L, Mp, w) for k, w in (("z", Z), ("hd", H))}
    got = {k: v[:B] for k, v in rows.items()}
    got.update({k: v[:, :B] for k, v in planes.items()})
    pad = {k: v[:, B:] for k, v in planes.items()}
    for k, w in (("dA2", D), ("dA6", D), ("dA1", H)):
        if k != "dA6" or cfg.continuous:
            got[k] = ctx.activation(k, L * Mp * w).reshape(L, Mp, w)[:, :B]
    got["dMuLv"] = ctx.activation("dMuLv", Mp * 2 * Z).reshape(Mp, 2 * Z)[:B]
    got["dA3"] = ctx.activation("dA3", Mp * H).reshape(Mp, H)[:B]
    g = ctx.get_grads()
    for (n, s), gg in zip(O.param_shapes(cfg), O.unflatten(g, cfg)):
        got["g" + n] = gg.reshape(s)
    return got, pad, g


def judge(step, value, got, pad, g_dev, theta1, acc1):
    """(table line, failures) of one device step under every criterion of this module."""
    cfg = step.cfg
    e = errors(got, step.q64)
    bad = rejected(e, step.bound)
    oe, orst, obound = optimizer_check(cfg, step.theta(), step.acc_flat(), g_dev, theta1, acc1)
    bad += rejected(oe, obound)
    for k, v in pad.items():
        if v.size and not np.all(v == 0.0):
            bad.append(f"pad rows of {k}")
    vrel = abs(value - step.value64) / abs(step.value64)
    if not vrel <= VALUE_RTOL:
        bad.append("value")
    label = f"{step.name}-{step.state}"
    return (table_line(label, e, step.restate, step.bound) + "  |  " + table_line("", oe, orst, obound).strip()
            + f"  |  value {vrel:.1e}"), bad


def table_line(label, e, restate, bound):
    """'label  worst quantity  device / restatement / bound': the quantity nearest to (or furthest
    past) its bound."""
    n = max(e, key=lambda k: (e[k] / bound[k]) if e[k] == e[k] else math.inf)
    return f"{label:34s} {n:7s} {e[n]:.1e} / {restate[n]:.1e} / {bound[n]:.1e}"
