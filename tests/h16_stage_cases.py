"""The 16-bit step engine (vaeb_amd/csrc/engine_bf16.inc, step_bf16.hpp, gemm_bf16.hpp,
thin_bf16.hpp, h16_gemm_hooks.inc; bf16 and fp16 operands) per stage, from its own stored operands,
away from theta_0 -- TEST HELPER ONLY: the case table, the two states, the per-stage functions, the
criterion and the float32 stand-in for the device, shared by tests/test_h16_stage_host.py (no GPU)
and tests/test_gpu_h16_stage.py.

Why.  tests/test_gpu_bf16.py / test_gpu_fp16.py compare the step from init_params only
(W ~ N(0, 0.01): tanh linear, exp(lv) ~ 1, y ~ 1/2, a6 ~ 0), its data gradients norm-wise per tensor
(2e-3) and no stored operand at all.  One tile-corner element of dA2 wrong by its whole value moves
gW2 by ~1e-4 .. 1e-3 norm-wise.  A per-element gradient criterion cannot close that: whether a value
near a 16-bit rounding tie rounds the other way upstream moves a gradient element by 3e-8 .. 1e-3
of the block maximum.  So every stage is recomputed from the inputs the kernel itself read, as read
back from the device (vaeb_get_h16, include/vaeb_diag.h): an upstream flip then cannot reach the
comparison (teacher forcing, as tests/test_gpu_h16_traj.py does per step).

States.
  x30     f32_parity_cases.scale_params on theta_0 as test_bf16_step_parity draws it (init_params,
          biases 0.01 N(0, 1), then eps, from default_rng(seed); data_for(cfg, 3 B), minibatch 1),
          Adagrad accumulators 1e-3.  Z >= 128 (W1_DAMP): W1 and b1 get a further factor
          sqrt(64 / Z) -- z has Z terms of size ~|mu| + sd, not ~1, so scale_params' sqrt(64 / Kin)
          leaves |a1| ~ 30 and every hd saturated (share of |hd| < 0.99 below 0.4 at seeds 3, 4);
          decided on the host oracle, the figures are printed by tests/test_h16_stage_host.py.
  theta0  today's state, on three shapes: a failure there is no scaling effect.
The seed of a case is the first of SEED0, SEED0 + 1, ... that is fair: the x30 conditions of
f32_parity_cases.fair_reasons, and every 16-bit store of the float64 fp16-rounded oracle (the
backward's times the loss scale) inside fp16's range.  Both dtypes of a case share the seed.

Stages (stage_values; each from the device's own stored inputs, in float64):
  h      tanh(X W3 + b3)                         X the 16-bit data set, W the shadow before the step
  mulv   h_dev [W4 | W5] + [b4 | b5]             fp32 (criterion "gemm")
  z      mu_dev + exp(lv_dev / 2) eps            all L planes
  hd     tanh(z_dev W1 + b1)
  dA2 (, dA6)  the likelihood epilogue of hd_dev [W2 | W6] + b against x, times sl S
  dA1    (dA_dev [W2 | W6]^T) (1 - hd_dev^2)
  dml    [dMu | dLv] from dZ = dA1_dev W1^T, mu_dev, lv_dev, eps (LB and LA, over L), the latent
         terms times sc S
  dA3    (dml_dev [W4 | W5]^T) (1 - h_dev^2)
  gW*    each weight gradient = the product of its two stored operands / S (criterion "gemm")
  gb*    each bias gradient = the column sum of its stored operand / S (criterion "bias")
S is the fp16 loss scale of the mean objective (engine_bf16.inc h16_scale), 1 otherwise.

Criterion.  No bound comes from the device.
  16-bit stored element v against its float64 pre-rounding value t:
      |v - t| <= ulp16(t) / 2 + tau,   tau = MARGIN max(max|t32 - t64|, 2^-23 max|t64|) over the stage,
      t32 the same stage function fed float32 arrays, ulp16 the dtype's spacing at t (fp16: gradual
      underflow below 2^-14, as O.fp16_round).  v may differ from Q(t) only where t is within tau
      of a rounding tie, and then by one ulp.
  gemm   |C - ref| <= 1e-5 (|A| |B|) (+ 2^-23 |ref| where a bias is added): tests/test_gpu_bf16.py
         test_gemm_layouts' own bound.
  bias   the kernels sum the unrounded fp32 values, the test sees the rounded ones:
         sum_rows ulp16(stored) / 2 + 2^-23 sum_rows |stored| per column.
  value  1e-4 against the rounded float64 oracle; theta' - theta and acc' - acc per block with
         f32_parity_cases.optimizer_check on the gradient the device reports; the shadow is Q(theta)
         before and Q(theta') after the step, bit for bit.
RAISED holds a stage's tau raised to MARGIN x the error of a float32 NumPy restatement of the kernel's
own arithmetic, with that restatement beside it: the two tanh stages at theta_0 (ftanh_bf), nothing at x30.
"""
import dataclasses
import functools
import math

import numpy as np

from oracle import vaeb_oracle as O
from tests import f32_parity_cases as F

MARGIN = F.MARGIN
ULP32 = 2.0 ** -23
GEMM_TOL = 1e-5            # tests/test_gpu_bf16.py test_gemm_layouts
VALUE_RTOL = 1e-4
TODAY_GRAD = 2e-3          # today's norm-wise tolerance per gradient block
ACC0 = 1e-3
IDX = 1
NB = 3
SEED0 = 5                  # test_bf16_step_parity's seed
MAX_SEEDS = 32
F16_MAX = 65504.0

# name: (config, B, data): every shape from tests/test_gpu_bf16.py CASES
SHAPES = {
    "bern_LB_tails": (dict(D=200, H=136, Z=24), 200, "mnist"),            # row / column / K tails, no bit tile
    "bern_LB": (dict(D=256, H=128, Z=32), 256, "bits"),                   # binary data: x tile from bits
    "gauss_LB": (dict(D=256, H=96, Z=16, continuous=True), 192, "frey"),  # interleaved dA
    "bern_LA_L2": (dict(D=128, H=64, Z=16, estimator="LA", L=2), 136, "mnist"),
    "gauss_mean_map": (dict(D=128, H=64, Z=8, continuous=True, objective="mean_map"), 128, "frey"),   # fp16: S = 128
    "thin_tails": (dict(D=264, H=200, Z=128), 200, "mnist"),
    "thin_gauss_mean_map": (dict(D=128, H=64, Z=256, continuous=True, objective="mean_map"), 96, "frey"),   # S = 64
    "bern_LB_longk_tails": (dict(D=520, H=264, Z=24), 1100, "mnist"),
    "bern_LA_L8": (dict(D=128, H=64, Z=16, estimator="LA", L=8), 40, "mnist"),
    "gauss_LB_L5": (dict(D=128, H=64, Z=8, continuous=True, L=5), 72, "frey"),
}
# The three theta_0 shapes: tails without a bit tile, the interleaved Gaussian dA, the thin launches.  Chosen on
# the host so that neither tanh stage sits at its unraised tau: with the kernel's tanh (ftanh_bf) on the float32
# stand-in, h / hd are at 2.9 / 2.6, 0.50 / 3.2 and 2.0 / 0.59 x tau (bf16; fp16 3.1 / 2.1, 0.46 / 3.1, 2.4 / 0.34).
# gauss_mean_map and thin_gauss_mean_map put h at 1.00 and 0.96 x tau: whether they need RAISED would hang on the
# last digit of the host's float32 matrix product.
THETA0 = ("bern_LB_tails", "gauss_LB", "thin_tails")
DTYPES = ("bf16", "fp16")
CASES = [(n, "x30") for n in SHAPES] + [(n, "theta0") for n in THETA0]
CASE_IDS = [f"{n}-{s}" for n, s in CASES]
W1_DAMP = 128              # Z >= this: W1, b1 times a further sqrt(64 / Z) in the x30 state

STORED = ("h", "z", "hd", "dA2", "dA6", "dA1", "dml", "dA3")     # 16-bit stages, forward then backward
# (case, state, dtype, stage) -> (the restatement its tau rests on, that restatement's error max|. - t64| on the
# float32 stand-in, the unraised tau it exceeded).  At theta_0 max|h| ~ 0.2, so the unraised tau is ~4e-7, and
# EpiBiasAct's tanh (ftanh_bf: x itself below 2^-6, off by x^3 / 3 <= 1.27e-6; 1 - 2 / (1 + e^2x) above) exceeds
# it on the device by exactly what its float32 NumPy restatement does on the host (bern_LB_tails bf16: device
# 1.175e-6 / 1.104e-6 beyond half an ulp in h / hd, restatement 1.17e-6 / 1.10e-6).  tau = MARGIN x the
# restatement's error, computed from the step's own inputs (tau_of); the figures here are the record.
RAISED = {
    ("bern_LB_tails", "theta0", "bf16", "h"): ("ftanh_bf", 1.27e-6, 4.0e-7),
    ("bern_LB_tails", "theta0", "bf16", "hd"): ("ftanh_bf", 1.27e-6, 4.2e-7),
    ("bern_LB_tails", "theta0", "fp16", "h"): ("ftanh_bf", 1.27e-6, 4.0e-7),
    ("bern_LB_tails", "theta0", "fp16", "hd"): ("ftanh_bf", 1.27e-6, 5.8e-7),
    ("gauss_LB", "theta0", "bf16", "hd"): ("ftanh_bf", 1.27e-6, 3.2e-7),
    ("gauss_LB", "theta0", "fp16", "hd"): ("ftanh_bf", 1.27e-6, 3.95e-7),
    ("thin_tails", "theta0", "bf16", "h"): ("ftanh_bf", 1.27e-6, 5.1e-7),
    ("thin_tails", "theta0", "fp16", "h"): ("ftanh_bf", 1.27e-6, 5.1e-7),
}


def config(name):
    return O.Config(**SHAPES[name][0])


def batch(name):
    return SHAPES[name][1]


def loss_scale(cfg, B, dtype):
    """engine_bf16.inc h16_scale."""
    if dtype != "fp16" or cfg.objective != "mean_map":
        return 1.0
    return float(2 ** int(math.floor(math.log2(B))))


def data_of(name):
    cfg, B, kind = config(name), batch(name), SHAPES[name][2]
    if kind == "frey":
        return O.synthetic_frey(n=NB * B, D=cfg.D, seed=0)
    if kind == "bits":
        from vaeb_amd.synthetic import synth_like
        return synth_like(NB * B, D=cfg.D)
    return O.synthetic_mnist(n=NB * B, D=cfg.D, seed=0)


# ------------------------------------------------------------------ the 16-bit formats
def rounder(dtype, S=1.0):
    if dtype == "bf16":
        return O.bf16_round
    return O.fp16_round_scaled(S) if S != 1.0 else O.fp16_round


def to_bits(a, dtype):
    """float array -> the raw 16-bit words of its nearest 16-bit values."""
    a = np.ascontiguousarray(a, np.float32)
    if dtype == "fp16":
        return a.astype(np.float16).view(np.uint16)
    return (O.bf16_round(a).view(np.uint32) >> 16).astype(np.uint16)


def from_bits(u, dtype):
    """raw 16-bit words -> float64."""
    u = np.ascontiguousarray(u, np.uint16)
    if dtype == "fp16":
        return u.view(np.float16).astype(np.float64)
    return (u.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def store16(t, dtype):
    """A value stored in 16 bits and read back (float64)."""
    return from_bits(to_bits(t, dtype), dtype)


def ulp16(t, dtype):
    """The spacing of the 16-bit format at t (float64): 2^(floor(log2 |t|) - p), p = 7 (bf16) or 10
    (fp16), the exponent held at the smallest normal's below it."""
    p, emin = (7, -126) if dtype == "bf16" else (10, -14)
    t = np.abs(np.asarray(t, np.float64))
    _, e = np.frexp(t)                                       # |t| = m 2^e, m in [0.5, 1)
    return np.ldexp(1.0, np.where(t == 0, emin, np.maximum(e - 1, emin)) - p)


# ------------------------------------------------------------------ inputs
def theta0(cfg, B, seed):
    """(params, eps) as test_bf16_step_parity draws them."""
    rng = np.random.default_rng(seed)
    params = [p if p.ndim == 2 else (0.01 * rng.standard_normal(p.shape)).astype(np.float32)
              for p in O.init_params(cfg)]
    eps = rng.standard_normal((cfg.L, B, cfg.Z)).astype(np.float32)
    return params, eps


def draw(name, state, seed):
    cfg, B = config(name), batch(name)
    params, eps = theta0(cfg, B, seed)
    if state == "x30":
        params = F.scale_params(cfg, params)
        if cfg.Z >= W1_DAMP:
            f = np.float32(math.sqrt(F.WIDE / cfg.Z))
            params = [p * f if n in ("W1", "b1") else p for n, p in zip(cfg.names, params)]
    else:
        assert state == "theta0"
    acc = [np.full_like(p, ACC0) for p in params]
    return params, acc, eps


def scaled_store_max(cfg, out, S):
    """max|.| of every 16-bit store of one oracle step, the backward's times the loss scale."""
    m = {k: float(np.abs(out[k]).max()) for k in ("h", "z", "hd")}
    for k in ("dA2", "dA6", "dA1", "dMu", "dLv", "dA3"):
        if k in out:
            m[k] = S * float(np.abs(out[k]).max())
    return m


def fair(name, state, seed):
    """(reasons the seed is not fair, the figures)."""
    cfg, B = config(name), batch(name)
    params, _, eps = draw(name, state, seed)
    S = loss_scale(cfg, B, "fp16")
    xb = data_of(name)[IDX * B:(IDX + 1) * B].astype(np.float64)
    with np.errstate(all="ignore"):
        out = O.forward_backward(F.f64(params), xb, eps.astype(np.float64), cfg, q=rounder("fp16", S))
    s = F.stats(cfg, out)
    sm = scaled_store_max(cfg, out, S)
    s["store_max"] = max(sm.values())
    bad = F.fair_reasons(cfg, state, s)
    if not all(np.isfinite(v) and v <= F16_MAX for v in sm.values()):
        bad.append("a 16-bit store outside fp16's range")
    return bad, s


@dataclasses.dataclass
class Case:
    name: str
    state: str
    seed: int
    cfg: O.Config
    B: int
    x: np.ndarray            # the data set, float32 [NB B, D]
    eps: np.ndarray          # [L, B, Z] float32
    params: list
    acc: list
    stats: dict

    def theta(self):
        return O.flatten(self.params)

    def acc_flat(self):
        return O.flatten(self.acc)

    def xb(self):
        return self.x[IDX * self.B:(IDX + 1) * self.B]


@functools.lru_cache(maxsize=None)
def case(name, state):
    for seed in range(SEED0, SEED0 + MAX_SEEDS):
        bad, s = fair(name, state, seed)
        if not bad:
            params, acc, eps = draw(name, state, seed)
            c = Case(name, state, seed, config(name), batch(name), data_of(name), eps, params, acc, s)
            for a in [c.x, c.eps] + list(params) + list(acc):
                a.setflags(write=False)
            return c
    raise AssertionError(f"{name}-{state}: no fair seed in {MAX_SEEDS} tries")


# ------------------------------------------------------------------ the stages
def sigmoid(a):
    return 1 / (1 + np.exp(-a))


def weights_of(cfg, flat, dtype):
    """{name: float64 array} of an arena's parameters: the weights as the shadow holds them (16-bit),
    the biases as they are (fp32)."""
    out = {}
    for n, p in zip(cfg.names, O.unflatten(np.asarray(flat, np.float32), cfg)):
        out[n] = store16(p, dtype) if n.startswith("W") else p.astype(np.float64)
    return out


def ftanh_bf(x):
    """gemm_bf16.hpp ftanh_bf (the tanh of EpiBiasAct: enc and dechid) restated in float32 NumPy:
    1 - 2 / (1 + 2^(x 2 log2 e)), and x itself below 2^-6 (|tanh x - x| < x^3 / 3 <= 1.3e-6 there)."""
    x = np.asarray(x, np.float32)
    k = np.float32(2) * np.float32(1.4426950408889634)
    t = np.float32(1) - np.float32(2) / (np.float32(1) + np.exp2(x * k))
    return np.where(np.abs(x) < np.float32(0.015625), x, t).astype(np.float32)


def stage_values(c, S, X, W, dev, dt, std_fn=None, dtanh_hd=None, tanh=None):
    """{stage: pre-rounding value} of every stage in dtype dt, each from the stored inputs `dev` the
    kernel reads (decoded to float), the 16-bit data X [B, D] and the weights W (weights_of).
    std_fn / dtanh_hd: what a mutant of tests/test_h16_stage_host.py replaces; tanh: the kernel's own
    (ftanh_bf) for a restatement of RAISED."""
    tanh = tanh or np.tanh
    cfg, B, L, Z = c.cfg, c.B, c.cfg.L, c.cfg.Z
    a = lambda v: np.asarray(v, dt)
    w = {k: a(v) for k, v in W.items()}
    std_fn = std_fn or (lambda lv: np.exp(dt(0.5) * lv))
    dtanh_hd = dtanh_hd or (lambda hd: 1 - hd * hd)
    sc = 1.0 / B if cfg.objective == "mean_map" else 1.0
    s_, sl = dt(sc * S), dt(sc * S / L)
    half = dt(0.5)
    X = a(X)
    h, mu, lv, eps = a(dev["h"]), a(dev["mu"]), a(dev["lv"]), a(dev["eps"])
    z, hd, dA1, dml = a(dev["z"]), a(dev["hd"]), a(dev["dA1"]), a(dev["dml"])
    W45 = np.concatenate([w["W4"], w["W5"]], axis=1)
    t = {}
    t["h"] = tanh(X @ w["W3"] + w["b3"])
    t["mulv"] = h @ W45 + np.concatenate([w["b4"], w["b5"]])
    std = std_fn(lv)
    z3 = mu[None] + std[None] * eps
    t["z"] = z3.reshape(L * B, Z)
    t["hd"] = tanh(z @ w["W1"] + w["b1"])
    xr = np.tile(X, (L, 1))
    y = sigmoid(hd @ w["W2"] + w["b2"])
    if cfg.continuous:
        r, e = xr - y, np.exp(-(hd @ w["W6"] + w["b6"]))
        t["dA2"] = sl * r * e * y * (1 - y)
        t["dA6"] = sl * (-half + half * r * r * e)
    else:
        t["dA2"] = sl * (xr - y)
    dHd = a(dev["dA2"]) @ w["W2"].T
    if cfg.continuous:
        dHd = dHd + a(dev["dA6"]) @ w["W6"].T
    t["dA1"] = dHd * dtanh_hd(hd)
    dZ = (dA1 @ w["W1"].T).reshape(L, B, Z)
    std0 = np.exp(half * lv)                 # the latent backward recomputes sd and z from mu, lv, eps
    zb = mu[None] + std0[None] * eps
    if cfg.estimator == "LA":
        dMu = dZ.sum(0) + sl * (-zb).sum(0)
        dLv = (dZ * half * std0[None] * eps).sum(0) + sl * (half - half * zb * std0[None] * eps).sum(0)
    else:
        dMu = dZ.sum(0) - s_ * mu
        dLv = (dZ * half * std0[None] * eps).sum(0) + s_ * half * (1 - np.exp(lv))
    t["dml"] = np.concatenate([dMu, dLv], axis=1)
    t["dA3"] = (dml @ W45.T) * (1 - h * h)
    assert all(v.dtype == dt for v in t.values()), {k: v.dtype for k, v in t.items()}
    return t


def grad_operands(c, X, dev):
    """{weight gradient: (A, B)} with g = A^T B / S, and {bias gradient: stored operand}; all as the
    device stores them (float64).  [W4 | W5] and [b4 | b5] split at column Z."""
    Z = c.cfg.Z
    ops = {"gW3": (X, dev["dA3"]), "gW4": (dev["h"], dev["dml"][:, :Z]), "gW5": (dev["h"], dev["dml"][:, Z:]),
           "gW1": (dev["z"], dev["dA1"]), "gW2": (dev["hd"], dev["dA2"])}
    bias = {"gb3": dev["dA3"], "gb4": dev["dml"][:, :Z], "gb5": dev["dml"][:, Z:], "gb1": dev["dA1"], "gb2": dev["dA2"]}
    if c.cfg.continuous:
        ops["gW6"] = (dev["hd"], dev["dA6"])
        bias["gb6"] = dev["dA6"]
    return ops, bias


# ------------------------------------------------------------------ the criterion
@dataclasses.dataclass
class Finding:
    stage: str
    kind: str                # "stored" | "gemm" | "bias"
    dev: float               # the error of the worst element (stored: beyond half an ulp)
    restate: float           # the float32 restatement's error (stored) / the operands' |A| |B| (gemm) there
    bound: float
    where: tuple             # (row, column) of the worst element
    flipped: float = 0.0     # stored: the share of elements that are not Q(t64)

    @property
    def ratio(self):
        return self.dev / self.bound if self.dev == self.dev else math.inf

    def line(self):
        r, col = self.where
        return (f"{self.stage} [{self.kind}] at ({r}, {col}), 16-tile ({r // 16}, {col // 16}), 64-block ({r // 64}, "
                f"{col // 64}): {self.dev:.3e} / {self.restate:.3e} / {self.bound:.3e}")


def tau_of(c, dtype, stage, t32, t64, raised=True):
    """(tau, the restatement error it rests on).  A RAISED stage: MARGIN x the error of its kernel
    restatement (t32 is then that restatement's value), computed here from the same inputs."""
    r = float(np.abs(t32.astype(np.float64) - t64).max())
    if raised and (c.name, c.state, dtype, stage) in RAISED:
        return MARGIN * r, r
    return MARGIN * max(r, ULP32 * float(np.abs(t64).max())), r


def worst(excess, bound):
    """Index of the element furthest past (or nearest to) its bound; NaN counts as furthest."""
    with np.errstate(all="ignore"):
        q = np.where(np.isfinite(excess), excess / bound, np.inf)
    return np.unravel_index(int(np.argmax(q)), q.shape)


def judge_stored(c, dtype, stage, v, t32, t64, raised=True):
    tau, r = tau_of(c, dtype, stage, t32, t64, raised)
    over = np.abs(v - t64) - 0.5 * ulp16(t64, dtype)
    i = worst(over, np.full(over.shape, tau))
    flipped = float(np.mean(v != store16(t64, dtype)))
    return Finding(stage, "stored", max(float(over[i]), 0.0) if over[i] == over[i] else math.nan, r, tau, tuple(int(k) for k in i),
                   flipped)


def judge_gemm(stage, got, A, Bm, S=1.0, bias=None):
    """got (fp32) against A^T-free product A @ Bm / S (+ bias) of stored operands, in float64."""
    ref = A @ Bm / S
    bound = GEMM_TOL * (np.abs(A) @ np.abs(Bm)) / S + 1e-30
    if bias is not None:
        ref = ref + bias
        bound = bound + ULP32 * np.abs(ref)
    err = np.abs(np.asarray(got, np.float64) - ref)
    i = worst(err, bound)
    return Finding(stage, "gemm", float(err[i]), float(bound[i] / GEMM_TOL), float(bound[i]), tuple(int(k) for k in i))


def judge_bias(stage, got, stored, dtype, S=1.0):
    ref = stored.sum(0) / S
    bound = ((0.5 * ulp16(stored, dtype)).sum(0) + ULP32 * np.abs(stored).sum(0)) / S + 1e-30
    err = np.abs(np.asarray(got, np.float64) - ref)
    i = worst(err, bound)
    return Finding(stage, "bias", float(err[i]), float(np.abs(stored).sum(0)[i] / S), float(bound[i]), (0, int(i[0])))


def judge(c, dtype, dev, grads, raised=True):
    """[Finding] of one step: dev = {buffer: float64 array of the valid rows} as stored (h, mu, lv,
    eps [L, B, Z], z, hd, dA2 (, dA6), dA1, dml, dA3; the backward's carry the loss scale), grads =
    {"gW3": ...} the reported data gradients, the weights those of the arena before the step.
    raised=False: every stage at its unraised tau (tests/test_h16_stage_host.py)."""
    cfg, B = c.cfg, c.B
    S = loss_scale(cfg, B, dtype)
    X = store16(c.xb(), dtype)
    W = weights_of(cfg, c.theta(), dtype)
    t64 = stage_values(c, S, X, W, dev, np.float64)
    t32 = stage_values(c, S, X, W, dev, np.float32)
    if raised and any(k[:3] == (c.name, c.state, dtype) for k in RAISED):
        tk = stage_values(c, S, X, W, dev, np.float32, tanh=ftanh_bf)
        t32 = {k: tk[k] if (c.name, c.state, dtype, k) in RAISED else v for k, v in t32.items()}
    out = []
    for k in STORED:
        if k in t64:
            out.append(judge_stored(c, dtype, k, dev[k], t32[k], t64[k], raised))
    W45 = np.concatenate([W["W4"], W["W5"]], axis=1)
    out.append(judge_gemm("mulv", np.concatenate([dev["mu"], dev["lv"]], axis=1), dev["h"], W45,
                          bias=np.concatenate([W["b4"], W["b5"]])))
    ops, bias = grad_operands(c, X, dev)
    for k, (A, Bm) in ops.items():
        out.append(judge_gemm(k, grads[k], A.T, Bm, S))
    for k, st in bias.items():
        out.append(judge_bias(k, grads[k], st, dtype, S))
    return out


def rejected(findings):
    return [f for f in findings if not f.dev <= f.bound]


def table_line(label, findings):
    f = max(findings, key=lambda f: f.ratio)
    return f"{label:40s} {f.stage:5s} {f.dev:.1e} / {f.restate:.1e} / {f.bound:.1e}"


def today_rel(a, b):
    """The norm-wise measure of tests/test_gpu_bf16.py."""
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# ------------------------------------------------------------------ the float32 stand-in for the device
def region_mask(form, diff, t):
    """Where a mutant that reaches inside a stage applies: "all", the first 16 x 16 "tile" (clipped to
    the array), its last "4x4" elements, or "1": the element of that tile the mutant changes most in
    units of its own size (so of its 16-bit spacing)."""
    m = np.zeros(diff.shape, bool)
    r1, c1 = min(16, diff.shape[0]), min(16, diff.shape[1])
    if form == "all":
        m[:] = True
    elif form == "tile":
        m[:r1, :c1] = True
    elif form == "4x4":
        m[r1 - 4:r1, c1 - 4:c1] = True
    else:
        assert form == "1"
        rel = np.abs(diff[:r1, :c1]) / (np.abs(t[:r1, :c1]) + 1e-30)
        m[np.unravel_index(int(np.argmax(rel)), rel.shape)] = True
    return m


def simulate(c, dtype, mutate=None):
    """One step as a device that computes every stage in float32 from its own stored operands would
    leave it: (dev, grads) in judge()'s form.  mutate(stage, value, dev) -> value replaces a stage's
    float32 output before it is stored (tests/test_h16_stage_host.py); its attributes reach inside a
    stage: std_fn / dtanh_hd (stage_values) within `region` (region_mask), swap, drop_k; amp < 1 applies
    that share of the change only."""
    cfg, B, L, Z = c.cfg, c.B, c.cfg.L, c.cfg.Z
    S = loss_scale(cfg, B, dtype)
    X = store16(c.xb(), dtype)
    W = weights_of(cfg, c.theta(), dtype)
    mut = mutate or (lambda stage, v, dev: v)
    kw = {k: getattr(mutate, k) for k in ("std_fn", "dtanh_hd") if hasattr(mutate, k)}
    amp = np.float32(getattr(mutate, "amp", 1.0))     # the share of the mutant's change that is applied
    zero = lambda *s: np.zeros(s)
    dev = {"h": zero(B, cfg.H), "mu": zero(B, Z), "lv": zero(B, Z), "eps": c.eps.astype(np.float64), "z": zero(L * B, Z),
           "hd": zero(L * B, cfg.H), "dA2": zero(L * B, cfg.D), "dA1": zero(L * B, cfg.H), "dml": zero(B, 2 * Z),
           "dA3": zero(B, cfg.H)}
    if cfg.continuous:
        dev["dA6"] = zero(L * B, cfg.D)
    raw = {}                                   # the unrounded float32 stage outputs (the bias gradients sum these)
    order = ("h", "mulv", "z", "hd", "dA2", "dA1", "dml", "dA3")
    tanh = getattr(mutate, "tanh", None)       # ftanh_bf: the stand-in with the kernel's own tanh
    for k in order:
        t = stage_values(c, S, X, W, dev, np.float32, tanh=tanh)
        names = ("dA2", "dA6") if k == "dA2" and cfg.continuous else (k,)
        vals = {n: t[n].copy() for n in names}
        if kw:
            tm = stage_values(c, S, X, W, dev, np.float32, tanh=tanh, **kw)
            for n in names:
                d = tm[n] - t[n]
                vals[n] = np.where(region_mask(getattr(mutate, "region", "all"), d, t[n]), t[n] + amp * d, t[n])
        if k == "dA2" and cfg.continuous and hasattr(mutate, "swap"):
            rows, cols = mutate.swap           # dA2 and dA6 exchanged there (one interleave group, or less of it)
            d = amp * (t["dA6"][rows, cols] - t["dA2"][rows, cols])
            vals["dA2"][rows, cols] += d
            vals["dA6"][rows, cols] -= d
        for n in names:
            v = mut(n, vals[n], dev)
            raw[n] = v
            if n == "mulv":
                dev["mu"], dev["lv"] = v[:, :Z].astype(np.float64), v[:, Z:].astype(np.float64)
            else:
                dev[n] = store16(v, dtype)
    ops, bias = grad_operands(c, X, dev)
    inv = np.float32(1.0 / S)
    drop = getattr(mutate, "drop_k", None)
    grads = {}
    for k, (A, Bm) in ops.items():
        g = (A.astype(np.float32).T @ Bm.astype(np.float32)) * inv
        if drop and drop[0] == k:
            _, n, kt = drop                    # the first n x n outputs without the last K block of kt rows
            g[:n, :n] = (A[:-kt, :n].astype(np.float32).T @ Bm[:-kt, :n].astype(np.float32)) * inv
        grads[k] = g
    rawb = {"gb3": raw["dA3"], "gb4": raw["dml"][:, :Z], "gb5": raw["dml"][:, Z:], "gb1": raw["dA1"], "gb2": raw["dA2"]}
    if cfg.continuous:
        rawb["gb6"] = raw["dA6"]
    for k, v in rawb.items():
        grads[k] = v.sum(0, dtype=np.float32) * inv
    return dev, grads


def oracle_grads(c, dtype):
    """{"gW3": ...} of the rounded float64 oracle, and its value SGVB / B: today's reference."""
    S = loss_scale(c.cfg, c.B, dtype)
    with np.errstate(all="ignore"):
        out = O.forward_backward(F.f64(c.params), c.xb().astype(np.float64), c.eps.astype(np.float64), c.cfg,
                                 q=rounder(dtype, S))
    return {"g" + n: g for n, g in zip(c.cfg.names, out["data_grads"])}, float(out["sgvb"]) / c.B


# ------------------------------------------------------------------ reading a device step
def deinterleave(dA, D):
    """[rows, 2 D] in 32-column groups [dA2 | dA6] -> (dA2, dA6), each [rows, D]."""
    g = dA.reshape(dA.shape[0], D // 32, 2, 32)
    return g[:, :, 0].reshape(-1, D), g[:, :, 1].reshape(-1, D)


def read_step(ctx, c, dtype):
    """(dev, grads, g_flat) of the step a 16-bit context has just taken (keep_grads), valid rows, in
    judge()'s form."""
    cfg, B, L, D, H, Z = c.cfg, c.B, c.cfg.L, c.cfg.D, c.cfg.H, c.cfg.Z
    rd = lambda k, rows, w: from_bits(ctx.get_h16(k, rows * w), dtype).reshape(rows, w)
    dev = {"h": rd("h", B, H), "z": rd("z", L * B, Z), "hd": rd("hd", L * B, H), "dA1": rd("dA1", L * B, H),
           "dml": rd("dml", B, 2 * Z), "dA3": rd("dA3", B, H)}
    if cfg.continuous:
        assert D % 32 == 0
        dev["dA2"], dev["dA6"] = deinterleave(rd("dA", L * B, 2 * D), D)
    else:
        dev["dA2"] = rd("dA", L * B, D)
    for k in ("mu", "lv"):
        dev[k] = ctx.get_h16(k, B * Z).reshape(B, Z).astype(np.float64)
    dev["eps"] = ctx.get_h16("eps", L * B * Z).reshape(L, B, Z).astype(np.float64)
    g = ctx.get_grads()
    grads = {"g" + n: gg.reshape(s).astype(np.float64) for (n, s), gg in zip(O.param_shapes(cfg), O.unflatten(g, cfg))}
    return dev, grads, g
