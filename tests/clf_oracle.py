"""The softmax MLP classifier (include/vaeb_hip.h vaeb_clf_*, vaeb_amd/csrc/engine_clf.inc,
clf_softmax.hpp) in NumPy -- TEST HELPER ONLY: the dtype-generic forward / backward for both losses
and under weight-dropout masks, the host mask (oracle/philox.py's Philox at the classifier's counter
site), the case table and the per-case float64 oracle / float32 restatement shared by
tests/test_clf_host.py (no GPU) and tests/test_gpu_clf.py.

The dtype of params is the dtype of the run: fed float64 arrays forward_backward is the oracle, fed
float32 arrays it is the float32 restatement that sets every device bound (MARGIN x its error, the
criterion of tests/ae_grad_cases.py, whose constants and block-error measure are imported, not
restated).  No bound comes from the device.

Gradients are those of f = sum of the rows' log-likelihood (+ the N(0, s2) prior with cfg.prior) with
respect to the REAL theta: under masks m the network runs on theta * m and dloglik/dtheta =
m * dloglik/dtheta~, so a dropped parameter's gradient is exactly -theta / s2 (0 without a prior).
"""
import dataclasses
import functools
import math

import numpy as np

from oracle import philox as PH
from tests import optim_oracle as OO
from tests.ae_grad_cases import GRAD_CAP, KINK, MARGIN, SCALE, VALUE_RTOL, WIDE, block_errors, blocks  # noqa: F401

EPS_LOG = 1e-7
SITE_C1 = 0x40000000          # the counter word c1 of the dropout draws
REG_WIDTH = 256               # the widest Dout clf_softmax.hpp keeps in registers (64 lanes x 4)


@dataclasses.dataclass(frozen=True)
class Cfg:
    Din: int
    Dh: tuple
    Dout: int
    act: str = "tanh"
    loss: str = "bernoulli"
    prior: bool = False
    s2: float = 1.0
    eta: float = 0.01


def param_shapes(cfg):
    d = [cfg.Din] + list(cfg.Dh)
    shp = [(f"W{i}", (d[i], d[i + 1])) for i in range(len(cfg.Dh))]
    shp += [(f"b{i}", (cfg.Dh[i],)) for i in range(len(cfg.Dh))]
    return shp + [("Wout", (cfg.Dh[-1], cfg.Dout)), ("bout", (cfg.Dout,))]


def names(cfg):
    return [n for n, _ in param_shapes(cfg)]


def init_params(cfg, seed):
    rs = np.random.RandomState(seed)
    return [rs.normal(0.0, 0.01, size=s).astype(np.float32) for _, s in param_shapes(cfg)]


def flatten(arrays):
    return np.concatenate([np.asarray(a).ravel() for a in arrays])


def unflatten(flat, cfg, dtype=None):
    out, o = [], 0
    for _, s in param_shapes(cfg):
        k = int(np.prod(s))
        out.append(np.asarray(flat[o:o + k], dtype or flat.dtype).reshape(s))
        o += k
    assert o == len(flat)
    return out


def scale_params(cfg, params):
    """tests/ae_grad_cases.py scale_params' idea: every layer x 30, a layer with more than WIDE
    inputs x 30 sqrt(WIDE / Kin)."""
    kin = {}
    for n, s in param_shapes(cfg):
        if len(s) == 2:
            kin[n] = kin["b" + n[1:]] = s[0]
    return [(p * (SCALE * min(1.0, math.sqrt(WIDE / kin[n])))).astype(np.float32) for n, p in zip(names(cfg), params)]


def _act(act, v):
    if act == "tanh":
        return np.tanh(v)
    if act == "sigmoid":
        return 1 / (1 + np.exp(-v))
    return np.maximum(v, 0)


def _dact(act, h):
    if act == "tanh":
        return 1 - h * h
    if act == "sigmoid":
        return h * (1 - h)
    return (h > 0).astype(h.dtype)


def softmax(a, subtract_max=True):
    mx = a.max(axis=1, keepdims=True) if subtract_max else np.zeros((a.shape[0], 1), a.dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(a - mx)
        S = e.sum(axis=1, keepdims=True)
        return e / S, mx, S


def forward_backward(params, X, Y, cfg, masks=None, need_grad=True, variant=None):
    """{"value": the log-likelihood sum, "rows": per row, "P", "A" (logits), "H" (activations,
    H[0] = X), "pre" (hidden pre-activations), "grads": per block, param_shapes order}.
    variant: one of the WRONG implementations tests/test_clf_host.py holds the bounds against
    ("cat_delta", "no_dot", "no_max", "wgrad_unmasked", "bwd_unmasked"); never set by a parity test."""
    dt = params[0].dtype.type
    assert all(p.dtype == params[0].dtype for p in params)
    X, Y = np.asarray(X, dt), np.asarray(Y, dt)
    nh = len(cfg.Dh)
    eff = params if masks is None else [p * np.asarray(m, dt) for p, m in zip(params, masks)]
    W, b, Wout, bout = eff[:nh], eff[nh:2 * nh], eff[2 * nh], eff[2 * nh + 1]
    H, pre = [X], []
    for i in range(nh):
        pre.append(H[-1] @ W[i] + b[i])
        H.append(_act(cfg.act, pre[-1]))
    A = H[-1] @ Wout + bout
    P, mx, S = softmax(A, subtract_max=variant != "no_max")
    eps = dt(EPS_LOG)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if cfg.loss == "bernoulli":
            rows = (Y * np.log(P + eps) + (1 - Y) * np.log(1 - P + eps)).sum(axis=1)
        else:
            rows = (Y * (A - mx - np.log(S))).sum(axis=1)
    out = {"value": rows.sum(dtype=np.float64) if dt is np.float64 else rows.sum(), "rows": rows, "P": P, "A": A,
           "H": H, "pre": pre}
    if not need_grad:
        return out
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if cfg.loss == "bernoulli" and variant != "cat_delta":
            dP = Y / (P + eps) - (1 - Y) / (1 - P + eps)
            dot = dt(0) if variant == "no_dot" else (P * dP).sum(axis=1, keepdims=True)
            d = P * (dP - dot)
        else:
            d = Y - P * Y.sum(axis=1, keepdims=True)
    back = params if variant == "bwd_unmasked" else eff      # the weights the data backward reads
    gW, gb = [None] * nh, [None] * nh
    gWout, gbout = H[-1].T @ d, d.sum(axis=0)
    dh = (d @ back[2 * nh].T) * _dact(cfg.act, H[-1])
    for i in range(nh - 1, -1, -1):
        gW[i], gb[i] = H[i].T @ dh, dh.sum(axis=0)
        if i:
            dh = (dh @ back[i].T) * _dact(cfg.act, H[i])
    grads = gW + gb + [gWout, gbout]
    if masks is not None and variant != "wgrad_unmasked":
        grads = [g * np.asarray(m, dt) for g, m in zip(grads, masks)]
    if cfg.prior:
        grads = [g - p / dt(cfg.s2) for g, p in zip(grads, params)]
    out["grads"] = [np.asarray(g, params[0].dtype) for g in grads]
    return out


# ------------------------------------------------------------------ the dropout mask on the host
def threshold(keep):
    """T = floor(keep 2^32) from the float32 keep, as the engine forms it (in double)."""
    return int(math.floor(float(np.float32(keep)) * 4294967296.0))


def host_mask(seed, step, draw, P, keep):
    """uint8 [P]: parameter i is kept iff output word i & 3 of the Philox block at (c0 = i >> 2,
    c1 = SITE_C1, c23(step, domain)) is below T.  draw -1: the training domain 0; draw l >= 0: the
    evaluation domain 1 | (l + 1) << 1."""
    g = np.arange((int(P) + 3) // 4, dtype=np.uint64)
    c = PH.c23(step, 0 if draw < 0 else 1 | ((int(draw) + 1) << 1))
    seed = PH._u64(seed)
    w = PH.philox4x32_10(g & PH.M32, np.uint64(SITE_C1), c & PH.M32, c >> PH._S32, seed & PH.M32, seed >> PH._S32)
    words = np.stack(w, axis=1).ravel()[:int(P)]
    return (words < np.uint64(threshold(keep))).astype(np.uint8) if threshold(keep) < 2 ** 32 else np.ones(int(P), np.uint8)


def split_mask(flat, cfg):
    return unflatten(np.asarray(flat), cfg)


def row_masks(cfg, seed, step, keep):
    """A WRONG mask: one draw per row of each W (per element of a b) instead of one per parameter."""
    shapes = param_shapes(cfg)
    n = sum(s[0] for _, s in shapes)
    m = host_mask(seed, step, -1, n, keep)
    out, o = [], 0
    for _, s in shapes:
        r = m[o:o + s[0]]
        out.append(np.repeat(r[:, None], s[1], axis=1) if len(s) == 2 else r.copy())
        o += s[0]
    return out


# ------------------------------------------------------------------ the case table
# name: (Din, Dh, Dout, act, batch, what).  The smallest shapes at which the kernels can still go wrong.
SHAPES = {
    "edge": (37, (17, 33), 10, "tanh", 17, "N and M one past a tile"),
    "b1": (33, (16,), 2, "relu", 1, "K = 1 weight gradients, the smallest softmax, dead units"),
    "d17": (31, (32,), 17, "sigmoid", 15, "one past a 16-lane row"),
    "d65": (24, (15,), 65, "tanh", 33, "one past a wavefront"),
    "d257": (40, (31,), REG_WIDTH + 1, "tanh", 20, "the looping path: one past the width kept in registers"),
    "k513": (513, (33,), 10, "tanh", 33, "forward K = 513"),
    "b513": (20, (18,), 5, "tanh", 513, "the deep weight-gradient loop"),
}
LOSSES = ("bernoulli", "categorical")
CASES = [(n, sc, loss) for n in SHAPES for sc in (False, True) for loss in LOSSES]
CASE_IDS = [f"{n}-{'x30' if sc else 'theta0'}-{loss}" for n, sc, loss in CASES]
MASK_SEED, MASK_STEP, KEEP = 15485863, 3, 0.5
MAX_SEEDS = 64


def cfg_of(name, loss="bernoulli", prior=False, s2=1.0):
    Din, Dh, Dout, act, _, _ = SHAPES[name]
    return Cfg(Din, Dh, Dout, act, loss, prior, s2)


def data_for(cfg, n, seed):
    rng = np.random.default_rng(seed)
    X = rng.random((n, cfg.Din)).astype(np.float32)
    Y = np.zeros((n, cfg.Dout), np.float32)
    Y[np.arange(n), rng.integers(0, cfg.Dout, n)] = 1.0
    return X, Y


def draw(cfg, B, scaled, seed):
    params = init_params(cfg, 15485863 + seed)
    if scaled:
        params = scale_params(cfg, params)
    Xtr, Ytr = data_for(cfg, 2 * B + 16, seed)
    idx = np.random.default_rng(100 + seed).choice(Xtr.shape[0], size=B, replace=False).astype(np.int32)
    return params, Xtr, Ytr, idx


def fair(cfg, params, Xtr, Ytr, idx, masks):
    """relu rows: no float64 hidden pre-activation within KINK of 0 (float32 and float64 then agree on
    the side of the kink) and 20 % to 80 % of the hidden units dead."""
    if cfg.act != "relu":
        return True
    out = forward_backward([p.astype(np.float64) for p in params], Xtr[idx], Ytr[idx], cfg, masks, need_grad=False)
    pre = np.concatenate([a.ravel() for a in out["pre"]])
    return float(np.abs(pre).min()) >= KINK and 0.2 <= float((pre <= 0).mean()) <= 0.8


@dataclasses.dataclass
class Step:
    cfg: Cfg
    params: list               # float32
    Xtr: np.ndarray
    Ytr: np.ndarray
    idx: np.ndarray
    masks: object              # list of uint8 arrays, or None
    out64: dict
    g64: dict                  # {block: float64 gradient}
    restate: dict              # {block: error of the float32 restatement}; blocks with g64 == 0 left out
    bound: dict
    zero: list                 # blocks whose float64 gradient is identically zero
    value64: float
    restate_value: float
    restate_P: float           # max |P32 - P64|

    def theta(self):
        return flatten(self.params)

    def shapes(self):
        return param_shapes(self.cfg)


def nonzero(g64):
    return {n: g for n, g in g64.items() if np.abs(g).max() > 0}


def make_step(cfg, params, Xtr, Ytr, idx, masks=None):
    X, Y = Xtr[idx], Ytr[idx]
    out64 = forward_backward([p.astype(np.float64) for p in params], X, Y, cfg, masks)
    out32 = forward_backward(params, X, Y, cfg, masks)
    assert out32["grads"][0].dtype == np.float32 and out32["P"].dtype == np.float32
    g64 = dict(zip(names(cfg), out64["grads"]))
    g32 = dict(zip(names(cfg), [g.astype(np.float64) for g in out32["grads"]]))
    nz = nonzero(g64)
    restate = block_errors({n: g32[n] for n in nz}, nz)
    v64 = float(out64["value"])
    return Step(cfg, params, Xtr, Ytr, idx, masks, out64, g64, restate, {n: MARGIN * e for n, e in restate.items()},
                [n for n in g64 if n not in nz], v64, abs(float(out32["value"]) - v64) / abs(v64),
                float(np.abs(out32["P"].astype(np.float64) - out64["P"]).max()))


@functools.lru_cache(maxsize=None)
def case(name, scaled, loss, masked=False, prior=False):
    """The Step of one table case; masked: under the host mask of (MASK_SEED, MASK_STEP) at KEEP."""
    cfg = cfg_of(name, loss, prior, s2=2.0)
    B = SHAPES[name][4]
    P = sum(int(np.prod(s)) for _, s in param_shapes(cfg))
    masks = split_mask(host_mask(MASK_SEED, MASK_STEP, -1, P, KEEP), cfg) if masked else None
    for seed in range(MAX_SEEDS):
        params, Xtr, Ytr, idx = draw(cfg, B, scaled, seed)
        if fair(cfg, params, Xtr, Ytr, idx, masks):
            step = make_step(cfg, params, Xtr, Ytr, idx, masks)
            for a in [Xtr, Ytr, idx] + params:
                a.setflags(write=False)
            return step
    raise AssertionError(f"{name}: no fair seed below {MAX_SEEDS}")


def device_errors(step, gflat):
    """({block: error} over the blocks with a non-zero float64 gradient, [zero blocks that are not
    exactly zero in gflat])."""
    g = blocks(gflat, step.shapes())
    nz = nonzero(step.g64)
    return block_errors({n: g[n] for n in nz}, nz), [n for n in step.zero if np.any(g[n] != 0)]


# ------------------------------------------------------------------ the saturated case
SAT_P_ATOL = 1e-6             # the device's bound on |P - P64| and |sum_j P_ij - 1| there


@functools.lru_cache(maxsize=None)
def saturated(loss):
    """12-9-10 tanh, hidden weights theta_0 x 30, output weights N(0, 40^2) (logits of order 60:
    exp(a) overflows float32 without the max subtraction), half the rows labelled one class past the
    arg-max.  A logit of that size carries ~1e-5 of float32 rounding, which a row with two
    near-equal leading logits turns into ~2.5e-6 of P: the seed is the first whose float32
    restatement keeps |P32 - P64| within a quarter of SAT_P_ATOL, so the device's 1e-6 asks for
    float32 arithmetic and not for luck."""
    cfg = Cfg(12, (9,), 10, "tanh", loss)
    B = 24
    for seed in range(7, 7 + MAX_SEEDS):
        rs = np.random.RandomState(seed)
        params = init_params(cfg, seed)
        params[0] = (params[0] * 30).astype(np.float32)
        params[2] = rs.normal(0.0, 40.0, size=params[2].shape).astype(np.float32)
        X = rs.random_sample((B, cfg.Din)).astype(np.float32)
        P = forward_backward([p.astype(np.float64) for p in params], X, np.zeros((B, cfg.Dout)), cfg, need_grad=False)["P"]
        cls = (P.argmax(axis=1) + (np.arange(B) % 2)) % cfg.Dout
        Y = np.zeros((B, cfg.Dout), np.float32)
        Y[np.arange(B), cls] = 1.0
        step = make_step(cfg, params, X, Y, np.arange(B, dtype=np.int32))
        if 4 * step.restate_P <= SAT_P_ATOL:
            step.seed = seed
            return step
    raise AssertionError("saturated: no seed below the restatement condition")


# ------------------------------------------------------------------ trajectories
def trajectory(cfg, params, S0, S1, Xtr, Ytr, batches, h, t0, dt, masks=None):
    """len(batches) steps of rule h (tests/optim_oracle.py) in dtype dt, the first at optimiser step
    t0 + 1; masks: one list per step, or None.  Returns (values (sums), theta, S0, S1)."""
    p, s0, s1 = OO.as_dtype(params, dt), OO.as_dtype(S0, dt), OO.as_dtype(S1, dt)
    vals = []
    for j, b in enumerate(batches):
        out = forward_backward(p, Xtr[np.asarray(b)], Ytr[np.asarray(b)], cfg, None if masks is None else masks[j])
        vals.append(float(out["value"]))
        p, s0, s1 = OO.apply(p, s0, s1, out["grads"], h, t0 + 1 + j)
    return vals, p, s0, s1


def accuracy(Y, P):
    """mlp.py:367-373: rows with Y[i, argmax_j P_ij] == 1 (a count)."""
    return int((Y[np.arange(Y.shape[0]), np.argmax(P, axis=1)] == 1.0).sum())


# ------------------------------------------------------------------ "it learns"
LEARN_SEED, LEARN_DH, LEARN_ETA, LEARN_BATCH, LEARN_EPOCHS = 15485863, (32,), 0.1, 100, 5


@functools.lru_cache(maxsize=None)
def learn_setup():
    """(Xtr, Ytr, Xte, Yte, theta_0): GenerateGaussians(1000, 1000) and then theta_0, both from the
    global numpy RNG seeded with LEARN_SEED in the reference's order (mlp.py:424-428); the global RNG
    is put back as it was."""
    from vaeb_amd import mlp
    state = np.random.get_state()
    try:
        np.random.seed(LEARN_SEED)
        data = mlp.GenerateGaussians(1000, 1000)
        cfg = Cfg(2, LEARN_DH, 2, "tanh", eta=LEARN_ETA)
        theta0 = [np.random.normal(0.0, 0.01, size=s).astype(np.float32) for _, s in param_shapes(cfg)]
    finally:
        np.random.set_state(state)
    return (*data, theta0)


@functools.lru_cache(maxsize=None)
def learn_oracle():
    """The float64 MAP run of the "it learns" schedule: (test accuracy, train accuracy, values)."""
    Xtr, Ytr, Xte, Yte, theta0 = learn_setup()
    cfg = Cfg(2, LEARN_DH, 2, "tanh", eta=LEARN_ETA)
    rows = np.arange(Xtr.shape[0])
    batches = [rows[lb:lb + LEARN_BATCH] for lb in range(0, len(rows), LEARN_BATCH)] * LEARN_EPOCHS
    zeros = [np.zeros_like(p) for p in theta0]
    vals, p, _, _ = trajectory(cfg, theta0, zeros, [None] * len(theta0), Xtr, Ytr, batches, OO.adagrad_hyper(LEARN_ETA),
                               0, np.float64)
    acc = [accuracy(Y, forward_backward(p, X, Y, cfg, need_grad=False)["P"]) / X.shape[0] for X, Y in ((Xte, Yte), (Xtr, Ytr))]
    return acc[0], acc[1], vals
