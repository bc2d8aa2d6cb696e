"""Per-element gradient parity of the layer-stack engine's training step (vaeb_ae_train,
vaeb_amd/csrc/ae_mlp.hpp, engine_ae.inc) -- TEST HELPER ONLY: the case table, the input setup,
the gradient recovery and the per-block error shared by tests/test_ae_grads_host.py (no GPU) and
tests/test_gpu_ae_grads.py.

Recovery.  With the AdaGrad accumulator set to ZERO before the step, acc' = g^2 exactly and
theta' - theta = eta g / (|g| + 1e-6) carries the sign of g, so

    g = sign(theta' - theta) * sqrt(acc')

gives the step's gradient element by element, from the two arrays the ABI already returns.  An
element whose step rounds to nothing in float32 (|g| <~ 1e-9 beside a theta of order 1) loses its
sign and costs |g| of error, nothing on the scale below.

Error of a parameter block (an entry of param_shapes):  max|g - g64| / max|g64|, g64 the float64
oracle's gradient (oracle/ae_oracle.py, tests/vae_stack_oracle.py).

Bound of a case and block:  16 x the same measure of the float32 restatement -- the same oracle
functions fed float32 arrays, its gradient recovered in the same way from its float32 theta' and
acc'.  16 x is the margin of tests/test_gpu_eval_path.py.  No bound comes from the device.

Inputs.  Every case runs at theta_0 (N(0, 0.01) as drawn) and at scaled weights: every layer's W
and b x 30 (as tests/test_gpu_ae.py::test_ae_predict_parity), or x 30 sqrt(64 / Kin) for a layer
whose input is wider than 64, which keeps that layer's pre-activations where a 64-wide layer's
are at x 30 instead of saturating it.  idx is a gathered, unordered subset of a larger Xtr.  The
seed of a case is the first one that is fair (fair()): in the relu rows no hidden pre-activation of
the float64 forward has |a| < 1e-4 (float32 and float64 then agree on the side of the kink) and
20 % to 80 % of the hidden units are dead; at scaled weights some hidden unit and some output mean
have left their theta_0 range.  tests/test_ae_grads_host.py holds the conditions the inputs meet.
"""
import dataclasses
import functools
import math

import numpy as np

from oracle import ae_oracle as A
from tests import vae_stack_oracle as V

VALUE_RTOL = 2e-5          # the step's value: tests/test_gpu_ae.py, tests/test_vae_stack_host.py
MARGIN = 16.0              # device bound = MARGIN x the float32 restatement's error
GRAD_CAP = 1e-4            # a condition on the inputs: every bound <= the gradient cap of
                           # tests/test_gpu_many_samples.py
SCALE = 30.0
WIDE = 64                  # a layer with more inputs than this gets SCALE sqrt(WIDE / Kin)
KINK = 1e-4                # relu rows: no float64 hidden pre-activation nearer to 0 than this


@dataclasses.dataclass(frozen=True)
class Shape:
    name: str
    kw: tuple               # AEConfig keyword items
    B: int
    latents: tuple = ("point", "gauss")
    what: str = ""

    def cfg(self):
        return A.AEConfig(**dict(self.kw))


def _shape(name, B, what, latents=("point", "gauss"), **kw):
    return Shape(name, tuple(sorted(kw.items())), B, latents, what)


SHAPES = [
    _shape("edge_bin_tanh", 17, "N and M of 1, 15, 17, 31, 33; batch one past a tile",
           Dobs=37, Denc=(17, 33), Dz=1, Ddec=(15, 31), otype="binary", act="tanh", s2=2.0),
    _shape("edge_cont_sigmoid", 15, "bias row alone in a tile (Kin = 32, 16); [dA | dA2] straddling K1 = 37, "
           "[dmu | dlv] straddling K1 = 17; Dz over two column tiles",
           Dobs=37, Denc=(32,), Dz=17, Ddec=(16,), otype="cont", act="sigmoid"),
    _shape("edge_relu_b1", 1, "batch 1: the weight gradients' K = 1; dead units",
           Dobs=33, Denc=(31,), Dz=5, Ddec=(17,), otype="binary", act="relu"),
    _shape("k512_513", 33, "forward K = 513 into the latent layer (F_LATENT at 8 chunks in flight), output layer "
           "K = 512; backward K = 512 and 513",
           Dobs=21, Denc=(513,), Dz=3, Ddec=(512,), otype="cont", act="tanh"),
    _shape("batch_512", 512, "weight-gradient K = 512, the last size on the shallow loop",
           Dobs=24, Denc=(20,), Dz=4, Ddec=(18,), otype="binary", act="tanh"),
    _shape("batch_513", 513, "weight-gradient K = 513, the first size on the deep loop",
           Dobs=24, Denc=(20,), Dz=4, Ddec=(18,), otype="binary", act="tanh"),
    _shape("latent_deep_k", 20, "B_LATENT with K = 520", latents=("gauss",),
           Dobs=40, Denc=(24,), Dz=4, Ddec=(520,), otype="binary", act="tanh"),
]
SHAPE = {s.name: s for s in SHAPES}

# (shape name, latent, scaled) of every GPU case
CASES = [(s.name, lat, scaled) for s in SHAPES for lat in s.latents for scaled in (False, True)]
CASE_IDS = [f"{n}-{lat}-{'x30' if sc else 'theta0'}" for n, lat, sc in CASES]

MAX_SEEDS = 64


# ------------------------------------------------------------------ the two latents behind one face
def oracle(latent):
    return V if latent == "gauss" else A


def names(cfg, latent):
    return [n for n, _ in oracle(latent).param_shapes(cfg)]


def layer_inputs(cfg, latent):
    """{parameter name: width of its layer's input}."""
    out = {}
    for n, s in oracle(latent).param_shapes(cfg):
        if len(s) == 2:
            out[n] = s[0]
    for n in list(out):
        b = "b" + n[1:]
        out[b] = out[n]
    return out


def scale_params(cfg, params, latent):
    """Every layer x 30, a layer wider than WIDE at its input x 30 sqrt(WIDE / Kin)."""
    kin = layer_inputs(cfg, latent)
    out = []
    for n, p in zip(names(cfg, latent), params):
        f = SCALE * min(1.0, math.sqrt(WIDE / kin[n]))
        out.append((p * f).astype(np.float32))
    return out


def data_for(cfg, n, seed):
    rng = np.random.default_rng(seed)
    if cfg.otype == "binary":
        return (rng.random((n, cfg.Dobs)) < 0.3).astype(np.float32)
    return rng.beta(2.0, 2.0, size=(n, cfg.Dobs)).astype(np.float32)


def forward_backward(cfg, latent, params, X, eps, need_grad=True):
    """The latent's oracle on gathered rows X; the dtype of params is the dtype of the run."""
    if latent == "gauss":
        return V.forward_backward(params, X, eps, cfg, need_grad=need_grad)
    return A.forward_backward(params, X, cfg, need_grad=need_grad)


def value_of(out, latent, M):
    return (out["elbo"] if latent == "gauss" else out["loglik"]) / M


def hidden_preacts(cfg, latent, params, out):
    """The hidden layers' pre-activations of an oracle forward (from its stored activations)."""
    p = dict(zip(names(cfg, latent), params))
    pre = []
    for i in range(len(cfg.Denc)):
        pre.append(out["H"][i] @ p[f"Wenc{i}"] + p[f"benc{i}"])
    for i in range(len(cfg.Ddec)):
        pre.append(out["G"][i] @ p[f"Wdec{i}"] + p[f"bdec{i}"])
    return pre


def hidden_acts(out):
    return out["H"][1:] + out["G"][1:]


# ------------------------------------------------------------------ recovery and the criterion
def recover(theta0, theta1, acc1):
    """g = sign(theta' - theta) sqrt(acc') of a step taken from a zero accumulator (flat arrays)."""
    theta0, theta1, acc1 = (np.asarray(a, np.float64) for a in (theta0, theta1, acc1))
    return np.sign(theta1 - theta0) * np.sqrt(acc1)


def blocks(flat, shapes):
    out, o = {}, 0
    for n, s in shapes:
        k = int(np.prod(s))
        out[n] = np.asarray(flat[o:o + k], np.float64).reshape(s)
        o += k
    assert o == len(flat)
    return out


def block_errors(g, g64):
    """{block: max|g - g64| / max|g64|} of two {block: array} gradients."""
    return {n: float(np.abs(g[n] - g64[n]).max() / np.abs(g64[n]).max()) for n in g64}


def rejected(err, bound):
    """Blocks of err above their bound: the criterion of the GPU test."""
    return [n for n in err if not err[n] <= bound[n]]


def restated_step(cfg, latent, params, X, eps):
    """One float32 step of the oracle from a zero accumulator on gathered rows X:
    (value, theta' flat, acc' flat), every array float32 as on the device."""
    assert all(p.dtype == np.float32 for p in params)
    out = forward_backward(cfg, latent, params, X.astype(np.float32), None if eps is None else eps.astype(np.float32))
    acc = [np.zeros_like(p) for p in params]
    new_p, new_a = A.adagrad(params, acc, out["grads"], np.float32(cfg.eta))
    assert new_p[0].dtype == np.float32 and new_a[0].dtype == np.float32
    return value_of(out, latent, X.shape[0]), A.flatten(new_p), A.flatten(new_a)


@dataclasses.dataclass
class Step:
    """One step's inputs, its float64 oracle and the float32 restatement's error."""
    cfg: A.AEConfig
    latent: str
    seed: int
    Xtr: np.ndarray
    idx: np.ndarray
    eps: object                 # [M x Dz] float32 (Gaussian latent) or None
    params: list                # float32
    shapes: list
    out64: dict                 # the float64 oracle's forward / backward on Xtr[idx]
    value64: float
    g64: dict                   # {block: float64 gradient}
    restate: dict               # {block: error of the float32 restatement}
    bound: dict                 # {block: MARGIN x restate}
    restate_value: float

    def theta(self):
        return A.flatten(self.params)

    def device_errors(self, theta1, acc1):
        return block_errors(blocks(recover(self.theta(), theta1, acc1), self.shapes), self.g64)


def make_step(cfg, latent, params, Xtr, idx, eps, seed=0):
    """Oracle, restatement and bounds of one step on Xtr[idx] (eps: the Gaussian latent's noise)."""
    shapes = oracle(latent).param_shapes(cfg)
    X = Xtr[idx]
    p64 = [p.astype(np.float64) for p in params]
    out64 = forward_backward(cfg, latent, p64, X.astype(np.float64), None if eps is None else eps.astype(np.float64))
    g64 = dict(zip([n for n, _ in shapes], out64["grads"]))
    v32, th32, ac32 = restated_step(cfg, latent, params, X, eps)
    restate = block_errors(blocks(recover(A.flatten(params), th32, ac32), shapes), g64)
    value64 = value_of(out64, latent, len(idx))
    step = Step(cfg, latent, seed, Xtr, idx, eps, params, shapes, out64, value64, g64, restate,
                {n: MARGIN * e for n, e in restate.items()}, abs(v32 - value64) / abs(value64))
    for a in [Xtr, idx] + params + list(g64.values()) + ([eps] if eps is not None else []):
        a.setflags(write=False)
    return step


def draw(cfg, latent, B, scaled, seed):
    """params, Xtr, idx, eps of one seed: theta_0 from the latent's own init_params."""
    params = oracle(latent).init_params(cfg, seed=15485863 + seed)
    if scaled:
        params = scale_params(cfg, params, latent)
    Xtr = data_for(cfg, 2 * B + 16, seed)
    rng = np.random.default_rng(100 + seed)
    idx = rng.choice(Xtr.shape[0], size=B, replace=False).astype(np.int32)
    eps = rng.standard_normal((B, cfg.Dz)).astype(np.float32) if latent == "gauss" else None
    return params, Xtr, idx, eps


def off_theta0(cfg, out):
    """Some hidden unit where f' has left its theta_0 value and some output mean away from 1/2."""
    h = np.concatenate([a.ravel() for a in hidden_acts(out)])
    if cfg.act == "tanh":
        hid = bool((np.abs(h) > 0.9).any())
    elif cfg.act == "sigmoid":
        hid = bool(((h < 0.2) | (h > 0.8)).any())
    else:
        hid = True                                  # relu: the dead share, below
    return hid and bool(((out["Xpr"] < 0.2) | (out["Xpr"] > 0.8)).any())


def fair(cfg, latent, scaled, params, Xtr, idx, eps):
    """The conditions a seed has to meet (relu rows: the kink and the dead share; scaled weights:
    off_theta0)."""
    p64 = [p.astype(np.float64) for p in params]
    out = forward_backward(cfg, latent, p64, Xtr[idx].astype(np.float64),
                           None if eps is None else eps.astype(np.float64), need_grad=False)
    ok = True
    if cfg.act == "relu":
        pre = np.concatenate([a.ravel() for a in hidden_preacts(cfg, latent, p64, out)])
        ok = float(np.abs(pre).min()) >= KINK and 0.2 <= float((pre <= 0).mean()) <= 0.8
    return ok and (not scaled or off_theta0(cfg, out))


@functools.lru_cache(maxsize=None)
def case(name, latent, scaled, B=None):
    """The Step of one table case (B: another batch on the same shape and seed rule)."""
    sh = SHAPE[name]
    cfg = sh.cfg()
    B = sh.B if B is None else B
    for seed in range(MAX_SEEDS):
        params, Xtr, idx, eps = draw(cfg, latent, B, scaled, seed)
        if fair(cfg, latent, scaled, params, Xtr, idx, eps):
            return make_step(cfg, latent, params, Xtr, idx, eps, seed)
    raise AssertionError(f"{name}: no fair seed below {MAX_SEEDS}")


def table_line(label, err, bound, restate):
    """'label: worst block  device / restatement / bound' -- the block nearest to (or furthest past)
    its bound."""
    n = max(err, key=lambda k: err[k] / bound[k] if bound[k] > 0 else math.inf)
    return f"{label:38s} {n:8s} {err[n]:.1e} / {restate[n]:.1e} / {bound[n]:.1e}"
