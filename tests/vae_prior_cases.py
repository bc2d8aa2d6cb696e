"""Cases of the two-mode latent prior tests (tests/test_vae_prior_host.py, tests/test_gpu_vae_prior.py)
-- TEST HELPER ONLY: the case table, the inputs, and per case and form the float64 oracle
(tests/vae_prior_oracle.py), its float32 restatement and the per-block bounds, in the manner of
tests/ae_grad_cases.py, whose recovery (g = sign(theta' - theta) sqrt(acc') off a zero accumulator),
error measure, MARGIN = 16 and GRAD_CAP = 1e-4 are borrowed as they stand.

Shapes sit at the tile engine's edges: Dz of 1, 15, 16, 17, 33 (the latent's 16-column tiles and the
[M][ceil(Dz / 16)] partials), M of 1, 5, 33, one hidden layer of 12 to 40 units, Dobs 24 to 96, both
output types, K = 2 and 3 at M = 5 (B_LATENT_IW reads mu at stacked row g mod M), and one
784-500-20-500 case at B = 100.  Widths 0.5, 0.1, 0.05; one case has mean1 = 2.

Inputs.  theta_0 (N(0, 0.01)) x 10 per layer, x 10 sqrt(64 / Kin) for a layer wider than 64 at its
input; then bzmu = a u with u uniform on [-0.5, 1.5], so the posterior means cover both modes, the
valley between them and both outer flanks, and bzlv uniform on [-6, -1] (posterior widths 0.05 to
0.6: some samples stay beside their mean, some cross the valley).  tests/test_vae_prior_host.py
holds the conditions these inputs meet (the shares of r near 0, between and near 1; an element with
|t| > 100; every bound <= GRAD_CAP).  The seed of a case is the first at which the float32
restatement of its single step from acc = 1e-4 moves no element of theta' more than 1e-6 = a tenth
of check_theta's threshold from the float64 oracle's, in both forms: at width 0.05 (c = 400) a
gradient element of ~0.02 that is left over from terms of ~100 carries ~3e-4 of float32 error, and
|g| ~ sqrt(acc) is where an AdaGrad step is most sensitive; in a model of fewer than 10^4 parameters
check_theta allows no such element.  The 784-500-20-500 case has the seed, of 0 to 8, with the
fewest elements past that threshold in its importance-weighted form (7 of 815824, a share of 9e-6
against the 1e-4 allowed; the restatement's float32 log w ~ -580 carries ~3e-5 into the weights).
"""
import dataclasses
import functools
import math

import numpy as np

from oracle import ae_oracle as A
from tests import ae_grad_cases as G
from tests import vae_prior_oracle as PO
from tests import vae_stack_oracle as V

WSCALE = 10.0


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    kw: tuple               # AEConfig keyword items
    M: int
    K: int                  # samples of the importance-weighted step
    mean1: float
    width: float
    seed: int               # of the inputs (module docstring)

    def cfg(self):
        return A.AEConfig(**dict(self.kw))


def _case(name, M, K, mean1, width, seed, **kw):
    return Case(name, tuple(sorted(kw.items())), M, K, mean1, width, seed)


CASES = [
    _case("dz1_m5_bin", 5, 2, 1.0, 0.5, 0, Dobs=24, Denc=(12,), Dz=1, Ddec=(12,), otype="binary"),
    _case("dz15_m33_cont", 33, 2, 1.0, 0.1, 2, Dobs=37, Denc=(20,), Dz=15, Ddec=(24,), otype="cont"),
    _case("dz16_m1_bin", 1, 3, 1.0, 0.05, 1, Dobs=48, Denc=(24,), Dz=16, Ddec=(16,), otype="binary", act="sigmoid"),
    _case("dz17_m5_cont_a2", 5, 3, 2.0, 0.1, 3, Dobs=96, Denc=(40,), Dz=17, Ddec=(33,), otype="cont"),
    _case("dz33_m33_bin", 33, 2, 1.0, 0.05, 1, Dobs=64, Denc=(32,), Dz=33, Ddec=(40,), otype="binary", s2=2.0),
    _case("dz33_m5_cont_w05", 5, 2, 1.0, 0.5, 0, Dobs=40, Denc=(16,), Dz=33, Ddec=(17,), otype="cont"),
    _case("mnist_like", 100, 2, 1.0, 0.5, 6, Dobs=784, Denc=(500,), Dz=20, Ddec=(500,), otype="binary"),
]
CASE = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
STEPS = [(c.name, form) for c in CASES for form in PO.FORMS]
STEP_IDS = [f"{n}-{form}" for n, form in STEPS]


def scale_params(cfg, params):
    kin = G.layer_inputs(cfg, "gauss")
    return [(p * (WSCALE * min(1.0, math.sqrt(G.WIDE / kin[n])))).astype(np.float32)
            for n, p in zip(V.names(cfg), params)]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(cfg, Xtr, idx, params, {form: eps}) of a case: float32 arrays, read-only."""
    c = CASE[name]
    cfg = c.cfg()
    seed = c.seed
    params = scale_params(cfg, V.init_params(cfg, seed=15485863 + seed))
    rng = np.random.default_rng(1000 + seed)
    p = dict(zip(V.names(cfg), params))
    p["bzmu"][:] = (c.mean1 * rng.uniform(-0.5, 1.5, cfg.Dz)).astype(np.float32)
    p["bzlv"][:] = rng.uniform(-6.0, -1.0, cfg.Dz).astype(np.float32)
    Xtr = G.data_for(cfg, 2 * c.M + 16, seed)
    idx = rng.choice(Xtr.shape[0], size=c.M, replace=False).astype(np.int32)
    eps = {"elbo": rng.standard_normal((c.M, cfg.Dz)).astype(np.float32),
           "iw": rng.standard_normal((c.K, c.M, cfg.Dz)).astype(np.float32)}
    for a in [Xtr, idx] + params + list(eps.values()):
        a.setflags(write=False)
    return cfg, Xtr, idx, params, eps


def oracle(cfg, params, X, eps, mean1, width, form, dtype, **kw):
    return PO.forward_backward([q.astype(dtype) for q in params], X.astype(dtype), np.asarray(eps, dtype), cfg,
                               mean1, width, form, **kw)


def restated_step(cfg, params, X, eps, mean1, width, form, **kw):
    """One float32 step of the oracle from a zero accumulator: (value / M, theta' flat, acc' flat)."""
    out = oracle(cfg, params, X, eps, mean1, width, form, np.float32, **kw)
    acc = [np.zeros_like(q) for q in params]
    new_p, new_a = A.adagrad(params, acc, out["grads"], np.float32(cfg.eta))
    assert new_p[0].dtype == np.float32 and new_a[0].dtype == np.float32
    return out["value"] / X.shape[0], A.flatten(new_p), A.flatten(new_a)


def make_step(cfg, params, Xtr, idx, eps, mean1, width, form, seed=0):
    """A tests/ae_grad_cases.py Step (oracle, restatement, bounds) of one two-mode step."""
    shapes = V.param_shapes(cfg)
    X = Xtr[idx]
    out64 = oracle(cfg, params, X, eps, mean1, width, form, np.float64)
    g64 = dict(zip([n for n, _ in shapes], out64["grads"]))
    v32, th32, ac32 = restated_step(cfg, params, X, eps, mean1, width, form)
    restate = G.block_errors(G.blocks(G.recover(A.flatten(params), th32, ac32), shapes), g64)
    value64 = out64["value"] / len(idx)
    return G.Step(cfg, "gauss", seed, Xtr, idx, eps, params, shapes, out64, value64, g64, restate,
                  {n: G.MARGIN * e for n, e in restate.items()}, abs(v32 - value64) / abs(value64))


@functools.lru_cache(maxsize=None)
def step(name, form):
    cfg, Xtr, idx, params, eps = inputs(name)
    c = CASE[name]
    return make_step(cfg, params, Xtr, idx, eps[form], c.mean1, c.width, form, c.seed)


def acc0(params):
    """The single-step tests' accumulator (tests/test_gpu_ae.py: 1e-4 everywhere)."""
    return [np.full(q.shape, 1e-4, np.float32) for q in params]


def step64(cfg, Xtr, params, acc, idx, eps, mean1, width, form, Xenc=None):
    """The float64 oracle's train(idx): (value / M, theta', acc', aux)."""
    return PO.train_step([q.astype(np.float64) for q in params], [a.astype(np.float64) for a in acc],
                         Xtr.astype(np.float64), idx, np.asarray(eps, np.float64), cfg, mean1, width, form,
                         Xenc=None if Xenc is None else np.asarray(Xenc, np.float64))
