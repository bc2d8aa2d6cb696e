"""The deferred dW2 (| dW6) tiling (engine_f32.inc w2_plan, latent.hpp enc_latent16_w2_kernel): one
tile worker per workgroup at the planned width, dispatched ahead of the encoder rows, against
the in-step dW2 (VAEB_DW2_DEFER=0, 32-wide tiles in the dhd launch) and the paired 32-wide form
(VAEB_DW2_PAIRED=1): bit for bit, because no form changes the order in which an output element's
K chunks are summed.  Shapes: the smallest at which the step defers its dW2 at L = 1 (latent
fan-in ceil(H / 16) > 16), B = 36 (three row blocks, the last partial); D = 50 takes the scalar
loads, the Gaussian 56-272 has its [W2 | W6] boundary inside a tile, 784-319 / 784-320 have the
bias row last in a tile / alone in one.  Two more cases reach the 48- and 64-wide tiles, which
the plan only picks next to a large encoder grid (784-500 at B = 100 and B = 132).

Against the float64 oracle on the oracle's Philox draw, the trajectory tolerances of
tests/test_gpu_step.py: ELBO 1e-3 relative, theta 5e-3 absolute."""
import functools

import numpy as np
import pytest

from oracle import philox as P
from oracle import vaeb_oracle as O

pytestmark = pytest.mark.gpu

SEED = 10
ORDER = np.array([1, 0, 2, 1, 0, 2], np.int32)   # update_many(3), a sync update, update_many(2)
# (name, config, B, planned width)
CASES = [
    ("d104", dict(D=104, H=272, Z=4), 36, 32),
    ("d50_scalar", dict(D=50, H=272, Z=4), 36, 32),
    ("gauss56", dict(D=56, H=272, Z=2, continuous=True), 36, 32),
    ("h319", dict(D=784, H=319, Z=20), 36, 32),
    ("h320", dict(D=784, H=320, Z=20), 36, 32),
    ("mnist_w48", dict(D=784, H=500, Z=20), 100, 48),
    ("mnist_w64", dict(D=784, H=500, Z=20), 132, 64),
]
# (VAEB_DW2_DEFER, VAEB_DW2_PAIRED)
MODES = {"tiles": ("1", "0"), "in_step": ("0", "0"), "paired": ("1", "1")}


def data_for(cfg, n):
    return O.synthetic_frey(n=n, D=cfg.D, seed=0) if cfg.continuous else O.synthetic_mnist(n=n, D=cfg.D, seed=0)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle's trajectory over ORDER (float64): per-step ELBOs and the final theta."""
    _, kw, B, _ = next(c for c in CASES if c[0] == name)
    cfg = O.Config(**kw)
    x = data_for(cfg, 3 * B)
    p = [q.astype(np.float64) for q in O.init_params(cfg)]
    a = [np.zeros_like(q) for q in p]
    elbos = []
    for t, b in enumerate(ORDER):
        eps = P.train_eps(SEED, t, int(b), B, B, 0, 1, cfg.Z)
        e, p, a, _ = O.step(p, a, x[b * B:(b + 1) * B].astype(np.float64), eps, cfg)
        elbos.append(e)
    return elbos, O.flatten(p)


def run(cfg, B, x, mode, use_graph, monkeypatch):
    from vaeb_amd import _lib
    monkeypatch.setenv("VAEB_DW2_DEFER", MODES[mode][0])
    monkeypatch.setenv("VAEB_DW2_PAIRED", MODES[mode][1])
    ctx = _lib.Context(cfg.D, cfg.H, cfg.Z, B, decoder=int(cfg.continuous), max_eval_rows=B, use_graph=use_graph)
    ctx.set_data(x)
    ctx.set_params(O.flatten(O.init_params(cfg)))
    ctx.set_eps_mode(_lib.EPS_PHILOX, SEED)
    ctx.set_step(0)
    out = []
    ctx.update_many(ORDER[:3])
    out.append(ctx.get_params())                  # flush of the third step's pending dW2
    out.append(ctx.update(int(ORDER[3])))         # a synchronous step after a flush
    ctx.update_many(ORDER[4:])                    # (the first of them with a pending dW2)
    out.append(ctx.get_params())
    out.append(ctx.get_adagrad_state())
    out.append(ctx.epoch_elbo()[0])
    slots = [n for n, _ in ctx.profile_steps(1)]
    ctx.close()
    return out, slots


@pytest.mark.parametrize("name,kw,B,width", CASES, ids=[c[0] for c in CASES])
def test_tile_forms_agree_bitwise_and_track_the_oracle(name, kw, B, width, monkeypatch):
    from vaeb_amd import _lib
    cfg = O.Config(**kw)
    pl = _lib.dw2_plan(cfg.D, cfg.H, cfg.Z, B, decoder=int(cfg.continuous))
    assert (pl["width"], pl["paired"]) == (width, False)
    x = data_for(cfg, 3 * B)
    res = {}
    for mode in MODES:
        for use_graph in (True, False):
            out, slots = run(cfg, B, x, mode, use_graph, monkeypatch)
            # the deferred launch actually ran (or, in-step, did not)
            assert ("p1_enc_latent_w2" in slots) == (mode != "in_step"), (mode, slots)
            res[mode, use_graph] = out
    ref = res["in_step", True]
    for key, out in res.items():
        for i, (a, b) in enumerate(zip(out, ref)):
            assert np.array_equal(np.asarray(a), np.asarray(b)), (key, i)
    elbos, theta = reference(name)
    got = res["tiles", True]
    assert abs(got[1] - elbos[3]) <= 1e-3 * abs(elbos[3]), (got[1], elbos[3])
    assert np.abs(got[2] - theta).max() <= 5e-3
