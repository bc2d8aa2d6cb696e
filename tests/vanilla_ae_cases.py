"""Case table and inputs of the vanilla-autoencoder step tests -- TEST HELPER ONLY, shared by
tests/test_vanilla_ae_host.py (no GPU) and tests/test_gpu_vanilla_ae.py.

The shapes are six of tests/ae_grad_cases.py (the tile engine's edges, K = 512 / 513 and batches of
512 / 513) with the otype and the latent swapped; recovery (recover), the per-block error
(block_errors), the bound (MARGIN = 16 x the float32 restatement's error), VALUE_RTOL and GRAD_CAP
are that file's.  The oracle is tests/vanilla_ae_oracle.py.

Inputs.  theta_0 from seed 7 on (init_params), unscaled or through scale_params(.., "point"); data
rows and the gathered idx as in ae_grad_cases.draw.  The seed of a case is the first one from 7 that
is fair (fair()): relu rows have no float64 hidden or latent pre-activation within KINK of 0 and
20 % to 80 % dead units, the latent layer included; at scaled weights the code has left the range
where f' is flat (tanh: some |Z| > 0.9, sigmoid: some Z outside [0.3, 0.7]) and some output is
outside [0.2, 0.8].  No condition looks at a gradient or at the device.
"""
import dataclasses
import functools

import numpy as np

from tests import ae_grad_cases as G
from tests import vanilla_ae_oracle as VA

SHAPE_NAMES = ["edge_bin_tanh", "edge_cont_sigmoid", "edge_relu_b1", "k512_513", "batch_512", "batch_513"]
FIRST_SEED = 7

# (shape, latent, otype, scaled)
CASES = [(n, "act", "se", sc) for n in SHAPE_NAMES for sc in (False, True)]
CASES += [("edge_bin_tanh", "act", "binary", sc) for sc in (False, True)]
CASES += [("edge_cont_sigmoid", "act", "cont", sc) for sc in (False, True)]
CASES += [("edge_bin_tanh", "point", "se", sc) for sc in (False, True)]
CASE_IDS = [f"{n}-{lat}-{ot}-{'x30' if sc else 'theta0'}" for n, lat, ot, sc in CASES]


def cfg_of(name, otype):
    return dataclasses.replace(G.SHAPE[name].cfg(), otype=otype)


def data_for(cfg, n, seed):
    """Bernoulli(0.3) rows for the binary output, Beta(2, 2) rows otherwise (ae_grad_cases.data_for)."""
    rng = np.random.default_rng(seed)
    if cfg.otype == "binary":
        return (rng.random((n, cfg.Dobs)) < 0.3).astype(np.float32)
    return rng.beta(2.0, 2.0, size=(n, cfg.Dobs)).astype(np.float32)


def scale(cfg, params):
    return G.scale_params(VA.layout(cfg), params, "point")


def draw(cfg, B, scaled, seed):
    params = VA.init_params(cfg, seed=seed)
    if scaled:
        params = scale(cfg, params)
    Xtr = data_for(cfg, 2 * B + 16, seed)
    idx = np.random.default_rng(100 + seed).choice(Xtr.shape[0], size=B, replace=False).astype(np.int32)
    return params, Xtr, idx


def preacts(cfg, latent, params, out):
    """Pre-activations of every unit that goes through f: the hidden layers, and the latent's
    under latent "act"."""
    pre = G.hidden_preacts(VA.layout(cfg), "point", params, out)
    return pre + ([out["Zpre"]] if latent == "act" else [])


def code_off_flat(cfg, Z):
    """f'(Z) matters: the code has left the range where f' is (nearly) constant."""
    if cfg.act == "tanh":
        return bool((np.abs(Z) > 0.9).any())
    if cfg.act == "sigmoid":
        return bool(((Z < 0.3) | (Z > 0.7)).any())
    return True                                         # relu: the dead share


def fair(cfg, latent, scaled, params, Xtr, idx):
    p64 = [p.astype(np.float64) for p in params]
    out = VA.forward_backward(p64, Xtr[idx].astype(np.float64), cfg, latent, need_grad=False)
    ok = True
    if cfg.act == "relu":
        pre = np.concatenate([a.ravel() for a in preacts(cfg, latent, p64, out)])
        ok = float(np.abs(pre).min()) >= G.KINK and 0.2 <= float((pre <= 0).mean()) <= 0.8
    if scaled:
        ok = ok and (latent != "act" or code_off_flat(cfg, out["Z"]))
        ok = ok and bool(((out["Xpr"] < 0.2) | (out["Xpr"] > 0.8)).any())
    return ok


def restated_step(cfg, latent, params, X):
    """One float32 step of the oracle from a zero accumulator: (value / M, theta' flat, acc' flat)."""
    assert all(p.dtype == np.float32 for p in params)
    out = VA.forward_backward(params, X.astype(np.float32), cfg, latent)
    new_p, new_a = VA.adagrad(params, [np.zeros_like(p) for p in params], out["grads"], np.float32(cfg.eta))
    assert new_p[0].dtype == np.float32 and new_a[0].dtype == np.float32
    return out["value"] / X.shape[0], G.A.flatten(new_p), G.A.flatten(new_a)


def make_step(cfg, latent, params, Xtr, idx, seed=0):
    """Oracle, restatement and bounds of one step on Xtr[idx], as ae_grad_cases.make_step."""
    shapes = VA.param_shapes(cfg)
    X = Xtr[idx]
    out64 = VA.forward_backward([p.astype(np.float64) for p in params], X.astype(np.float64), cfg, latent)
    g64 = dict(zip(VA.names(cfg), out64["grads"]))
    v32, th32, ac32 = restated_step(cfg, latent, params, X)
    restate = G.block_errors(G.blocks(G.recover(G.A.flatten(params), th32, ac32), shapes), g64)
    value64 = out64["value"] / len(idx)
    step = G.Step(cfg, latent, seed, Xtr, idx, None, params, shapes, out64, value64, g64, restate,
                  {n: G.MARGIN * e for n, e in restate.items()}, abs(v32 - value64) / abs(value64))
    for a in [Xtr, idx] + params + list(g64.values()):
        a.setflags(write=False)
    return step


@functools.lru_cache(maxsize=None)
def case(name, latent, otype, scaled, B=None):
    cfg = cfg_of(name, otype)
    B = G.SHAPE[name].B if B is None else B
    for seed in range(FIRST_SEED, FIRST_SEED + G.MAX_SEEDS):
        params, Xtr, idx = draw(cfg, B, scaled, seed)
        if fair(cfg, latent, scaled, params, Xtr, idx):
            return make_step(cfg, latent, params, Xtr, idx, seed)
    raise AssertionError(f"{name}: no fair seed from {FIRST_SEED}")
