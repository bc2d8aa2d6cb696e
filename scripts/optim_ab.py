#!/usr/bin/env python
"""Update rules of the layer-stack engine: the evidence lines under profiles/optimizers/.

    python scripts/optim_ab.py digests [out]   default-AdaGrad contexts, this build against another
    python scripts/optim_ab.py time [out]      train_many us per step per rule, the two builds alternating
    python scripts/optim_ab.py learn [out]     marginal_ll by epoch under each of the four rules

The other build is vaeb_amd/libvaeb_hip_<VAEB_AB_OTHER>.so (default "parent": the library of the
parent commit, built there with __graft_entry__.build() and copied under that name).  Both
libraries are loaded into this one process: vaeb_amd/_lib.py a second time under another module name
with VAEB_LIB_VARIANT set while it loads.

digests: the sequence of scripts/prior_ab.py -- one 16-step sequence per model (point, Gaussian ELBO,
iw_samples = 3, MASK-corrupting Gaussian) at 96-(40, 24)-17-(24, 40) on each build, the update rule
left at its default; a line per (build, model) with SHA-256 digests of theta, the accumulator and the
per-step values, then `identical=` per model.
time: 784-(500)-20-(500), binary, B = 100, train_many over 600 steps, one warm-up round and five
timed rounds of: other build, this build AdaGrad, SGA, AdaDelta, Adam, other build again.  The last
against the first is the spread the other build shows against itself.
learn: ConstructVAE 196-128-16-128 on the 4000 synthetic rows of prior_ab.py learn, 60 epochs of 40
steps under AdaGrad(0.01), Adam(1e-3), AdaDelta() and GradientAscent(1e-3, 0.9); marginal_ll (K = 16)
per row by epoch.  An observation, no pass mark.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from prior_ab import MODELS, OTHER_NAME, THIS, emit, other_lib, sequence   # noqa: E402


# ------------------------------------------------------------------ digests
def digests(out):
    libs = {"this": THIS, OTHER_NAME: other_lib()}
    res = {}
    for model, kw in MODELS.items():
        for name, L in libs.items():
            res[model, name] = sequence(L, kw)
            emit(out, dict(build=name, model=model, rule="adagrad (default)", **res[model, name]))
    ok = True
    for model in MODELS:
        same = res[model, "this"] == res[model, OTHER_NAME]
        ok = ok and same
        emit(out, dict(model=model, identical=same))
    return 0 if ok else 1


# ------------------------------------------------------------------ time
RULES = {"sga": ("sga", 1e-3, 0.9), "adadelta": ("adadelta", 1.0, 0.95), "adam": ("adam", 1e-3, 0.9, 0.999)}


def timed_ctx(L, rule):
    rng = np.random.default_rng(3)
    n = 6000
    X = (rng.random((n, 784)) < 0.3).astype(np.float32)
    ctx = L.AEContext(784, (500,), 20, (500,), otype="binary", max_batch=100, latent="gauss")
    ctx.set_data(X)
    ctx.set_params((0.01 * rng.standard_normal(ctx.P)).astype(np.float32))
    ctx.set_eps_mode(L.EPS_PHILOX, 10)
    if rule:
        ctx.set_optimizer(*RULES[rule])
    idx = np.concatenate([rng.permutation(n) for _ in range(10)]).astype(np.int32)   # 600 steps of 100
    return ctx, idx


def timings(out):
    O = other_lib()
    cfgs = [("a_other_adagrad", O, None), ("b_this_adagrad", THIS, None), ("c_this_sga", THIS, "sga"),
            ("d_this_adadelta", THIS, "adadelta"), ("e_this_adam", THIS, "adam"), ("f_other_adagrad_again", O, None)]
    ctxs = [(name,) + timed_ctx(L, rule) for name, L, rule in cfgs]
    us = {name: [] for name, _, _ in ctxs}
    for rnd in range(6):                       # round 0 warms up
        for name, ctx, idx in ctxs:
            t0 = time.perf_counter()
            ctx.train_many(idx, 100)
            dt = time.perf_counter() - t0
            if rnd:
                us[name].append(round(dt / 600 * 1e6, 3))
    params = ctxs[0][1].P
    for name, ctx, _ in ctxs:
        ctx.close()
    med = {k: float(np.median(v)) for k, v in us.items()}
    for k in us:
        emit(out, dict(config=k, other=OTHER_NAME, us_per_step=us[k], median=med[k], steps_per_round=600))
    emit(out, dict(params=params, extra_state_bytes_per_step_two_slot=8 * params,
                   other_against_itself=round(med["f_other_adagrad_again"] - med["a_other_adagrad"], 3),
                   this_adagrad_minus_other=round(med["b_this_adagrad"] - med["a_other_adagrad"], 3),
                   sga_minus_adagrad=round(med["c_this_sga"] - med["b_this_adagrad"], 3),
                   adadelta_minus_adagrad=round(med["d_this_adadelta"] - med["b_this_adagrad"], 3),
                   adam_minus_adagrad=round(med["e_this_adam"] - med["b_this_adagrad"], 3)))
    return 0


# ------------------------------------------------------------------ learn
def learn(out):
    from vaeb_amd import ae
    from vaeb_amd.infalg import AdaDelta, AdaGrad, Adam, GradientAscent
    rng = np.random.default_rng(0)
    nbits, D, n = 8, 196, 4000                 # the rows of prior_ab.py learn
    patterns = rng.random((nbits, D)) < 0.15
    bits = rng.random((n, nbits)) < 0.5
    p = 0.05 + 0.9 * (1 - np.prod(1 - bits[:, :, None] * patterns[None], axis=1))
    X = (rng.random((n, D)) < p).astype(np.float32)
    rules = [("adagrad_0.01", lambda: AdaGrad(0.01)), ("adam_1e-3", lambda: Adam(1e-3)), ("adadelta", lambda: AdaDelta()),
             ("sga_1e-3_mu0.9", lambda: GradientAscent(1e-3, 0.9))]
    for name, make in rules:
        np.random.seed(15485863)               # the same theta_0 and permutations under every rule
        train, *_ = ae.ConstructVAE(X, Denc=[128], Dz=16, Ddec=[128], max_batch=1000, inf=make())
        curve = [round(train.marginal_ll(X, 16) / n, 3)]
        for _ in range(60):
            ae.train_epochs(train, n, 1, batch_size=100, verbose=False)
            curve.append(round(train.marginal_ll(X, 16) / n, 3))
        emit(out, dict(rule=name, optimizer=list(train.optimizer), steps=train.ctx.get_opt_step(),
                       marginal_ll_per_row_by_epoch=curve))
        train.ctx.close()
    return 0


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    fh = open(sys.argv[2], "w") if len(sys.argv) > 2 else None
    fn = {"digests": digests, "time": timings, "learn": learn}.get(mode)
    if fn is None:
        sys.exit(__doc__)
    sys.exit(fn(fh))
