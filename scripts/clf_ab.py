#!/usr/bin/env python
"""Softmax MLP classifier: the evidence lines under profiles/classifier/.

    python scripts/clf_ab.py digests [out]   vaeb_ae steps under every rule and latent, this build against another
    python scripts/clf_ab.py time [out]      classifier train_many us per step, MAP against dropout
    python scripts/clf_ab.py profile         one dropout run for a kernel trace (rocprofv3 --kernel-trace --stats)

The other build is vaeb_amd/libvaeb_hip_<VAEB_AB_OTHER>.so (default "parent"), loaded as in
scripts/prior_ab.py.

digests: a 5-step train_many (partial last batch) of a 96-(40, 24)-17-(24, 40) autoencoder per latent
(point, gauss, act) and update rule on each build; a line per (build, latent, rule) with SHA-256 digests
of theta, both state slots and the values, then `identical=` per pair.
time: Din 784, Dout 10, batch 100 at Dh = [1000, 1000] (mlp.py:435) and [500, 300] (mlp.py:440), AdaGrad,
one warm-up round and four timed rounds of 600 steps per variant (2400 timed steps), MAP and dropout at
keep 0.5 alternating.  The dropout step's yardstick is the MAP step of the same build and shape; next to
the difference stand the bytes its mask pass moves (theta read, theta~ and the byte mask written, the
byte mask read again by the weight gradients).
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from prior_ab import OTHER_NAME, THIS, emit, other_lib, sha   # noqa: E402

RULES = {"adagrad": None, "sga": ("sga", 1e-3, 0.9), "adadelta": ("adadelta", 1.0, 0.95), "adam": ("adam", 1e-3, 0.9, 0.999)}


# ------------------------------------------------------------------ digests
def ae_sequence(L, latent, rule):
    rng = np.random.default_rng(5)
    Dobs, n, B = 96, 150, 32
    X = (rng.random((n, Dobs)) < 0.3).astype(np.float32)
    ctx = L.AEContext(Dobs, (40, 24), 17, (24, 40), otype="binary", max_batch=B, latent=latent)
    try:
        ctx.set_data(X)
        ctx.set_params((0.1 * rng.standard_normal(ctx.P)).astype(np.float32))
        if latent == "gauss":
            ctx.set_eps_mode(L.EPS_PHILOX, 10)
            ctx.set_step(3)
        if RULES[rule]:
            ctx.set_optimizer(*RULES[rule])
        vals = ctx.train_many(rng.permutation(n).astype(np.int32), B)   # 32, 32, 32, 32, 22
        two = L.AE_RULE_SLOTS[rule] == 2
        return dict(theta=sha(ctx.get_params()), s0=sha(ctx.get_opt_state(0)), s1=sha(ctx.get_opt_state(1)) if two else None,
                    values=sha(vals), steps=len(vals), last_value=float(vals[-1]))
    finally:
        ctx.close()


def digests(out):
    libs = {"this": THIS, OTHER_NAME: other_lib()}
    ok = True
    for latent in ("point", "gauss", "act"):
        for rule in RULES:
            res = {}
            for name, L in libs.items():
                res[name] = ae_sequence(L, latent, rule)
                emit(out, dict(build=name, latent=latent, rule=rule, **res[name]))
            same = res["this"] == res[OTHER_NAME]
            ok = ok and same
            emit(out, dict(latent=latent, rule=rule, identical=same))
    return 0 if ok else 1


# ------------------------------------------------------------------ time
SHAPES = {"784-1000-1000-10": (1000, 1000), "784-500-300-10": (500, 300)}
STEPS = 600


def clf_ctx(Dh, dropout):
    rng = np.random.default_rng(3)
    n = 6000
    X = rng.random((n, 784)).astype(np.float32)
    Y = np.zeros((n, 10), np.float32)
    Y[np.arange(n), rng.integers(0, 10, n)] = 1.0
    ctx = THIS.CLFContext(784, Dh, 10, eta=0.01, max_batch=100, dropout=dropout, keep=0.5)
    ctx.set_data(X, Y)
    ctx.set_params((0.01 * rng.standard_normal(ctx.P)).astype(np.float32))
    ctx.set_seed(15485863)
    idx = np.concatenate([rng.permutation(n) for _ in range(STEPS // 60)]).astype(np.int32)
    return ctx, idx


def timings(out):
    for shape, Dh in SHAPES.items():
        ctxs = [("map",) + clf_ctx(Dh, False), ("dropout_keep_0.5",) + clf_ctx(Dh, True)]
        us = {name: [] for name, _, _ in ctxs}
        for rnd in range(5):                       # round 0 warms up
            for name, ctx, idx in ctxs:
                t0 = time.perf_counter()
                v = ctx.train_many(idx, 100)
                dt = time.perf_counter() - t0
                assert len(v) == STEPS and np.isfinite(v).all()
                if rnd:
                    us[name].append(round(dt / STEPS * 1e6, 3))
        P = ctxs[0][1].P
        for _, ctx, _ in ctxs:
            ctx.close()
        med = {k: float(np.median(v)) for k, v in us.items()}
        for k in us:
            emit(out, dict(shape=shape, variant=k, us_per_step=us[k], median=med[k], timed_steps=4 * STEPS))
        launches = len(Dh) + 1
        emit(out, dict(shape=shape, params=P, dropout_minus_map_us=round(med["dropout_keep_0.5"] - med["map"], 3),
                       map_spread_us=round(max(us["map"]) - min(us["map"]), 3),
                       mask_pass_bytes=9 * P, mask_bytes_reread_by_wgrad=P, extra_launches_per_step=1,
                       launches_per_map_step=3 * launches + 1))
    return 0


def profile(_):
    ctx, idx = clf_ctx((1000, 1000), True)
    ctx.train_many(idx[:200 * 100], 100)
    ctx.close()
    return 0


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    fh = open(sys.argv[2], "w") if len(sys.argv) > 2 else None
    fn = {"digests": digests, "time": timings, "profile": profile}.get(mode)
    if fn is None:
        sys.exit(__doc__)
    sys.exit(fn(fh))
