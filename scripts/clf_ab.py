#!/usr/bin/env python
"""Layer-stack engine, this build against another: the evidence lines under
profiles/classifier/ and profiles/stack_core/.

    python scripts/clf_ab.py digests [out]   vaeb_ae and vaeb_clf sequences, this build against another
    python scripts/clf_ab.py time [out]      classifier train_many us per step, MAP against dropout
    python scripts/clf_ab.py time_ab [out]   train_many us per step, the two builds alternating
    python scripts/clf_ab.py profile         one dropout run for a kernel trace (rocprofv3 --kernel-trace --stats)

The other build is vaeb_amd/libvaeb_hip_<VAEB_AB_OTHER>.so (default "parent"), loaded as in
scripts/prior_ab.py.

digests: SHA-256 digests per (build, sequence), then `identical=` per pair.  Autoencoders: a 5-step
train_many (n = 150, batch 32: a 22-row last batch) of a 96-(40, 24)-17-(24, 40) net per latent (point,
gauss, act) and update rule, and under AdaGrad and Adam a cont output, the squared-error output on the
activated latent, iw_samples = 3 (max_batch 96), the two-mode prior and mask corruption at 0.3: theta, both
state slots, the values, and over all 150 rows the chunked calls the context has (reconstruct, sq_error;
Gaussian latent: elbo, marginal_ll at K = 5; two-mode: encode_bits).  Classifiers: 96-(40, 24)-17 (P % 4 = 1)
on one-hot rows, {MAP, dropout keep 0.5} x {bernoulli, categorical} x rule, every other one with the prior:
theta, the slots, the values, predict (dropout: also 3 draws), loglik, accuracy.
time: Din 784, Dout 10, batch 100 at Dh = [1000, 1000] (mlp.py:435) and [500, 300] (mlp.py:440), AdaGrad,
one warm-up round and four timed rounds of 600 steps per variant (2400 timed steps), MAP and dropout at
keep 0.5 alternating.  The dropout step's yardstick is the MAP step of the same build and shape; next to
the difference stand the bytes its mask pass moves (theta read, theta~ and the byte mask written, the
byte mask read again by the weight gradients).
time_ab: the same rounds on the classifier 784-500-300-10 (MAP, dropout keep 0.5) and the Gaussian
autoencoder 784-(500)-20-(500) (AdaGrad, Adam), batch 100.  Which of two live contexts was created second
moves a step by up to 0.5 us whatever the build (a library against its own copy shows it), more than a
context's own rounds differ, so each of the four rounds creates a fresh pair, the build that is created and
run first changing from round to round, warms both up with one call and times the next; this
build's median is held to the other's median plus the other's own max - min over its four rounds.
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
AE_EXTRA = {
    "cont": dict(otype="cont"),
    "se_act": dict(otype="se", latent="act"),
    "gauss_iw3": dict(latent="gauss", iw_samples=3, max_batch=96),
    "gauss_twomode": dict(latent="gauss", prior="twomode"),
    "gauss_mask": dict(latent="gauss", corruption="mask"),
}


def set_rule(ctx, rule):
    if RULES[rule]:
        ctx.set_optimizer(*RULES[rule])


def state(L, ctx, rule, vals):
    two = L.AE_RULE_SLOTS[rule] == 2
    return dict(theta=sha(ctx.get_params()), s0=sha(ctx.get_opt_state(0)), s1=sha(ctx.get_opt_state(1)) if two else None,
                values=sha(vals), steps=len(vals), last_value=float(vals[-1]))


def ae_sequence(L, rule, **kw):
    rng = np.random.default_rng(5)
    Dobs, n, B = 96, 150, 32
    kw = dict(dict(otype="binary", latent="point", max_batch=B), **kw)
    X = rng.random((n, Dobs)).astype(np.float32)
    if kw["otype"] == "binary":
        X = (X < 0.3).astype(np.float32)
    ctx = L.AEContext(Dobs, (40, 24), 17, (24, 40), **kw)
    try:
        gauss = kw["latent"] == "gauss"
        ctx.set_data(X)
        ctx.set_params((0.1 * rng.standard_normal(ctx.P)).astype(np.float32))
        if gauss:
            ctx.set_eps_mode(L.EPS_PHILOX, 10)
            ctx.set_step(3)
        if kw.get("corruption"):
            ctx.set_corruption_noise(L.EPS_PHILOX, 11)
            ctx.set_corruption_level(0.3)
        set_rule(ctx, rule)
        vals = ctx.train_many(rng.permutation(n).astype(np.int32), B)   # 32, 32, 32, 32, 22
        res = state(L, ctx, rule, vals)
        sq, sq_rows = ctx.sq_error(X, rows=True)                        # five chunks, the last of 22 rows
        res.update(reconstruct=sha(ctx.reconstruct(X)), sq_error=sq, sq_rows=sha(sq_rows))
        if gauss:
            ll, ll_rows = ctx.marginal_ll(X, 5, rows=True)
            res.update(elbo=ctx.elbo(X), marginal_ll=ll, marginal_ll_rows=sha(ll_rows))
        if kw.get("prior") == "twomode":
            res.update(bits=sha(ctx.encode_bits(X)))
        return res
    finally:
        ctx.close()


def clf_sequence(L, rule, dropout, loss, prior):
    rng = np.random.default_rng(7)
    Din, Dout, n, B = 96, 17, 150, 32
    X = rng.random((n, Din)).astype(np.float32)
    Y = np.zeros((n, Dout), np.float32)
    Y[np.arange(n), rng.integers(0, Dout, n)] = 1.0
    ctx = L.CLFContext(Din, (40, 24), Dout, loss=loss, prior=prior, s2=2.0, max_batch=B, dropout=dropout, keep=0.5)
    try:
        ctx.set_data(X, Y)
        ctx.set_params((0.1 * rng.standard_normal(ctx.P)).astype(np.float32))
        ctx.set_seed(15485863)
        ctx.set_step(3)
        set_rule(ctx, rule)
        vals = ctx.train_many(rng.permutation(n).astype(np.int32), B)
        res = state(L, ctx, rule, vals)
        res.update(predict=sha(ctx.predict(X)), loglik=ctx.loglik(X, Y), accuracy=ctx.accuracy(X, Y))
        if dropout:
            res.update(predict3=sha(ctx.predict(X, draws=3)), loglik_draw=ctx.loglik(X, Y, draw=1),
                       accuracy3=ctx.accuracy(X, Y, draws=3))
        return res
    finally:
        ctx.close()


def digests(out):
    libs = {"this": THIS, OTHER_NAME: other_lib()}
    seqs = [(dict(kind="ae", latent=latent, rule=rule), ae_sequence, dict(latent=latent))
            for latent in ("point", "gauss", "act") for rule in RULES]
    seqs += [(dict(kind="ae", model=model, rule=rule), ae_sequence, kw)
             for model, kw in AE_EXTRA.items() for rule in ("adagrad", "adam")]
    for i, (dropout, loss, rule) in enumerate((d, l, r) for d in (False, True) for l in ("bernoulli", "categorical")
                                              for r in RULES):
        kw = dict(dropout=dropout, loss=loss, prior=bin(i).count("1") % 2 == 1)   # each rule, loss and mode with both
        seqs.append((dict(kind="clf", rule=rule, **kw), clf_sequence, kw))
    ok = True
    for tag, fn, kw in seqs:
        res = {name: fn(L, tag["rule"], **kw) for name, L in libs.items()}
        for name in libs:
            emit(out, dict(build=name, **tag, **res[name]))
        same = res["this"] == res[OTHER_NAME]
        ok = ok and same
        emit(out, dict(**tag, identical=same))
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


def ab_ctx(L, kind, variant):
    rng = np.random.default_rng(3)
    n = 6000
    if kind == "clf":
        X = rng.random((n, 784)).astype(np.float32)
        Y = np.zeros((n, 10), np.float32)
        Y[np.arange(n), rng.integers(0, 10, n)] = 1.0
        ctx = L.CLFContext(784, (500, 300), 10, eta=0.01, max_batch=100, dropout=variant == "dropout_keep_0.5", keep=0.5)
        ctx.set_data(X, Y)
        ctx.set_seed(15485863)
    else:
        ctx = L.AEContext(784, (500,), 20, (500,), otype="binary", max_batch=100, latent="gauss")
        ctx.set_data((rng.random((n, 784)) < 0.3).astype(np.float32))
        ctx.set_eps_mode(L.EPS_PHILOX, 10)
        set_rule(ctx, variant)
    ctx.set_params((0.01 * rng.standard_normal(ctx.P)).astype(np.float32))
    idx = np.concatenate([rng.permutation(n) for _ in range(STEPS // 60)]).astype(np.int32)
    return ctx, idx


def timings_ab(out):
    libs = {OTHER_NAME: other_lib(), "this": THIS}
    ok = True
    for kind, shape, variants in (("clf", "784-500-300-10", ("map", "dropout_keep_0.5")),
                                  ("ae", "784-(500)-20-(500) gauss", ("adagrad", "adam"))):
        for variant in variants:
            us, first = {name: [] for name in libs}, []
            for rnd in range(4):                   # a fresh pair of contexts per round; even rounds the other build first
                order = list(libs.items())[::1 if rnd % 2 == 0 else -1]
                ctxs = [(name,) + ab_ctx(L, kind, variant) for name, L in order]
                first.append(order[0][0])
                for timed in (False, True):        # each context's first call warms up
                    for name, ctx, idx in ctxs:
                        t0 = time.perf_counter()
                        v = ctx.train_many(idx, 100)
                        dt = time.perf_counter() - t0
                        assert len(v) == STEPS and np.isfinite(v).all()
                        if timed:
                            us[name].append(round(dt / STEPS * 1e6, 3))
                for _, ctx, _ in ctxs:
                    ctx.close()
            med = {k: float(np.median(v)) for k, v in us.items()}
            for k in us:
                emit(out, dict(kind=kind, shape=shape, variant=variant, build=k, us_per_step=us[k], median=med[k],
                               timed_steps=4 * STEPS))
            spread = round(max(us[OTHER_NAME]) - min(us[OTHER_NAME]), 3)
            within = med["this"] <= med[OTHER_NAME] + spread
            ok = ok and within
            emit(out, dict(kind=kind, shape=shape, variant=variant, this_minus_other_us=round(med["this"] - med[OTHER_NAME], 3),
                           other_spread_us=spread, within=within, created_first=first))
    return 0 if ok else 1


def profile(_):
    ctx, idx = clf_ctx((1000, 1000), True)
    ctx.train_many(idx[:200 * 100], 100)
    ctx.close()
    return 0


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    fh = open(sys.argv[2], "w") if len(sys.argv) > 2 else None
    fn = {"digests": digests, "time": timings, "time_ab": timings_ab, "profile": profile}.get(mode)
    if fn is None:
        sys.exit(__doc__)
    sys.exit(fn(fh))
