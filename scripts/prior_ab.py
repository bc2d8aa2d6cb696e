#!/usr/bin/env python
"""Two-mode latent prior: the evidence lines under profiles/latent_prior/.

    python scripts/prior_ab.py digests [out]   normal-prior contexts, this build against another
    python scripts/prior_ab.py time [out]      train_many us per step, the two builds alternating
    python scripts/prior_ab.py learn [out]     a short two-mode training run with a falling width

The other build is vaeb_amd/libvaeb_hip_<VAEB_AB_OTHER>.so (default "parent": the library of the
parent commit, built there with __graft_entry__.build() and copied under that name).  Both
libraries are loaded into this one process: vaeb_amd/_lib.py a second time under another module name
with VAEB_LIB_VARIANT set while it loads.

digests: one multi-step sequence per model (point, Gaussian ELBO, iw_samples = 3, MASK-corrupting
Gaussian) on each build; a line per (build, model) with SHA-256 digests of theta, the accumulators and
the per-step values, then `identical=` per model.
time: 784-(500)-20-(500), binary, B = 100, train_many over 600 steps, one warm-up round
and five timed rounds of: other build normal, this build normal, this build two-mode, other build
again.  The last against the first is the spread the other build shows against itself.
learn: ConstructVAE(prior=("twomode", w0)) on synthetic rows, the width falling per epoch; reports
marginal_ll, the share of |mu - nearest mode| < width, and the reconstruction error of
decode_code(code(X)) against that of reconstruct(X).  An observation, no pass mark.
"""
import hashlib
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vaeb_amd import _lib as THIS   # noqa: E402

OTHER_NAME = os.environ.get("VAEB_AB_OTHER", "parent")


def other_lib():
    """vaeb_amd/_lib.py once more, bound to libvaeb_hip_<OTHER_NAME>.so."""
    os.environ["VAEB_LIB_VARIANT"] = OTHER_NAME
    try:
        spec = importlib.util.spec_from_file_location("vaeb_lib_other", os.path.join(ROOT, "vaeb_amd", "_lib.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.load()
    finally:
        del os.environ["VAEB_LIB_VARIANT"]
    return mod


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


def emit(out, rec):
    s = json.dumps(rec)
    print(s, flush=True)
    if out:
        out.write(s + "\n")
        out.flush()


# ------------------------------------------------------------------ digests
MODELS = {
    "point": dict(latent="point"),
    "gauss_elbo": dict(latent="gauss"),
    "gauss_iw3": dict(latent="gauss", iw_samples=3),
    "gauss_mask": dict(latent="gauss", corruption="mask"),
}


def sequence(L, kw):
    """Two epochs of train_many (partial last batch) from fixed theta: theta, acc, values."""
    rng = np.random.default_rng(5)
    Dobs, n, B = 96, 230, 32
    X = (rng.random((n, Dobs)) < 0.3).astype(np.float32)
    K = kw.get("iw_samples", 1)
    ctx = L.AEContext(Dobs, (40, 24), 17, (24, 40), otype="binary", max_batch=K * B, **kw)
    try:
        ctx.set_data(X)
        ctx.set_params((0.1 * rng.standard_normal(ctx.P)).astype(np.float32))
        if kw["latent"] == "gauss":
            ctx.set_eps_mode(L.EPS_PHILOX, 10)
            ctx.set_step(3)
        if kw.get("corruption"):
            ctx.set_corruption_noise(L.EPS_PHILOX, 11)
            ctx.set_corruption_level(0.3)
        vals = [ctx.train_many(rng.permutation(n).astype(np.int32), B) for _ in range(2)]
        return dict(theta=sha(ctx.get_params()), acc=sha(ctx.get_adagrad_state()), values=sha(np.concatenate(vals)),
                    steps=int(sum(len(v) for v in vals)), last_value=float(vals[-1][-1]))
    finally:
        ctx.close()


def digests(out):
    libs = {"this": THIS, OTHER_NAME: other_lib()}
    res = {}
    for model, kw in MODELS.items():
        for name, L in libs.items():
            res[model, name] = sequence(L, kw)
            emit(out, dict(build=name, model=model, **res[model, name]))
    ok = True
    for model in MODELS:
        same = res[model, "this"] == res[model, OTHER_NAME]
        ok = ok and same
        emit(out, dict(model=model, identical=same))
    return 0 if ok else 1


# ------------------------------------------------------------------ time
def timed_ctx(L, prior):
    rng = np.random.default_rng(3)
    n = 6000
    X = (rng.random((n, 784)) < 0.3).astype(np.float32)
    kw = {"prior": "twomode"} if prior == "twomode" else {}
    ctx = L.AEContext(784, (500,), 20, (500,), otype="binary", max_batch=100, latent="gauss", **kw)
    ctx.set_data(X)
    ctx.set_params((0.01 * rng.standard_normal(ctx.P)).astype(np.float32))
    ctx.set_eps_mode(L.EPS_PHILOX, 10)
    idx = np.concatenate([rng.permutation(n) for _ in range(10)]).astype(np.int32)   # 600 steps of 100
    return ctx, idx


def timings(out):
    O = other_lib()
    cfgs = [("a_other_normal", O, "normal"), ("b_this_normal", THIS, "normal"), ("c_this_twomode", THIS, "twomode"),
            ("d_other_normal_again", O, "normal")]
    ctxs = [(name,) + timed_ctx(L, prior) for name, L, prior in cfgs]
    us = {name: [] for name, _, _ in ctxs}
    for rnd in range(6):                       # round 0 warms up
        for name, ctx, idx in ctxs:
            t0 = time.perf_counter()
            ctx.train_many(idx, 100)
            dt = time.perf_counter() - t0
            if rnd:
                us[name].append(round(dt / 600 * 1e6, 3))
    for name, ctx, _ in ctxs:
        ctx.close()
    med = {k: float(np.median(v)) for k, v in us.items()}
    for k in us:
        emit(out, dict(config=k, other=OTHER_NAME, us_per_step=us[k], median=med[k], steps_per_round=600))
    emit(out, dict(other_against_itself=round(med["d_other_normal_again"] - med["a_other_normal"], 3),
                   this_normal_minus_other=round(med["b_this_normal"] - med["a_other_normal"], 3),
                   twomode_minus_normal=round(med["c_this_twomode"] - med["b_this_normal"], 3)))
    return 0


# ------------------------------------------------------------------ learn
def learn(out):
    from vaeb_amd import ae
    rng = np.random.default_rng(0)
    # rows that are binary codes at heart: 8 hidden bits, each lighting a random pattern of pixels
    nbits, D, n = 8, 196, 4000
    patterns = rng.random((nbits, D)) < 0.15
    bits = rng.random((n, nbits)) < 0.5
    p = 0.05 + 0.9 * (1 - np.prod(1 - bits[:, :, None] * patterns[None], axis=1))
    X = (rng.random((n, D)) < p).astype(np.float32)
    np.random.seed(15485863)
    widths = [round(float(w), 3) for w in np.linspace(0.5, 0.1, 60)]   # one per epoch of 40 steps
    train, reconstruct, encode, decode, theta = ae.ConstructVAE(X, Denc=[128], Dz=16, Ddec=[128], max_batch=1000,
                                                                prior=("twomode", widths[0]))

    def report(epoch):
        a, w = train.prior
        mu = encode(X)
        near = np.minimum(np.abs(mu), np.abs(mu - a))
        direct = train.ctx.sq_error(X) / n
        coded = float(((X - train.decode_code(train.code(X))) ** 2).sum() / n)
        emit(out, dict(epoch=epoch, width=round(w, 4), marginal_ll_per_row=round(train.marginal_ll(X, 16) / n, 3),
                       share_mu_within_width_of_a_mode=round(float((near < w).mean()), 4),
                       sq_error_reconstruct=round(direct, 3), sq_error_decode_code=round(coded, 3),
                       bits_set=round(float(train.code(X).mean()), 3)))

    report(0)
    for e, w in enumerate(widths):
        train.set_prior(width=w)
        ae.train_epochs(train, n, 1, batch_size=100, verbose=False)
        if e % 10 == 9:
            report(e + 1)
    return 0


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    fh = open(sys.argv[2], "w") if len(sys.argv) > 2 else None
    fn = {"digests": digests, "time": timings, "learn": learn}.get(mode)
    if fn is None:
        sys.exit(__doc__)
    sys.exit(fn(fh))
