"""Step time of the layer-stack deep VAE: 784-(500)-20-(500), B = 100, one
train_many epoch of --steps steps per round, one warm-up round and --rounds timed ones (host clock
around the call, which ends in a stream synchronise); prints one JSON line with the median and
the range in us per step, and SHA-256 digests of theta and of the per-step values after the last
round (the same inputs, seed and step in every process: two builds that compute the same bits print
the same digests).

    --iw K        iw_samples (0: the ELBO step); max_batch = 100 max(K, 1)
    --otype       binary | cont
VAEB_LIB_VARIANT=<v> loads vaeb_amd/libvaeb_hip_<v>.so (an earlier build) instead; an earlier build
has no iw_samples, so --iw 0 does not pass the argument.
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vaeb_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iw", type=int, default=0)
    ap.add_argument("--otype", default="binary")
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=100)
    a = ap.parse_args()
    D, H, Z, N = 784, 500, 20, 10000
    rng = np.random.default_rng(0)
    X = (rng.random((N, D)) < 0.3).astype(np.float32) if a.otype == "binary" else rng.beta(2, 2, (N, D)).astype(np.float32)
    kw = {"iw_samples": a.iw} if a.iw else {}
    ctx = _lib.AEContext(D, [H], Z, [H], otype=a.otype, act="tanh", max_batch=a.batch * max(a.iw, 1), latent="gauss", **kw)
    ctx.set_data(X)
    ctx.set_params(rng.normal(0.0, 0.01, ctx.P).astype(np.float32))
    ctx.set_eps_mode(_lib.EPS_PHILOX, 10)
    idx = rng.integers(0, N, a.steps * a.batch).astype(np.int32)
    us = []
    for r in range(a.rounds + 1):
        t0 = time.perf_counter()
        vals = ctx.train_many(idx, a.batch)
        dt = time.perf_counter() - t0
        if r:
            us.append(dt / a.steps * 1e6)
    theta = ctx.get_params()
    print(json.dumps({
        "variant": os.environ.get("VAEB_LIB_VARIANT", "this"), "iw": a.iw, "otype": a.otype, "steps": a.steps,
        "us_per_step_median": round(float(np.median(us)), 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2),
        "last_value": float(vals[-1]), "finite": bool(np.isfinite(theta).all() and np.isfinite(vals).all()),
        "theta_sha": hashlib.sha256(theta.tobytes()).hexdigest()[:16],
        "values_sha": hashlib.sha256(np.ascontiguousarray(vals).tobytes()).hexdigest()[:16]}))
    ctx.close()


if __name__ == "__main__":
    main()
