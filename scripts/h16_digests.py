#!/usr/bin/env python
"""SHA-256 digests of what the 16-bit engine computes, one line per case, for a bit-for-bit
comparison of two builds of the library (VAEB_LIB_VARIANT=<name> selects libvaeb_hip_<name>.so):

    python scripts/h16_digests.py > a.txt;  VAEB_LIB_VARIANT=parent python scripts/h16_digests.py > b.txt;  cmp a.txt b.txt

Training cases print: case id, then the digests of theta, the Adagrad state, the stored gradients
('-' without keep_grads), the 16-bit shadow (get_shadow) and the returned ELBO values.  Evaluation
cases print the digests of the returned values / arrays.  Six Philox steps per training case unless
its id says otherwise.  Switches are environment variables read at context creation, so every case
sets its own and restores the environment.  (RCCL prints a version banner to stdout at the first
comm_init; the files under profiles/r9 keep the case lines only.)"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import vaeb_oracle as O   # noqa: E402
from vaeb_amd import _lib             # noqa: E402

DTYPES = {"bf16": _lib.DTYPE_BF16, "fp16": _lib.DTYPE_F16}
ORDER = np.array([3, 1, 4, 1, 5, 2], np.int32)
# (D, H, Z, B, oracle Config options): the smallest shapes that reach each arm of the step
SHAPES = {
    "dzfuse": (256, 128, 32, 256, {}),
    "tails": (200, 136, 24, 200, {}),                      # Z % 16 != 0: split-K dz; D % 32 != 0: no bit copy of X
    "thin": (264, 200, 128, 200, {}),                      # thin launches, K tail
    "thin_gauss_mean": (128, 64, 256, 96, dict(continuous=True, objective="mean_map")),   # + fp16 loss scale
    "gauss": (256, 96, 16, 192, dict(continuous=True)),
    "la_l2": (128, 64, 16, 136, dict(estimator="LA", L=2)),
    "la_l8": (128, 64, 16, 40, dict(estimator="LA", L=8)),
    "dtt": (512, 264, 40, 520, {}),
}
SWITCHES = [("VAEB_BF_FORK", "0"), ("VAEB_BF_DTT", "0"), ("VAEB_BF_DZFUSE", "0"), ("VAEB_BF_THIN", "0"),
            ("VAEB_BF_THIN", "2"), ("VAEB_BF_GEMM8", "0"), ("VAEB_BF_GEMM8", "15")]
DP = [{"VAEB_DP_OVERLAP": o, "VAEB_DP_SHARD": s} for o in "01" for s in "01"] + \
     [{"VAEB_DP_OVERLAP": "1", "VAEB_BF_FORK": "0"}]


def sha(a):
    return "-" if a is None else hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32]


def setup(shape, dtype, keep_grads=True, use_graph=True, rows=None):
    D, H, Z, B, kw = SHAPES[shape]
    cfg = O.Config(D=D, H=H, Z=Z, **kw)
    ctx = _lib.Context(D, H, Z, B, L=cfg.L, decoder=int(cfg.continuous), estimator=int(cfg.estimator == "LA"),
                       objective=int(cfg.objective == "mean_map"), lr=cfg.lr, keep_grads=keep_grads, max_eval_rows=512,
                       use_graph=use_graph, dtype=DTYPES[dtype])
    n = rows or 6 * B
    x = O.synthetic_frey(n=n, D=D, seed=1) if cfg.continuous else O.synthetic_mnist(n=n, D=D, seed=1)
    ctx.set_data(x)
    ctx.set_params(O.flatten(O.init_params(cfg)))
    ctx.set_eps_mode(_lib.EPS_PHILOX, 10)
    ctx.set_step(0)
    return cfg, ctx, x


def state_line(cid, cfg, ctx, elbo, grads):
    nw = ctx.P - (2 * cfg.H + 2 * cfg.Z + cfg.D * (2 if cfg.continuous else 1))
    print(cid, sha(ctx.get_params()), sha(ctx.get_adagrad_state()), sha(ctx.get_grads() if grads else None),
          sha(ctx.get_shadow(nw)), sha(np.asarray(elbo, np.float64)), flush=True)
    ctx.close()


def train_case(cid, shape, dtype, env=None, form="many", keep_grads=True, comm=False):
    saved = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        cfg, ctx, _ = setup(shape, dtype, keep_grads=keep_grads, use_graph=form != "eager")
        if comm:
            ctx.comm_init(_lib.Context.comm_unique_id(), 0, 1)
        B = SHAPES[shape][3]
        if form == "single":          # vaeb_update: rows addressed from the call's index
            elbo = [ctx.update(int(i)) for i in ORDER]
        elif form == "host_eps":      # pushed eps, one step per push
            ctx.set_eps_mode(_lib.EPS_HOST)
            rng = np.random.default_rng(3)
            elbo = []
            for i in ORDER:
                ctx.push_eps(rng.standard_normal((cfg.L, B, cfg.Z)).astype(np.float32))
                elbo.append(ctx.update(int(i)))
        elif form == "profile":       # profiled steps are no training steps, but deterministic
            ctx.profile_steps(2)
            ctx.synchronize()
            elbo = []
        else:                         # update_many: graph replay, or eager launches (use_graph=False)
            ctx.update_many(ORDER)
            elbo = ctx.epoch_elbo()
        state_line(cid, cfg, ctx, elbo, keep_grads or comm)
    except _lib.VaebError as e:       # (a library error is an outcome too: both builds must report it)
        print(cid, "error:", e, flush=True)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def eval_case(dtype):
    n = 2 * 512 + 7                   # not a multiple of max_eval_rows
    cfg, ctx, x = setup("dzfuse", dtype, keep_grads=False, rows=n)
    ctx.update_many(ORDER[:2])        # off theta_0
    ctx.synchronize()
    v = ctx.validate(x)
    ctx.set_valid_data(x)
    vr = ctx.validate_resident()
    print(f"eval-{dtype}", sha(np.float64([v, vr])), sha(ctx.reconstruct(x)), sha(ctx.reconstruct_sampled(x, 3)), end=" ")
    ctx.set_eps_mode(_lib.EPS_HOST)
    ctx.push_eps(np.random.default_rng(4).standard_normal((1, 3 * n, cfg.Z)).astype(np.float32))
    print(sha(ctx.reconstruct_sampled(x, 3)), flush=True)
    ctx.close()


def main():
    for dtype in DTYPES:
        for shape in SHAPES:
            train_case(f"shape-{shape}-{dtype}", shape, dtype)
        for shape in ("dzfuse", "thin", "dtt"):
            for var, val in SWITCHES:
                train_case(f"switch-{shape}-{var}={val}-{dtype}", shape, dtype, env={var: val}, keep_grads=False)
        for form in ("eager", "single", "host_eps", "profile"):
            train_case(f"form-{form}-{dtype}", "dzfuse", dtype, form=form)
        for env in DP:
            tag = ",".join(f"{k}={v}" for k, v in env.items())
            train_case(f"dp-{tag}-{dtype}", "dzfuse", dtype, env=env, keep_grads=False, comm=True)
        eval_case(dtype)


if __name__ == "__main__":
    main()
