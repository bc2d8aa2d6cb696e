#!/usr/bin/env python
"""SHA-256 digests of what the context layer returns (evaluation calls, buffer lifecycle, the
layer-stack engine), one line per case, for a bit-for-bit comparison of two builds of the library
(VAEB_LIB_VARIANT=<name> selects libvaeb_hip_<name>.so):

    python scripts/ctx_digests.py a.txt;  VAEB_LIB_VARIANT=parent python scripts/ctx_digests.py b.txt;  cmp a.txt b.txt

Every context has max_eval_rows = 64 and evaluates n = 2 * 64 + 7 rows: three chunks, the last one
neither full nor a multiple of 16.  Each evaluation case runs two Philox training steps first, so
theta is off its start.  A line is the case id followed by name=digest pairs; a call the library
refuses prints name=error:<text> (both builds must refuse with the same text).  Lines go to the
file named on the command line (stdout without one; RCCL prints a banner to stdout at comm_init)."""
import hashlib
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import vaeb_oracle as O   # noqa: E402
from vaeb_amd import _lib             # noqa: E402

MER = 64
N = 2 * MER + 7
K = 5                                  # more samples than one pass holds for the 7-row chunk at L = 1
EST = {"LB": _lib.EST_LB, "LA": _lib.EST_LA, "FV": _lib.EST_FV, "FVS": _lib.EST_FVS}
DTYPES = {"f32": _lib.DTYPE_F32, "bf16": _lib.DTYPE_BF16, "fp16": _lib.DTYPE_F16}
OUT = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout


def sha(a):
    if a is None:
        return "-"
    if isinstance(a, (tuple, list)):
        return "+".join(sha(v) for v in a)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


def call(f, *a, **kw):
    """The digest of f's result, or the library's refusal."""
    try:
        r = f(*a, **kw)
        return sha(np.float64(r) if isinstance(r, float) else r)
    except _lib.VaebError as e:
        return "error:" + str(e).replace(" ", "_")


def line(cid, pairs):
    print(cid, " ".join(f"{k}={v}" for k, v in pairs), file=OUT, flush=True)


def data(D, gauss, n=N, seed=1):
    return O.synthetic_frey(n=n, D=D, seed=seed) if gauss else O.synthetic_mnist(n=n, D=D, seed=seed)


def make(D, H, Z, B, gauss=False, est="LB", L=1, dtype="f32", x=None, keep_grads=False):
    """A context with data, start parameters, Philox noise and step 0."""
    cfg = O.Config(D=D, H=H, Z=Z, continuous=gauss, L=L, estimator="LB" if est == "FVS" else est)
    ctx = _lib.Context(D, H, Z, B, L=L, decoder=int(gauss), estimator=EST[est], max_eval_rows=MER,
                       dtype=DTYPES[dtype], keep_grads=keep_grads)
    ctx.set_data(data(D, gauss) if x is None else x)
    flat = O.flatten(O.init_params(cfg))
    ctx.set_params(flat)
    if est in ("FV", "FVS"):
        ctx.set_fv_state(flat, np.full_like(flat, 1e-3), np.zeros_like(flat), np.zeros_like(flat))
    ctx.set_eps_mode(_lib.EPS_PHILOX, 10)
    ctx.set_step(0)
    return ctx


def eps_for(ctx, rows, seed):
    c = ctx.cfg
    return np.random.default_rng(seed).standard_normal((c.L, rows, c.Z)).astype(np.float32)


def train6(ctx):
    """Six Philox steps: theta, the Adagrad state and the ELBO values."""
    def run():
        ctx.set_eps_mode(_lib.EPS_PHILOX, 10)
        vals = [ctx.update(i % 2) for i in range(2)]
        ctx.update_many(np.array([1, 0, 1, 0], np.int32))
        vals += list(ctx.epoch_elbo())
        return [ctx.get_params(), ctx.get_adagrad_state(), np.float64(vals)]
    return call(run)


# ------------------------------------------------------------------ evaluation calls
def eval_case(cid, D, H, Z, B, gauss, est, L, dtype):
    x = data(D, gauss)
    try:
        ctx = make(D, H, Z, B, gauss, est, L, dtype, x=x)
    except _lib.VaebError as e:
        return line(cid, [("create", "error:" + str(e).replace(" ", "_"))])
    out = [("two_steps", call(lambda: (ctx.update_many(np.array([1, 0], np.int32)), ctx.synchronize(), ctx.get_params())[2]))]
    z = np.random.default_rng(7).standard_normal((N, Z)).astype(np.float32)
    out.append(("validate", call(ctx.validate, x)))
    out.append(("set_valid", call(ctx.set_valid_data, x)))
    out.append(("validate_res", call(ctx.validate_resident)))
    out.append(("recon", call(ctx.reconstruct, x)))
    out.append(("recon3", call(ctx.reconstruct_sampled, x, 3)))
    out.append(("full0", call(ctx.reconstruct_full, x, 0)))
    out.append(("full3", call(ctx.reconstruct_full, x, 3)))
    out.append(("decode", call(ctx.decode, z)))
    out.append(("encode", call(ctx.encode, x)))
    out.append(("mll", call(ctx.marginal_ll, x, K, rows=True)))
    out.append(("mll_res", call(ctx.marginal_ll_resident, K)))
    # host eps: the rows each call needs, pushed before it
    ctx.set_eps_mode(_lib.EPS_HOST)
    for name, rows, f in (("h_validate", N, lambda: ctx.validate(x)),
                          ("h_validate_res", N, ctx.validate_resident),
                          ("h_recon3", 3 * N, lambda: ctx.reconstruct_sampled(x, 3)),
                          ("h_full3", 3 * N, lambda: ctx.reconstruct_full(x, 3)),
                          ("h_mll", K * N, lambda: ctx.marginal_ll(x, K, rows=True)),
                          ("h_mll_res", K * N, lambda: ctx.marginal_ll_resident(K))):
        ctx.push_eps(eps_for(ctx, rows, 4))
        out.append((name, call(f)))
    # the all-reduce arm of the two resident calls (a communicator of one rank)
    ctx.set_eps_mode(_lib.EPS_PHILOX, 10)
    out.append(("comm", call(lambda: ctx.comm_init(_lib.Context.comm_unique_id(), 0, 1))))
    out.append(("c_validate_res", call(ctx.validate_resident)))
    out.append(("c_mll_res", call(ctx.marginal_ll_resident, K)))
    ctx.close()
    line(cid, out)


# ------------------------------------------------------------------ buffer lifecycle
def lifecycle(dtype, D, H, Z, B):
    x = data(D, False)
    tail = lambda ctx: [("validate", call(ctx.validate, x)), ("train6", train6(ctx))]   # noqa: E731

    ctx = make(D, H, Z, B, dtype=dtype, x=data(D, False, n=3 * B + 5, seed=2))
    ctx.update_many(np.array([2, 0, 1], np.int32))
    ctx.synchronize()
    ctx.set_data(x)                                  # fewer rows than before, graphs captured in between
    line(f"life-set_data-{dtype}", [("after", call(ctx.get_params))] + tail(ctx))
    ctx.close()

    ctx = make(D, H, Z, B, dtype=dtype, x=x)
    ctx.set_valid_data(data(D, False, n=MER + 3, seed=3))
    first = call(ctx.validate_resident)
    ctx.set_valid_data(x)
    line(f"life-set_valid-{dtype}", [("first", first), ("second", call(ctx.validate_resident))] + tail(ctx))
    ctx.close()

    ctx = make(D, H, Z, B, dtype=dtype, x=x)
    ctx.set_eps_mode(_lib.EPS_HOST)
    out = []
    for rows in (B, 3 * N, N):                        # grows, then shrinks inside the grown buffer
        ctx.push_eps(eps_for(ctx, rows, rows))
        if rows == B:
            out.append(("step", call(ctx.update, 0)))
        elif rows == 3 * N:
            out.append(("recon3", call(ctx.reconstruct_sampled, x, 3)))
        else:
            out.append(("h_validate", call(ctx.validate, x)))
    for i in range(3):                                # host-eps steps from the shrunk buffer
        ctx.push_eps(eps_for(ctx, B, 20 + i))
        out.append((f"h_step{i}", call(ctx.update, i % 2)))
    ctx.push_eps(eps_for(ctx, N, 40))                 # and the rows the closing validate needs
    line(f"life-push_eps-{dtype}", out + tail(ctx))
    ctx.close()

    a = make(D, H, Z, B, dtype=dtype, x=x)
    a.update_many(np.array([1, 0, 1], np.int32))
    a.synchronize()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "ctx.ckpt")
        a.checkpoint_save(path)
        b = make(D, H, Z, B, dtype=dtype, x=x)
        b.update_many(np.array([0, 1], np.int32))    # graphs captured before the load
        b.synchronize()
        b.checkpoint_load(path)
    line(f"life-checkpoint-{dtype}", [("step", str(b.get_step())), ("theta", call(b.get_params)),
                                       ("same", str(np.array_equal(a.get_params(), b.get_params())))] + tail(b))
    a.close()
    b.close()

    ctx = make(D, H, Z, B, dtype=dtype, x=x)
    tl = call(lambda: np.int64(ctx.debug_timeline(1).shape))
    line(f"life-timeline-{dtype}", [("launches", tl)] + tail(ctx))
    ctx.close()


def lifecycle_fvs(D, H, Z, B):
    x = data(D, False)
    ctx = make(D, H, Z, B, est="FVS", x=x)
    ctx.set_eps_mode(_lib.EPS_HOST)
    rng = np.random.default_rng(11)
    out = []
    for i in range(3):
        ctx.push_fv_noise(rng.standard_normal(ctx.P).astype(np.float32))
        ctx.push_eps(eps_for(ctx, B, 30 + i))
        out.append((f"step{i}", call(ctx.update, i % 2)))
    out.append(("fv", call(ctx.get_fv_state)))
    ctx.set_eps_mode(_lib.EPS_PHILOX, 10)
    line("life-push_fv_noise-f32", out + [("validate", call(ctx.validate, x)), ("train6", train6(ctx))])
    ctx.close()


# ------------------------------------------------------------------ the layer-stack engine
def ae_case(cid, Dobs, Denc, Dz, Ddec, otype, mb, n):
    rng = np.random.default_rng(5)
    X = (rng.random((n, Dobs)) < 0.3).astype(np.float32) if otype == "binary" else rng.random((n, Dobs)).astype(np.float32)
    ctx = _lib.AEContext(Dobs, Denc, Dz, Ddec, otype=otype, max_batch=mb, latent="gauss")
    ctx.set_data(X)
    ctx.set_params((0.1 * rng.standard_normal(ctx.P)).astype(np.float32))
    ctx.set_eps_mode(_lib.EPS_PHILOX, 10)
    ctx.set_step(3)
    idx = np.concatenate([rng.permutation(n), rng.permutation(n)]).astype(np.int32)   # two epochs, partial last batches
    out = [("train_many", call(lambda: [ctx.train_many(idx[:n], mb), ctx.train_many(idx[n:], mb)])),
           ("theta", call(ctx.get_params)), ("acc", call(ctx.get_adagrad_state)),
           ("recon", call(ctx.reconstruct, X)), ("encode_dist", call(ctx.encode_dist, X)),
           ("elbo", call(ctx.elbo, X)), ("mll", call(ctx.marginal_ll, X, K, rows=True))]
    ctx.set_data(X[: n // 2])                         # the replaced dataset buffer
    out.append(("train_half", call(ctx.train, np.arange(min(mb, n // 2), dtype=np.int32))))
    ctx.close()
    line(cid, out)


def main():
    for D, H, Z in ((72, 40, 8), (64, 48, 40)):      # fused latent; Z > 32: split heads
        for gauss in (False, True):
            for est, L in (("LB", 1), ("LA", 2), ("FV", 1), ("FVS", 1)):
                eval_case(f"eval-f32-{D}-{H}-{Z}-{'gauss' if gauss else 'bern'}-{est}", D, H, Z, 32, gauss, est, L, "f32")
    for dtype in ("bf16", "fp16"):
        eval_case(f"eval-{dtype}-256-128-32-bern-LB", 256, 128, 32, 64, False, "LB", 1, dtype)
        eval_case(f"eval-{dtype}-256-96-16-gauss-LB", 256, 96, 16, 64, True, "LB", 1, dtype)
    lifecycle("f32", 72, 40, 8, 32)
    lifecycle("bf16", 256, 128, 32, 64)
    lifecycle_fvs(72, 40, 8, 32)
    ae_case("ae-96-40-6-binary", 96, (40,), 6, (40,), "binary", 100, 350)
    ae_case("ae-24-12-20-cont", 24, (12,), 20, (12,), "cont", 16, 55)


if __name__ == "__main__":
    main()
