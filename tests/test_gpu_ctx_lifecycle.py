"""Device-memory lifecycle of a context (vaeb_hip.hip: every buffer belongs to the context's
DevOwner, dev_owner.hpp): buffers that calls replace -- the dataset, the resident validation set,
the pushed eps, the FVS weight noise -- a checkpoint round trip and one diagnostics timeline, with
captured graphs in between.  None of it may change what the context computes: after the sequence
the context validates bit for bit like a fresh context given the same data, parameters, seed and
step.  And a process can create and destroy contexts for as long as it likes."""
import numpy as np
import pytest

from oracle import vaeb_oracle as O

pytestmark = pytest.mark.gpu

D, H, Z, B, MER = 72, 40, 8, 32, 64
N = 2 * MER + 7
DTYPES = ["f32", "bf16"]


def make(dtype, x, **kw):
    from vaeb_amd import _lib
    d, h, z = (D, H, Z) if dtype == "f32" else (256, 128, 32)
    ctx = _lib.Context(d, h, z, B, max_eval_rows=MER, dtype=_lib.DTYPE_F32 if dtype == "f32" else _lib.DTYPE_BF16, **kw)
    ctx.set_data(x)
    ctx.set_params(O.flatten(O.init_params(O.Config(D=d, H=h, Z=z))))
    ctx.set_eps_mode(_lib.EPS_PHILOX, 10)
    ctx.set_step(0)
    return ctx


@pytest.mark.parametrize("dtype", DTYPES)
def test_replaced_buffers_leave_the_context_as_a_fresh_one(dtype, tmp_path):
    from vaeb_amd import _lib
    d, z = (D, Z) if dtype == "f32" else (256, 32)
    xa = O.synthetic_mnist(n=3 * B + 5, D=d, seed=2)
    xb = O.synthetic_mnist(n=N, D=d, seed=1)
    rng = np.random.default_rng(4)
    ctx = make(dtype, xa)
    first = ctx.validate(xb)
    ctx.update_many(np.array([2, 0, 1], np.int32))             # graphs captured on the first dataset
    ctx.set_data(xb)                                            # ... which a second, longer one replaces
    ctx.update_many(np.array([3, 1], np.int32))
    ctx.set_valid_data(xa)
    ctx.validate_resident()
    ctx.set_valid_data(xb)                                      # the resident set replaced
    ctx.set_eps_mode(_lib.EPS_HOST)
    for rows in (B, 3 * N, N):                                  # the eps buffer grows, then is reused shrunk
        ctx.push_eps(rng.standard_normal((1, rows, z)).astype(np.float32))
    host_v = ctx.validate(xb)
    ctx.push_eps(rng.standard_normal((1, B, z)).astype(np.float32))
    ctx.update(0)
    ctx.set_eps_mode(_lib.EPS_PHILOX, 10)
    stamped = ctx.debug_timeline(1).shape[0]                    # one stamped step (fp32 launches stamp), then plain ones
    assert stamped >= 1 or dtype != "f32"
    ctx.update_many(np.array([0, 1, 2], np.int32))
    ctx.synchronize()
    path = str(tmp_path / "ctx.ckpt")
    ctx.checkpoint_save(path)
    other = make(dtype, xb)
    other.update_many(np.array([1, 0], np.int32))               # graphs captured before the load
    other.checkpoint_load(path)
    assert other.get_step() == ctx.get_step()
    assert np.array_equal(other.get_params(), ctx.get_params())
    assert np.array_equal(other.get_adagrad_state(), ctx.get_adagrad_state())

    second = ctx.validate(xb)
    resident = ctx.validate_resident()
    fresh = make(dtype, xb)
    fresh.set_params(ctx.get_params())
    fresh.set_adagrad_state(ctx.get_adagrad_state())
    fresh.set_step(ctx.get_step())
    assert np.isfinite(first) and np.isfinite(host_v) and second != first
    assert second == fresh.validate(xb)                         # bitwise
    assert second == other.validate(xb)
    assert resident == second                                   # the same rows, chunks and noise keys
    # ... and all three train on alike
    order = np.array([1, 3, 0, 2, 1, 0], np.int32)
    runs = []
    for c in (ctx, other, fresh):
        c.update_many(order)
        runs.append((c.epoch_elbo()[0] if c is fresh else None, c.get_params(), c.get_adagrad_state()))
        c.close()
    for _, p, a in runs[:2]:
        assert np.array_equal(p, runs[2][1]) and np.array_equal(a, runs[2][2])
    assert np.isfinite(runs[2][0])


def test_fvs_weight_noise_buffer_is_created_once():
    """push_fv_noise allocates on first use (and drops the captured graphs once)."""
    from vaeb_amd import _lib
    x = O.synthetic_mnist(n=N, D=D, seed=1)
    vals = []
    for _ in range(2):
        ctx = make("f32", x, estimator=_lib.EST_FVS)
        flat = ctx.get_params()
        ctx.set_fv_state(flat, np.full_like(flat, 1e-3), np.zeros_like(flat), np.zeros_like(flat))
        ctx.update_many(np.array([0, 1], np.int32))             # Philox steps: graphs without a noise buffer
        ctx.set_eps_mode(_lib.EPS_HOST)
        rng = np.random.default_rng(11)
        out = []
        for i in range(3):
            ctx.push_fv_noise(rng.standard_normal(ctx.P).astype(np.float32))
            ctx.push_eps(rng.standard_normal((1, B, Z)).astype(np.float32))
            out.append(ctx.update(i))
        vals.append((out, ctx.get_fv_state()[0]))
        ctx.close()
    assert np.all(np.isfinite(vals[0][0])) and vals[0][0] == vals[1][0]
    assert np.array_equal(vals[0][1], vals[1][1])


def test_fifty_contexts_created_and_destroyed_then_one_more():
    from vaeb_amd import _lib
    x = O.synthetic_mnist(n=2 * B, D=D, seed=1)
    for i in range(50):
        kind = i % 3
        if kind == 2:
            ae = _lib.AEContext(24, (12,), 4, (12,), max_batch=16)
            ae.set_data(x[:, :24])
            ae.set_data(x[:16, :24])
            ae.close()
            continue
        ctx = make("bf16" if kind else "f32", O.synthetic_mnist(n=2 * B, D=256, seed=1) if kind else x)
        ctx.set_valid_data(x if not kind else O.synthetic_mnist(n=B, D=256, seed=3))
        ctx.update(1)
        ctx.close()
    ctx = make("f32", x)
    assert np.isfinite(ctx.update(0)) and np.isfinite(ctx.validate(x))
    ctx.close()
