"""The evaluation-only forward of the fp32 engine, row by row against the float64 oracle.

Evaluation chunks never take the folded training kernels (engine_f32.inc folded_latent), so
vaeb_validate, vaeb_validate_resident, vaeb_reconstruct*, vaeb_decode and vaeb_encode run PEnc
(big-K), heads_dechid_kernel<1 | 2> (Z <= 32) or PHeads + PDecHid (Z > 32), PDecOut in MODE_EVAL /
MODE_RECON and elbo_kernel -- kernels a training step with Z <= 32 never launches.  Here they are
checked per element and per (sample, row) at L > 4 (heads_dechid_kernel's l >= kLP planes read z
back from global memory), H > 512 and H > 1024 (its second tile loop, GCH = 8 in the decoder
output), Z > 32, odd shapes and the Gaussian decoder, in one chunk and in chunks whose last one is
short: elbo_kernel sums Me * nctD partials, pad rows included, and after a full chunk the pad
rows of a short one sit on stale rows, so every pad-row partial has to be exactly 0.

Parameters, data and noise (the recipe of tests/test_gpu_marginal_ll.py::make_case): every tensor
0.1 * default_rng(3).standard_normal(shape) as float32; eps [L, n, Z], then the three
reconstruction samples [3, n, Z], from the same generator afterwards; data from the oracle's
synthetic sets with seed 5.  Reference: O.forward_backward(..., need_grad=False) in float64.

Device layouts (rows of the LAST chunk of the call, Mp = its rows rounded up to 16):
  h, mu, lv [Mp][.]; eps, z, hd [L][Mp][.]
  lp_part  [(l * Mp + m) * cdiv(D, 16) + tile]                    (phases.hpp PDecOut::epilogue_row)
  kl_part  LB [m * cdiv(Z, 16) + t], LA [(l * Mp + m) * cdiv(Z, 16) + t]
           (fused.hpp heads_dechid_kernel for Z <= 32; for Z > 32 PHeads::epilogue writes the
           same two layouts with t the 16-column tile of the launch, read at phases.hpp:182, 187)

Tolerances
  * activations and decoder outputs: 1e-5 absolute, the project's number (tests/test_gpu_step.py);
    at H = 1040 max(1e-5, 16 x restatement error), where the restatement error is the max
    absolute difference between the float32 and the float64 NumPy run of the same oracle function;
  * log p per (sample, row) and every validate sum: 1e-4 relative (the project's ELBO tolerance);
  * KL (LB) / prior - log q (LA) per row: 16 x the restatement error of those rows (they go down
    to ~5e-3, so a relative bound is ill-conditioned; summation order and the device's fast exp
    each cost a few float32 roundings of the operands, and the restatement holds one of each);
  * stored eps: equal to the pushed float32 values; pad-row partials: exactly 0.0.
No tolerance comes from the device's output.

Recorded on the first run on an MI355X (every test prints its figures; -s shows them).  Max error
of the device against float64 / restatement error, single-chunk contexts:

  case             z              hd             log p rows (rel)  KL | LA rows: device / restatement / bound
  odd_z3           1.5e-7/3.2e-7  1.1e-7/9.2e-8  7.2e-8            5.6e-8 / 1.5e-7 / 2.4e-6
  odd_z3_chunks20  8.8e-8/3.2e-7  9.5e-8/9.2e-8  8.2e-8            3.9e-8 / 9.5e-8 / 1.5e-6
  z28_LA_L6        7.6e-7/9.3e-7  3.2e-7/3.3e-7  5.5e-8            3.6e-6 / 1.1e-5 / 1.7e-4
  z36_L2           3.5e-7/4.2e-7  2.5e-7/3.2e-7  6.6e-8            8.8e-7 / 4.5e-7 / 7.2e-6
  gauss_oddD_L5    1.9e-7/4.1e-7  1.4e-7/9.8e-8  5.7e-8            1.5e-7 / 1.5e-7 / 2.4e-6
  h600             4.6e-7/4.8e-7  2.3e-7/1.9e-7  6.3e-8            1.1e-6 / 9.0e-7 / 1.4e-5
  h1040_gauss_L5   1.5e-6/3.1e-6  6.5e-7/1.3e-6  6.6e-7            2.7e-6 / 1.0e-5 / 1.7e-4
  d784_LA_L5       4.6e-7/7.8e-7  2.2e-7/2.6e-7  3.2e-8            2.3e-6 / 5.9e-6 / 9.5e-5

h, mu, lv <= 9.4e-7 (h1040_gauss_L5 mu; its bound 4.1e-5, elsewhere <= 4.2e-7 against 1e-5); every
validate sum (one chunk or several, host eps or Philox, host rows or resident) within 2.6e-8
relative; the decoder means of reconstruct / reconstruct_sampled / reconstruct_full / decode
<= 3.4e-7 and the log-sigma heads <= 1.5e-6 (h1040_gauss_L5, restatement 4.5e-6, bound 7.1e-5);
no non-zero pad-row partial.
"""
import functools

import numpy as np
import pytest

from oracle import philox as P
from oracle import vaeb_oracle as O
from tests.test_gpu_marginal_ll import stacked
from tests.test_gpu_step import make_ctx
from tests.test_philox_oracle import STEP

pytestmark = pytest.mark.gpu

B = 16
SEED = (37 << 32) | 0x2468ACE
ODD = dict(D=37, H=19, Z=3)
CASES = {
    # name: (config, n, max_eval_rows of the contexts)
    "odd_z3": (ODD, 13, (16,)),
    "odd_z3_chunks20": (ODD, 50, (20,)),                                         # chunks 20, 20, 10
    "z28_LA_L6": (dict(D=200, H=96, Z=28, estimator="LA", L=6), 37, (48, 16)),   # one chunk; 16, 16, 5
    "z36_L2": (dict(D=66, H=48, Z=36, L=2), 30, (32,)),
    "gauss_oddD_L5": (dict(D=45, H=30, Z=6, continuous=True, L=5), 17, (32,)),
    "h600": (dict(D=48, H=600, Z=8), 20, (32,)),
    "h1040_gauss_L5": (dict(D=36, H=1040, Z=20, continuous=True, L=5), 19, (32,)),
    "d784_LA_L5": (dict(D=784, H=64, Z=20, estimator="LA", L=5), 20, (32,)),
}
SINGLE = [(name, mer) for name, (_, _, mers) in CASES.items() for mer in mers]


def chunked_mers(name):
    """The case's own sizes plus one that splits its rows into a full first and a short last
    chunk (16 where the listed ones hold all rows)."""
    _, n, mers = CASES[name]
    return sorted(set(mers) | ({16} if min(mers) >= n else set()), reverse=True)


CHUNKED = [(name, mer) for name in CASES for mer in chunked_mers(name)]


def r16(n):
    return (n + 15) // 16 * 16


def maxabs(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


@functools.lru_cache(maxsize=None)
def case(name):
    """cfg, float32 params / x / eps / eps3, the float64 forward and per-row outputs, and the
    restatement error (float32 vs float64 NumPy) of each of them; computed once per case."""
    kw, n, _ = CASES[name]
    cfg = O.Config(**kw)
    rng = np.random.default_rng(3)
    params = [(0.1 * rng.standard_normal(s)).astype(np.float32) for _, s in O.param_shapes(cfg)]
    eps = rng.standard_normal((cfg.L, n, cfg.Z)).astype(np.float32)
    eps3 = rng.standard_normal((3, n, cfg.Z)).astype(np.float32)
    x = (O.synthetic_frey if cfg.continuous else O.synthetic_mnist)(n=n, D=cfg.D, seed=5)

    def run(dt, z0=None):
        p, xx, e, e3 = [q.astype(dt) for q in params], x.astype(dt), eps.astype(dt), eps3.astype(dt)
        out = dict(O.forward_backward(p, xx, e, cfg, need_grad=False))
        out["hd"] = out["hd"].reshape(cfg.L, n, cfg.H)
        out["kl"] = out["la_rows"] if cfg.estimator == "LA" else out["kl_rows"]
        out["recon"] = O.reconstruct(p, xx, None, cfg)
        out["recon3"] = O.reconstruct(p, xx, e3, cfg)
        # decode at the float32 z the device is handed: the float64 run's z[0], rounded
        out["z0"] = out["z"][0].astype(np.float32) if z0 is None else z0
        out["dec_mu"], out["dec_ls"] = O.decode(p, out["z0"].astype(dt), cfg)
        if cfg.continuous:
            out["full0_mu"], out["full0_ls"] = O.reconstruct_full(p, xx, None, cfg)
            out["full3_mu"], out["full3_ls"] = O.reconstruct_full(p, xx, e3, cfg)
        return out

    out64 = run(np.float64)
    out32 = run(np.float32, out64["z0"])
    keys = [k for k in out64 if isinstance(out64[k], np.ndarray) and k not in ("z0", "a3")]
    restate = {k: maxabs(out32[k], out64[k]) for k in keys}
    for a in [x, eps, eps3] + params + [v for v in out64.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return cfg, params, x, eps, eps3, out64, restate


def atol(name, restate, key):
    """1e-5 absolute; at H = 1040 max(1e-5, 16 x the restatement error of that output)."""
    return max(1e-5, 16 * restate[key]) if CASES[name][0]["H"] == 1040 else 1e-5


def context(cfg, params, mer):
    ctx = make_ctx(cfg, B, keep_grads=False, max_eval_rows=mer)
    ctx.set_params(O.flatten(params))
    return ctx


@pytest.mark.parametrize("name,mer", SINGLE, ids=[f"{n}-{m}" for n, m in SINGLE])
def test_validate_activations_and_row_partials(name, mer):
    """validate with host eps, then what the call's last chunk left on the device: activations
    elementwise, the log p and KL / LA partials summed per (sample, row), every pad-row partial
    exactly 0, and the returned sum."""
    cfg, params, x, eps, _, out, restate = case(name)
    n, L, D, H, Z = x.shape[0], cfg.L, cfg.D, cfg.H, cfg.Z
    la = cfg.estimator == "LA"
    r0 = (n - 1) // mer * mer
    nl = n - r0
    Mp, nD, nZ = r16(nl), -(-D // 16), -(-Z // 16)
    ctx = context(cfg, params, mer)
    try:
        ctx.set_eps_mode(1)
        ctx.push_eps(eps)
        v = ctx.validate(x)
        got = {k: ctx.activation(k, Mp * w).reshape(Mp, w)[:nl] for k, w in (("h", H), ("mu", Z), ("lv", Z))}
        got.update({k: ctx.activation(k, L * Mp * w).reshape(L, Mp, w)[:, :nl]
                    for k, w in (("eps", Z), ("z", Z), ("hd", H))})
        lp = ctx.activation("lp_part", L * Mp * nD).reshape(L, Mp, nD)
        kl = ctx.activation("kl_part", (L if la else 1) * Mp * nZ).reshape(L if la else 1, Mp, nZ)
    finally:
        ctx.close()

    rows = slice(r0, n)
    ktol = 16 * restate["kl"]
    msg = [f"{name} mer={mer} (last chunk rows {r0}..{n - 1}, Mp={Mp}):"]
    bad = []
    for k in ("h", "mu", "lv", "z", "hd"):
        want = out[k][..., rows, :]
        e, t = maxabs(got[k], want), atol(name, restate, k)
        msg.append(f"{k} {e:.2e}/{t:.1e} (restatement {restate[k]:.1e})")
        if not e <= t:
            bad.append(k)
    if not np.array_equal(got["eps"], eps[:, rows]):
        bad.append("eps")
    lp_rows = lp.sum(axis=2, dtype=np.float64)[:, :nl]
    want = out["logp_rows"][:, rows]
    e = float((np.abs(lp_rows - want) / np.abs(want)).max())
    msg.append(f"logp rows rel {e:.2e}/1e-4")
    if not np.all(np.abs(lp_rows - want) <= 1e-4 * np.abs(want)):
        bad.append("logp_rows")
    kl_rows = kl.sum(axis=2, dtype=np.float64)[:, :nl]
    want = out["kl"][:, rows] if la else out["kl"][None, rows]
    e = maxabs(kl_rows, want)
    msg.append(f"{'la' if la else 'kl'} rows {e:.2e}/{ktol:.2e} (restatement {restate['kl']:.2e}, "
               f"min |row| {np.abs(want).min():.1e})")
    if not e <= ktol:
        bad.append("kl_rows")
    pad = (int(np.count_nonzero(lp[:, nl:])), int(np.count_nonzero(kl[:, nl:])))
    msg.append(f"non-zero pad partials lp {pad[0]} kl {pad[1]}")
    if pad != (0, 0) or np.isnan(lp[:, nl:]).any() or np.isnan(kl[:, nl:]).any():
        bad.append("pad rows")
    ref = float(out["sgvb"])
    msg.append(f"validate rel {abs(v - ref) / abs(ref):.2e}/1e-4")
    print(" ".join(msg))
    assert not bad, (bad, " ".join(msg))
    assert abs(v - ref) <= 1e-4 * abs(ref), (v, ref)


def planes_eval_eps(seed, step, n, L, Z):
    """[L, n, Z] of the validation stream: row = the row's index in the call, c1 = l * Z + j."""
    return P.eval_eps(seed, step, n, L * Z, 0).reshape(n, L, Z).transpose(1, 0, 2)


@pytest.mark.parametrize("name,mer", CHUNKED, ids=[f"{n}-{m}" for n, m in CHUNKED])
def test_chunked_validate_host_and_philox(name, mer):
    """validate and validate_resident over chunks (a full first chunk, a short last one), with
    host eps and with the device's own draws at L planes, each within 1e-4 relative."""
    from vaeb_amd import _lib
    cfg, params, x, eps, _, out, _ = case(name)
    n = x.shape[0]
    p64 = [p.astype(np.float64) for p in params]
    ctx = context(cfg, params, mer)
    try:
        ctx.set_eps_mode(_lib.EPS_HOST)
        ctx.push_eps(eps)
        ctx.set_valid_data(x)
        got = {"host validate": (ctx.validate(x), float(out["sgvb"])),
               "host resident": (ctx.validate_resident(), float(out["sgvb"]))}
        ctx.set_eps_mode(_lib.EPS_PHILOX, SEED)
        ctx.set_step(STEP)
        step = ctx.get_step()
        ref = float(O.validate(p64, x.astype(np.float64), planes_eval_eps(SEED, step, n, cfg.L, cfg.Z), cfg))
        got["philox validate"] = (ctx.validate(x), ref)
        got["philox resident"] = (ctx.validate_resident(), ref)
        assert ctx.get_step() == step      # evaluation draws at the counter and leaves it
    finally:
        ctx.close()
    print(f"{name} mer={mer}: " + ", ".join(f"{k} rel {abs(v - r) / abs(r):.2e}" for k, (v, r) in got.items()))
    for k, (v, r) in got.items():
        assert abs(v - r) <= 1e-4 * abs(r), (k, v, r)


@pytest.mark.parametrize("name,mer", CHUNKED, ids=[f"{n}-{m}" for n, m in CHUNKED])
def test_per_row_outputs(name, mer):
    """What the ABI returns per row, over the chunked contexts: reconstruct, reconstruct_sampled
    (three host-eps samples), reconstruct_full with its log-sigma head (Gaussian), decode of the
    oracle's z[0], encode."""
    from vaeb_amd import _lib
    cfg, params, x, eps, eps3, out, restate = case(name)
    ctx = context(cfg, params, mer)
    try:
        ctx.set_eps_mode(_lib.EPS_HOST)
        ctx.push_eps(stacked(eps3, L=cfg.L))
        got = {"recon": ctx.reconstruct(x), "recon3": ctx.reconstruct_sampled(x, 3)}
        got["dec_mu"], got["dec_ls"] = ctx.decode(np.asarray(out["z0"], np.float32))
        got["mu"], got["lv"] = ctx.encode(x)
        if cfg.continuous:
            got["full0_mu"], got["full0_ls"] = ctx.reconstruct_full(x, 0)
            got["full3_mu"], got["full3_ls"] = ctx.reconstruct_full(x, 3)
    finally:
        ctx.close()
    if not cfg.continuous:
        assert got.pop("dec_ls") is None
    errs = {k: (maxabs(v, out[k]), atol(name, restate, k)) for k, v in got.items()}
    print(f"{name} mer={mer}: " + ", ".join(f"{k} {e:.2e}/{t:.1e} (restatement {restate[k]:.1e})"
                                            for k, (e, t) in errs.items()))
    for k, (e, t) in errs.items():
        assert got[k].shape == out[k].shape and e <= t, (k, e, t)


# ------------------------------------------------------------------ FV / FVS contexts, the all-reduce arm
# The evaluation calls on the full-variational estimators and behind a one-rank communicator, at
# max_eval_rows = 64 over 2 * 64 + 7 rows (three chunks, the last neither full nor a multiple of
# 16).  FV evaluates the data term at the loaded theta, FVS at the posterior mean mu_theta (copied
# into the spare arena per call); theta and mu_theta differ here, so the wrong arena shows.  Oracle
# functions and tolerances are those of the tests above and of tests/test_gpu_marginal_ll.py
# (validate: n * data + thetaPrior as tests/test_gpu_step.py::test_fv_weight_sampling_step).
EVAL_MER, EVAL_N, EVAL_K = 64, 2 * 64 + 7, 5
EVAL_SHAPES = {"72-40-8": dict(D=72, H=40, Z=8), "64-48-40-gauss": dict(D=64, H=48, Z=40, continuous=True)}


@functools.lru_cache(maxsize=None)
def eval_inputs(shape):
    """cfg (LB), theta, mu_theta, sigma_theta, x, eps [1, n, Z], eps3 [3, n, Z], epsK [K, n, Z]."""
    cfg = O.Config(**EVAL_SHAPES[shape])
    n = EVAL_N
    rng = np.random.default_rng(3)
    theta = [(0.1 * rng.standard_normal(s)).astype(np.float32) for _, s in O.param_shapes(cfg)]
    mu = [(t + 0.05 * rng.standard_normal(t.shape)).astype(np.float32) for t in theta]
    sig = [np.full_like(t, 1e-3) for t in theta]
    eps = rng.standard_normal((1, n, cfg.Z)).astype(np.float32)
    eps3 = rng.standard_normal((3, n, cfg.Z)).astype(np.float32)
    epsK = rng.standard_normal((EVAL_K, n, cfg.Z)).astype(np.float32)
    x = (O.synthetic_frey if cfg.continuous else O.synthetic_mnist)(n=n, D=cfg.D, seed=5)
    for a in [x, eps, eps3, epsK] + theta + mu + sig:
        a.setflags(write=False)
    return cfg, theta, mu, sig, x, eps, eps3, epsK


def check_eval_calls(ctx, cfg, p, prior_of, x, eps, eps3, epsK, what):
    """Every evaluation call of ctx against the float64 oracle at parameters p; prior_of: None, or
    (mu, sigma) of the thetaPrior an FV context adds to n * data."""
    from tests.test_gpu_marginal_ll import RTOL, assert_matches, iw_reference
    from vaeb_amd import _lib
    n = x.shape[0]
    f64 = lambda q: [a.astype(np.float64) for a in q]   # noqa: E731
    p64, x64 = f64(p), x.astype(np.float64)
    out = O.forward_backward(p64, x64, eps.astype(np.float64), cfg, need_grad=False)
    ref_v = float(out["sgvb"])
    if prior_of is not None:
        ref_v = n * ref_v + O.fv_theta_prior(f64(prior_of[0]), f64(prior_of[1]))
    ctx.set_eps_mode(_lib.EPS_HOST)
    ctx.push_eps(eps)
    ctx.set_valid_data(x)
    sums = {"validate": (ctx.validate(x), ref_v), "validate_resident": (ctx.validate_resident(), ref_v)}
    ctx.push_eps(stacked(eps3))
    got = {"recon": ctx.reconstruct(x), "recon3": ctx.reconstruct_sampled(x, 3)}
    want = {"recon": O.reconstruct(p64, x64, None, cfg), "recon3": O.reconstruct(p64, x64, eps3.astype(np.float64), cfg)}
    if cfg.continuous:
        got["full3_mu"], got["full3_ls"] = ctx.reconstruct_full(x, 3)
        want["full3_mu"], want["full3_ls"] = O.reconstruct_full(p64, x64, eps3.astype(np.float64), cfg)
    z0 = out["z"][0].astype(np.float32)
    got["dec_mu"], dec_ls = ctx.decode(z0)
    want["dec_mu"], want_ls = O.decode(p64, z0.astype(np.float64), cfg)
    if cfg.continuous:
        got["dec_ls"], want["dec_ls"] = dec_ls, want_ls
    got["mu"], got["lv"] = ctx.encode(x)
    want["mu"], want["lv"] = out["mu"], out["lv"]
    cfg_la = O.Config(**{**cfg.__dict__, "estimator": "LA"})
    lw, ref_rows = iw_reference(O.forward_backward(p64, x64, epsK.astype(np.float64), cfg_la, need_grad=False), EVAL_K)
    ctx.push_eps(stacked(epsK))
    total, rows = ctx.marginal_ll(x, EVAL_K, rows=True)
    res = ctx.marginal_ll_resident(EVAL_K)
    # the device's own draws: validate and the resident form on stream 0
    ctx.set_eps_mode(_lib.EPS_PHILOX, SEED)
    ctx.set_step(STEP)
    ref_p = float(O.validate(p64, x64, planes_eval_eps(SEED, STEP, n, 1, cfg.Z), cfg))
    if prior_of is not None:
        ref_p = n * ref_p + O.fv_theta_prior(f64(prior_of[0]), f64(prior_of[1]))
    sums["philox validate"] = (ctx.validate(x), ref_p)
    sums["philox resident"] = (ctx.validate_resident(), ref_p)
    errs = {k: maxabs(v, want[k]) for k, v in got.items()}
    print(f"{what}: " + ", ".join(f"{k} rel {abs(v - r) / abs(r):.2e}" for k, (v, r) in sums.items()) + "; " +
          ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    for k, (v, r) in sums.items():
        assert abs(v - r) <= 1e-4 * abs(r), (what, k, v, r)
    for k, e in errs.items():
        assert got[k].shape == want[k].shape and e <= 1e-5, (what, k, e)
    assert_matches(total, rows, ref_rows, f"{what} marginal_ll")
    assert abs(res - ref_rows.sum()) <= RTOL * abs(ref_rows.sum()), (what, res, ref_rows.sum())


@pytest.mark.parametrize("shape", list(EVAL_SHAPES))
@pytest.mark.parametrize("est", ["FV", "FVS"])
def test_full_variational_contexts_evaluate_in_chunks(est, shape):
    cfg, theta, mu, sig, x, eps, eps3, epsK = eval_inputs(shape)
    ctx = make_ctx(O.Config(**{**cfg.__dict__, "estimator": est}), B, keep_grads=False, max_eval_rows=EVAL_MER)
    try:
        zero = np.zeros_like(O.flatten(theta))
        ctx.set_params(O.flatten(theta))
        ctx.set_fv_state(O.flatten(mu), O.flatten(sig), zero, zero)
        check_eval_calls(ctx, cfg, mu if est == "FVS" else theta, (mu, sig), x, eps, eps3, epsK, f"{est} {shape}")
        assert np.array_equal(ctx.get_params(), O.flatten(theta))      # evaluation leaves theta alone
    finally:
        ctx.close()


@pytest.mark.parametrize("shape", list(EVAL_SHAPES))
def test_evaluation_behind_a_one_rank_communicator(shape):
    """validate_resident and marginal_ll_resident all-reduce their sum over the ranks; with one
    rank the share is every row and the sum is unchanged."""
    from vaeb_amd import _lib
    cfg, theta, _, _, x, eps, eps3, epsK = eval_inputs(shape)
    ctx = context(cfg, theta, EVAL_MER)
    try:
        ctx.comm_init(_lib.Context.comm_unique_id(), 0, 1)
        check_eval_calls(ctx, cfg, theta, None, x, eps, eps3, epsK, f"world 1 {shape}")
    finally:
        ctx.close()
