"""The two-mode latent prior of the layer-stack engine (vaeb_ae_config.prior = VAEB_AE_PRIOR_TWO_MODE:
vaeb_amd/csrc/ae_mlp.hpp PAeFwdT<false, true> / PAeBwdT<., true>, ae_iwae.hpp ae_iw_sample_tm_kernel,
ae_codes.hpp, engine_ae.inc) against the float64 oracle (tests/vae_prior_oracle.py) on identical
theta / rows / eps.

Caps, all borrowed and checked on the host in tests/test_vae_prior_host.py (no bound comes from the
device):
  * a step's value: relative <= VALUE_RTOL = 2e-5; theta': check_theta; accumulator norm <= ACC_RTOL = 1e-4
  * per parameter block, the gradient recovered from a zero accumulator: 16 x the float32
    restatement's error (tests/ae_grad_cases.py MARGIN, every bound <= GRAD_CAP = 1e-4)
  * elbo(X), marginal_ll(X, K) over four chunks, and the steps of a width schedule: relative <= 1e-4
  * the binary codes: exact
Every test prints its figures (-s shows them).

Measured on an MI355X.  Single steps (28: 7 cases x 2 forms x 2 eps modes): value within 1.8e-7 of the
oracle.  Per block, device error / restatement error / bound of the block nearest to its bound:

  case                  block    device  / restate / bound      value    worst device / restate
  dz1_m5_bin-elbo       Wzlv     1.6e-07 / 8.8e-08 / 1.4e-06   2.0e-08   1.8
  dz1_m5_bin-iw         bzlv     6.4e-08 / 3.3e-08 / 5.3e-07   5.0e-08   1.9
  dz15_m33_cont-elbo    Wmu      1.2e-07 / 1.1e-07 / 1.8e-06   7.9e-08   1.1
  dz15_m33_cont-iw      bzmu     1.6e-07 / 1.5e-07 / 2.4e-06   4.9e-08   1.1
  dz16_m1_bin-elbo      Wzlv     2.8e-07 / 1.8e-07 / 2.9e-06   4.1e-08   1.5
  dz16_m1_bin-iw        bzlv     2.3e-07 / 3.2e-08 / 5.1e-07   3.6e-08   7.3
  dz17_m5_cont_a2-elbo  bdec0    1.0e-07 / 4.4e-08 / 7.1e-07   3.9e-08   2.3
  dz17_m5_cont_a2-iw    bdec0    1.0e-07 / 6.9e-08 / 1.1e-06   1.8e-07   1.5
  dz33_m33_bin-elbo     benc0    1.8e-07 / 1.3e-07 / 2.0e-06   5.1e-08   1.4
  dz33_m33_bin-iw       Wdec0    1.1e-07 / 1.1e-07 / 1.7e-06   1.3e-09   1.0
  dz33_m5_cont_w05-elbo benc0    1.1e-07 / 7.5e-08 / 1.2e-06   4.8e-09   1.4
  dz33_m5_cont_w05-iw   bzlv     2.0e-07 / 1.3e-07 / 2.2e-06   1.6e-08   1.5
  mnist_like-elbo       Wenc0    1.4e-07 / 1.9e-07 / 3.1e-06   1.6e-08   0.7
  mnist_like-iw         bout     2.8e-07 / 4.2e-07 / 6.6e-06   1.4e-08   0.7

elbo / marginal_ll over four chunks: 5.1e-8 and 8.8e-8 from the oracle, rows equal for max_batch 7,
15 and 64.  Two-mode at (0, 1) against a normal context: rows and the step's value equal, theta' within
3.2e-7.  The t = 1000 element: value 9e-9 from the oracle.  Width schedule: worst value 1.1e-7; the
fourth step lies 0.77 (relative) from the old width's oracle.  No cap was widened and no kernel changed
after the first run; the one assert that failed on it was this file's own guard in the MASK test
(clean and corrupted oracle values apart by > 100 x the cap: they are 17 x apart in the ELBO form),
now 10 x.
"""
import numpy as np
import pytest

from oracle import ae_oracle as A
from tests import ae_grad_cases as G
from tests import vae_prior_cases as C
from tests import vae_prior_oracle as PO
from tests import vae_stack_oracle as V
from tests.test_gpu_ae import check_theta
from tests.test_gpu_vae_stack import assert_step as assert_step_caps
from tests.test_vae_stack_host import ACC_RTOL, SEED, STEP, VALUE_RTOL

pytestmark = pytest.mark.gpu

EVAL_RTOL = 1e-4


def make_ctx(cfg, max_batch, prior="twomode", latent="gauss", iw_samples=1, corruption="none"):
    from vaeb_amd import _lib
    return _lib.AEContext(cfg.Dobs, cfg.Denc, cfg.Dz, cfg.Ddec, otype=cfg.otype, act=cfg.act, s2=cfg.s2,
                          eta=cfg.eta, max_batch=max_batch, latent=latent, iw_samples=iw_samples,
                          corruption=corruption, prior=prior)


def stacked(eps):
    """[K, n, Dz] (or [n, Dz]) -> the push: sample k of list position i at row k n + i."""
    return np.ascontiguousarray(eps, np.float32).reshape(-1, eps.shape[-1])


def case_ctx(name, form, **kw):
    """A two-mode context of the case at its prior, with its data: (ctx, case, K of the context)."""
    cfg, Xtr, idx, params, eps = C.inputs(name)
    c = C.CASE[name]
    K = c.K if form == "iw" else 1
    ctx = make_ctx(cfg, K * c.M, iw_samples=K, **kw)
    ctx.set_data(Xtr)
    ctx.set_prior(c.mean1, c.width)
    return ctx, c, K


# ------------------------------------------------------------------ 1. single steps
@pytest.mark.parametrize("mode", ["host", "philox"])
@pytest.mark.parametrize("name,form", C.STEPS, ids=C.STEP_IDS)
def test_single_step_against_the_oracle(name, form, mode):
    from vaeb_amd import _lib
    cfg, Xtr, idx, params, eps = C.inputs(name)
    acc = C.acc0(params)
    ctx, c, K = case_ctx(name, form)
    try:
        assert ctx.get_prior() == (np.float32(c.mean1), np.float32(c.width))
        ctx.set_params(A.flatten(params))
        ctx.set_adagrad_state(A.flatten(acc))
        if mode == "host":
            e = eps[form]
            ctx.set_eps_mode(_lib.EPS_HOST)
            ctx.push_eps(stacked(e))
        else:
            e = PO.train_eps(SEED, idx, cfg.Dz, STEP, form, K)
            ctx.set_eps_mode(_lib.EPS_PHILOX, SEED)
        ctx.set_step(STEP)
        got = ctx.train(idx)
        ref, ref_p, ref_a, _ = C.step64(cfg, Xtr, params, acc, idx, e, c.mean1, c.width, form)
        print(f"{name}-{form}-{mode}: value device {got:.6f} oracle {ref:.6f} rel {abs(got - ref) / abs(ref):.1e}")
        assert_step_caps(ctx, got, ref, ref_p, ref_a, cfg.eta)
        assert ctx.get_step() == STEP + 1
    finally:
        ctx.close()


# ------------------------------------------------------------------ 2. per-element gradients
@pytest.mark.parametrize("name,form", C.STEPS, ids=C.STEP_IDS)
def test_gradient_per_block(name, form):
    from vaeb_amd import _lib
    st = C.step(name, form)
    ctx, c, K = case_ctx(name, form)
    try:
        assert ctx.P == sum(int(np.prod(s)) for _, s in st.shapes)
        ctx.set_params(st.theta())
        ctx.set_adagrad_state(np.zeros(ctx.P, np.float32))
        ctx.set_eps_mode(_lib.EPS_HOST)
        ctx.push_eps(stacked(st.eps))
        v = ctx.train(st.idx)
        th1, ac1 = ctx.get_params(), ctx.get_adagrad_state()
    finally:
        ctx.close()
    err = st.device_errors(th1, ac1)
    vrel = abs(v - st.value64) / abs(st.value64)
    ratio = max(err[n] / st.restate[n] for n in err)
    print(G.table_line(f"{name}-{form}", err, st.bound, st.restate) + f"   value {vrel:.1e}   worst ratio {ratio:.1f}")
    bad = G.rejected(err, st.bound)
    assert not bad, {n: (err[n], st.restate[n], st.bound[n]) for n in bad}
    assert vrel <= VALUE_RTOL, (v, st.value64)


# ------------------------------------------------------------------ 3. the value calls
def eval_setup(name, B):
    """n = 3 B + 2 rows (four chunks, the last partial), eps for elbo [n, Dz] and marginal_ll [K, n, Dz]."""
    cfg, _, _, params, _ = C.inputs(name)
    c = C.CASE[name]
    n = 3 * B + 2
    X = G.data_for(cfg, n, 77)
    rng = np.random.default_rng(78)
    return cfg, c, params, X, rng.standard_normal((n, cfg.Dz)).astype(np.float32), \
        rng.standard_normal((3, n, cfg.Dz)).astype(np.float32)


@pytest.mark.parametrize("name", ["dz17_m5_cont_a2", "dz33_m33_bin"])
def test_elbo_and_marginal_ll_over_four_chunks(name):
    from vaeb_amd import _lib
    B = 7
    cfg, c, params, X, e1, e3 = eval_setup(name, B)
    ref_elbo = C.oracle(cfg, params, X, e1, c.mean1, c.width, "elbo", np.float64, need_grad=False)["value"]
    ref_iw = C.oracle(cfg, params, X, e3, c.mean1, c.width, "iw", np.float64, need_grad=False)
    rows_by_batch = []
    for mb in (B, 2 * B + 1, 64):
        ctx = make_ctx(cfg, mb)
        try:
            ctx.set_params(A.flatten(params))
            ctx.set_prior(c.mean1, c.width)
            ctx.set_eps_mode(_lib.EPS_HOST)
            ctx.push_eps(e1)
            elbo = ctx.elbo(X)
            ctx.push_eps(stacked(e3))
            ml, rows = ctx.marginal_ll(X, 3, rows=True)
        finally:
            ctx.close()
        print(f"{name} max_batch {mb}: elbo rel {abs(elbo - ref_elbo) / abs(ref_elbo):.1e}, marginal_ll rel "
              f"{abs(ml - ref_iw['value']) / abs(ref_iw['value']):.1e}, rows {np.abs(rows - ref_iw['rows']).max():.1e}")
        assert abs(elbo - ref_elbo) <= EVAL_RTOL * abs(ref_elbo)
        assert abs(ml - ref_iw["value"]) <= EVAL_RTOL * abs(ref_iw["value"])
        assert np.all(np.abs(rows - ref_iw["rows"]) <= EVAL_RTOL * np.abs(ref_iw["rows"]))
        rows_by_batch.append(rows)
    assert np.array_equal(rows_by_batch[0], rows_by_batch[1]) and np.array_equal(rows_by_batch[0], rows_by_batch[2])


# ------------------------------------------------------------------ 4. a = 0, s = 1
def test_two_mode_at_0_1_is_the_normal_prior_in_the_iw_forms():
    """Same theta, rows and eps on a two-mode context at (0, 1) and on a normal one: marginal_ll's rows
    and one iw_samples = 3 step agree to the step caps (not bitwise: the arithmetic differs)."""
    from vaeb_amd import _lib
    name = "dz17_m5_cont_a2"
    cfg, Xtr, idx, params, eps = C.inputs(name)
    acc = C.acc0(params)
    M, K = len(idx), 3
    res = []
    for prior in ("twomode", "normal"):
        ctx = make_ctx(cfg, K * M, prior=prior, iw_samples=K)
        try:
            if prior == "twomode":
                ctx.set_prior(0.0, 1.0)
            ctx.set_data(Xtr)
            ctx.set_params(A.flatten(params))
            ctx.set_adagrad_state(A.flatten(acc))
            ctx.set_eps_mode(_lib.EPS_HOST)
            ctx.push_eps(stacked(eps["iw"]))
            ml, rows = ctx.marginal_ll(Xtr[idx], K, rows=True)
            v = ctx.train(idx)
            res.append((ml, rows, v, ctx.get_params(), ctx.get_adagrad_state()))
        finally:
            ctx.close()
    (ml2, rows2, v2, th2, ac2), (ml1, rows1, v1, th1, ac1) = res
    print(f"marginal_ll rows rel {np.abs(rows2 - rows1).max() / np.abs(rows1).max():.1e}; step value rel "
          f"{abs(v2 - v1) / abs(v1):.1e}; theta' max diff {np.abs(th2 - th1).max():.1e}")
    assert np.all(np.abs(rows2 - rows1) <= VALUE_RTOL * np.abs(rows1))
    assert abs(ml2 - ml1) <= VALUE_RTOL * abs(ml1) and abs(v2 - v1) <= VALUE_RTOL * abs(v1)
    check_theta(th2, th1, cfg.eta)
    assert np.linalg.norm(ac2.astype(np.float64) - ac1) <= ACC_RTOL * np.linalg.norm(ac1.astype(np.float64))


# ------------------------------------------------------------------ 5. the overflow element
def test_overflow_element_is_finite_and_matches_the_oracle():
    """Width 0.05 and a latent held at z = 3: t = 1000, where log(1 + e^t) is inf in float32."""
    from vaeb_amd import _lib
    name = "dz16_m1_bin"
    cfg, Xtr, idx, params, eps = C.inputs(name)
    c = C.CASE[name]
    assert c.width == 0.05 and c.mean1 == 1.0
    params = [q.copy() for q in params]
    p = dict(zip(V.names(cfg), params))
    p["Wzmu"][:, 0] = 0.0
    p["Wzlv"][:, 0] = 0.0
    p["bzmu"][0], p["bzlv"][0] = 3.0, -30.0
    acc = C.acc0(params)
    out = C.oracle(cfg, params, Xtr[idx], eps["elbo"], c.mean1, c.width, "elbo", np.float64, need_grad=False)
    assert abs(out["t"][0, 0, 0] - 1000.0) < 1e-3
    for form in PO.FORMS:
        ctx, _, K = case_ctx(name, form)
        try:
            ctx.set_params(A.flatten(params))
            ctx.set_adagrad_state(A.flatten(acc))
            ctx.set_eps_mode(_lib.EPS_HOST)
            ctx.push_eps(stacked(eps[form]))
            ml = ctx.marginal_ll(Xtr[idx], 1) if form == "elbo" else None
            got = ctx.train(idx)
            ref, ref_p, ref_a, _ = C.step64(cfg, Xtr, params, acc, idx, eps[form], c.mean1, c.width, form)
            print(f"overflow-{form}: value device {got:.5f} oracle {ref:.5f} rel {abs(got - ref) / abs(ref):.1e}")
            assert np.isfinite(got) and np.isfinite(ctx.get_params()).all()
            assert_step_caps(ctx, got, ref, ref_p, ref_a, cfg.eta)
            if ml is not None:          # marginal_ll's form of the same term, K = 1
                r1 = C.oracle(cfg, params, Xtr[idx], eps["elbo"][None], c.mean1, c.width, "iw", np.float64,
                              need_grad=False)["value"]
                assert np.isfinite(ml) and abs(ml - r1) <= EVAL_RTOL * abs(r1)
        finally:
            ctx.close()


# ------------------------------------------------------------------ 6. a schedule of widths
def test_width_schedule_between_train_many_calls():
    """Two train_many calls of three steps, set_prior between them: every value tracks the oracle's
    trajectory, the step counter advances as ever, and the fourth step is the new width's."""
    from vaeb_amd import _lib
    name = "dz15_m33_cont"
    cfg, Xtr, idx, params, _ = C.inputs(name)
    B, widths = 11, (0.5, 0.1)
    a = C.CASE[name].mean1
    ctx = make_ctx(cfg, B)
    try:
        ctx.set_data(Xtr)
        ctx.set_params(A.flatten(params))
        ctx.set_eps_mode(_lib.EPS_PHILOX, SEED)
        ctx.set_step(STEP)
        got = []
        for w in widths:
            ctx.set_prior(a, w)
            assert ctx.get_prior() == (np.float32(a), np.float32(w))
            got += list(ctx.train_many(idx, B))
        assert ctx.get_step() == STEP + 6
    finally:
        ctx.close()
    p = [q.astype(np.float64) for q in params]
    acc = [np.zeros_like(q) for q in p]
    X64 = Xtr.astype(np.float64)
    ref, old_width_4th = [], None
    for j in range(6):
        sl = idx[(j % 3) * B:(j % 3 + 1) * B]
        e = PO.train_eps(SEED, sl, cfg.Dz, STEP + j, "elbo")
        if j == 3:
            old_width_4th = PO.train_step(p, acc, X64, sl, e, cfg, a, widths[0], "elbo")[0]
        v, p, acc, _ = PO.train_step(p, acc, X64, sl, e, cfg, a, widths[j // 3], "elbo")
        ref.append(v)
    rel = [abs(g - r) / abs(r) for g, r in zip(got, ref)]
    print("schedule: worst value rel %.1e; 4th step against the old width's oracle %.1e" %
          (max(rel), abs(got[3] - old_width_4th) / abs(old_width_4th)))
    assert max(rel) <= EVAL_RTOL
    assert abs(got[3] - old_width_4th) > 100 * EVAL_RTOL * abs(old_width_4th)


# ------------------------------------------------------------------ 7. with corruption
@pytest.mark.parametrize("form", PO.FORMS)
def test_mask_corrupted_two_mode_step(form):
    """The oracle is fed vaeb_ae_corrupt's rows as the encoder's input and the clean rows as the
    observations.  The two oracle values, corrupted and clean, lie 3.5e-4 (ELBO form) and 2.9e-2 (IW
    form) apart, 17 and 1400 times the value's cap."""
    from vaeb_amd import _lib
    name = "dz17_m5_cont_a2"
    cfg, Xtr, idx, params, eps = C.inputs(name)
    acc = C.acc0(params)
    ctx, c, K = case_ctx(name, form, corruption="mask")
    try:
        ctx.set_params(A.flatten(params))
        ctx.set_adagrad_state(A.flatten(acc))
        ctx.set_eps_mode(_lib.EPS_HOST)
        ctx.push_eps(stacked(eps[form]))
        ctx.set_corruption_noise(_lib.EPS_PHILOX, 99)
        ctx.set_corruption_level(0.3)
        ctx.set_step(STEP)
        xt = ctx.corrupt(idx)
        masked = float((xt != Xtr[idx]).mean())
        assert 0.15 < masked < 0.45 and np.all((xt == 0) | (xt == Xtr[idx]))
        got = ctx.train(idx)
        ref, ref_p, ref_a, _ = C.step64(cfg, Xtr, params, acc, idx, eps[form], c.mean1, c.width, form, Xenc=xt)
        clean = C.step64(cfg, Xtr, params, acc, idx, eps[form], c.mean1, c.width, form)[0]
        print(f"mask-{form}: value device {got:.6f} oracle {ref:.6f} (clean {clean:.6f}), masked {masked:.2f}")
        assert abs(clean - ref) > 10 * VALUE_RTOL * abs(ref)      # an encoder fed the clean rows would miss the cap
        assert_step_caps(ctx, got, ref, ref_p, ref_a, cfg.eta)
        assert ctx.get_step() == STEP + 1
    finally:
        ctx.close()


# ------------------------------------------------------------------ 8. binary codes
@pytest.mark.parametrize("Dz,a", [(1, 1.0), (31, 1.0), (32, 2.0), (33, -1.5)])
def test_codes_are_exact(Dz, a):
    """n spans three chunks, the last partial.  encode_bits is encode(X) >= a / 2 bit for bit (the
    same kernels give the same mu: no tolerance, no element left out), the padding bits are 0, and
    decode_bits is bitwise decode of the 0 / a matrix."""
    cfg = A.AEConfig(Dobs=40, Denc=(24,), Dz=Dz, Ddec=(20,), otype="binary")
    B, n = 9, 2 * 9 + 4
    params = C.scale_params(cfg, V.init_params(cfg, seed=5))
    rng = np.random.default_rng(Dz)
    p = dict(zip(V.names(cfg), params))
    p["bzmu"][:] = (a * rng.uniform(-0.5, 1.5, Dz)).astype(np.float32)
    X = G.data_for(cfg, n, 9)
    ctx = make_ctx(cfg, B)
    try:
        ctx.set_params(A.flatten(params))
        ctx.set_prior(a, 0.1)
        before = ctx.get_params()
        words = ctx.encode_bits(X)
        mu = ctx.encode(X)
        nw = -(-Dz // 32)
        assert words.shape == (n, nw) and words.dtype == np.uint32
        j = np.arange(Dz)
        bits = ((words[:, j // 32] >> (j % 32).astype(np.uint32)) & 1).astype(bool)
        want = mu >= np.float32(0.5) * np.float32(a)
        assert np.array_equal(bits, want)
        assert 0.2 < want.mean() < 0.8 or Dz == 1
        if Dz % 32:
            assert not (words[:, -1] >> np.uint32(Dz % 32)).any()
        z = np.where(bits, np.float32(a), np.float32(0)).astype(np.float32)
        out, ref = ctx.decode_bits(words), ctx.decode(z)
        assert out.shape == (n, cfg.Dobs) and np.array_equal(out, ref)
        # a word of all ones past Dz decodes as its low bits
        if Dz % 32:
            dirty = words.copy()
            dirty[:, -1] |= np.uint32((0xFFFFFFFF << (Dz % 32)) & 0xFFFFFFFF)
            assert np.array_equal(ctx.decode_bits(dirty), ref)
        assert np.array_equal(ctx.get_params(), before)
    finally:
        ctx.close()


def test_construct_vae_two_mode():
    from vaeb_amd import ae
    cfg = A.AEConfig(Dobs=64, Denc=(16,), Dz=5, Ddec=(16,), otype="binary")
    X = G.data_for(cfg, 250, 3)
    np.random.seed(15485863)
    train, reconstruct, encode, decode, theta = ae.ConstructVAE(X, Denc=[16], Dz=5, Ddec=[16], prior=("twomode", 0.5))
    assert train.prior == (1.0, 0.5) and train.code_bits_per_row == 5 and train.iw_samples == 1
    train.set_prior(width=0.25)
    assert train.prior == (1.0, 0.25)
    train.set_prior(mean1=2.0)
    assert train.prior == (2.0, 0.25)
    with pytest.raises(Exception, match="error -1"):
        train.set_prior(width=1e-4)
    assert train.prior == (2.0, 0.25)
    vals = ae.train_epochs(train, X.shape[0], 2, batch_size=100, verbose=False)
    assert len(vals) == 6 and np.isfinite(vals).all() and train.ctx.get_step() == 6
    code = train.code(X)
    assert code.shape == (250, 5) and code.dtype == bool
    assert np.array_equal(code, encode(X) >= np.float32(1.0))
    z = np.where(code, np.float32(2.0), np.float32(0)).astype(np.float32)
    assert np.array_equal(train.decode_code(code), decode(z))
    assert np.array_equal(train.decode_code(code.astype(np.int64)), decode(z))
    with pytest.raises(ValueError):
        train.decode_code(np.full((3, 5), 2))
    assert np.isfinite(train.elbo(X)) and np.isfinite(train.marginal_ll(X, 3))
    # prior=None is the constructor as it was: the same theta_0 draws, context and steps
    outs = []
    for kw in ({}, {"prior": None}):
        np.random.seed(7)
        t2 = ae.ConstructVAE(X, Denc=[16], Dz=5, Ddec=[16], **kw)[0]
        assert t2.ctx.prior == "normal" and not hasattr(t2, "code")
        outs.append((ae.train_epochs(t2, X.shape[0], 1, batch_size=100, verbose=False), t2.ctx.get_params()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


# ------------------------------------------------------------------ 9. errors
def test_error_codes():
    from vaeb_amd import _lib
    cfg = A.AEConfig(Dobs=24, Denc=(12,), Dz=3, Ddec=(12,), otype="binary")
    X = G.data_for(cfg, 6, 0)
    words = np.zeros((6, 1), np.uint32)
    for kw in (dict(prior="normal"), dict(prior="normal", latent="point"), dict(prior="normal", latent="act")):
        ctx = make_ctx(cfg, 4, **kw)
        try:
            for call in (lambda: ctx.set_prior(1.0, 0.25), ctx.get_prior, lambda: ctx.encode_bits(X),
                         lambda: ctx.decode_bits(words)):
                with pytest.raises(_lib.VaebError, match=r"error -1\b.*TWO_MODE"):
                    call()
        finally:
            ctx.close()
    for latent in ("point", "act"):
        with pytest.raises(_lib.VaebError, match=r"error -1\b.*prior"):
            make_ctx(cfg, 4, latent=latent)
    ctx = make_ctx(cfg, 4)
    try:
        assert ctx.get_prior() == (1.0, 0.25)                     # after create
        ctx.set_prior(-2.0, 0.5)
        for a, s in ((float("nan"), 0.5), (float("inf"), 0.5), (1001.0, 0.5), (1.0, 0.0), (1.0, 9e-4), (1.0, 1001.0),
                     (1.0, float("nan")), (1.0, -0.25)):
            with pytest.raises(_lib.VaebError, match=r"error -1\b"):
                ctx.set_prior(a, s)
            assert ctx.get_prior() == (-2.0, 0.5)
        ctx.set_prior(1e3, 1e-3)
        ctx.set_prior(-1e3, 1e3)
        L, h = ctx.lib, ctx.h
        import ctypes
        fp, wp = X.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        out = np.zeros((6, 24), np.float32)
        op = out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        assert L.vaeb_ae_encode_bits(h, fp, 0, wp) == -1 and L.vaeb_ae_encode_bits(h, None, 6, wp) == -1
        assert L.vaeb_ae_encode_bits(h, fp, 6, None) == -1 and L.vaeb_ae_encode_bits(h, fp, -1, wp) == -1
        assert L.vaeb_ae_decode_bits(h, wp, 0, op) == -1 and L.vaeb_ae_decode_bits(h, None, 6, op) == -1
        assert L.vaeb_ae_decode_bits(h, wp, 6, None) == -1
        assert L.vaeb_ae_get_prior(h, None, None) == -1
    finally:
        ctx.close()
