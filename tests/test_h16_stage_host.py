"""Host checks (no GPU) of the 16-bit engine's per-stage test (tests/h16_stage_cases.py,
tests/test_gpu_h16_stage.py): that its inputs are fair, that its criterion accepts a float32
restatement of every stage, and that it rejects what today's criterion lets through.

The device's stand-in is h16_stage_cases.simulate: every stage in float32 from its own 16-bit stored
operands, free running.  A mutant changes one stage of that stand-in; everything downstream is then
computed from the mutated stored buffer, as a device with that bug would.

Raised tau (test_raised_tau_rests_on_the_kernels_tanh).  With the epilogue's own tanh (ftanh_bf restated in
float32 NumPy) the stand-in exceeds the unraised tau at exactly the RAISED stages -- h and hd at theta_0, by
1.0e-6 .. 1.2e-6 beyond half an ulp against tau = 3.2e-7 .. 5.8e-7 -- and nowhere at x30; the restatement's error
is 1.27e-6 = (2^-6)^3 / 3, what the kernel's comment states.

Mutants (each one stage's output):
  corner  the tile-corner element (row 15 mod 16, column 15 mod 16) of dA2 that differs most from the
          row below takes that row's value (displaced by one row);
  tanh1   tanh' taken as 1 where |hd| > 0.95, in dA1;
  swap    dA2 and dA6 exchanged in the 32-column group 1 of the Gaussian dA (columns 32..63);
  scale   fp16, mean objective: the latent terms of [dMu | dLv] joined without the loss scale in one
          16-row block;
  explv2  exp(lv / 2) to second order (1 + a + a^2 / 2, a = lv / 2) in z;
  dropk   the last K block (K = L B, K % 32 != 0 rows) left out of the first 16 x 16 tile of gW2.
"Today" is the criterion of tests/test_gpu_bf16.py / test_gpu_fp16.py: every data-gradient block
norm-wise within 2e-3 of the rounded float64 oracle.  It is applied to the mutated stand-in in the SAME
x30 state in which the stage criterion then judges it (scaled weights amplify what a wrong stored element
does downstream: one element of dA2 wrong by its whole value moves gW1 by 3e-3 .. 4e-2 there, more than
the gW2 it is a factor of).  Every mutant must pass today's criterion and be rejected by the stage
criterion at the stage it was made in, and at no other (teacher forcing).  Where a mutant's full form does
not pass today's, the next smaller form of the same kind is taken and the form used is printed: a form is
(extent, share) -- the extent shrinks first (tanh1 / explv2: everywhere, the first 16 x 16 tile, its last
4 x 4 elements, the one element it changes most in units of its own size; swap: all rows, 16 rows, 1 row, one element pair; scale:
16, 4, 1 rows; dropk: a 16 x 16 ... 1 x 1 tile), then the share of the mutant's change that is applied
(1/2 ... 1/4096).  Each test prints: the form, today's norm-wise figure (and the unmutated stand-in's), the
stages rejected, and the mutated stage's worst element as error beyond half an ulp / float32 restatement
/ bound.
"""
import numpy as np
import pytest

from tests import h16_stage_cases as C

X30_NAMES = list(C.SHAPES)
CASE_DT = pytest.mark.parametrize("dtype", C.DTYPES)


class Mutant:
    """mutate argument of C.simulate: fn(stage, value, dev) -> value, and the attributes that reach
    inside a stage (std_fn, dtanh_hd, swap, drop_k)."""

    def __init__(self, fn=None, **attrs):
        self.fn = fn
        self.__dict__.update(attrs)

    def __call__(self, stage, v, dev):
        return self.fn(stage, v, dev) if self.fn else v


def corner(c, dtype, extent, share):
    def fn(stage, v, dev):
        if stage == "dA2":
            r, col = np.arange(15, v.shape[0] - 1, 16), np.arange(15, v.shape[1], 16)
            d = np.abs(v[r][:, col] - v[r + 1][:, col])
            i, j = np.unravel_index(int(np.argmax(d)), d.shape)
            assert d[i, j] > 0
            v[r[i], col[j]] += v.dtype.type(share) * (v[r[i] + 1, col[j]] - v[r[i], col[j]])
        return v
    return Mutant(fn)


def tanh1(c, dtype, extent, share):
    return Mutant(dtanh_hd=lambda hd: np.where(np.abs(hd) > 0.95, hd.dtype.type(1), 1 - hd * hd), region=extent, amp=share)


def swap(c, dtype, extent, share):
    rows, cols = {"all": (slice(None), slice(32, 64)), "16 rows": (slice(0, 16), slice(32, 64)),
                  "1 row": (slice(15, 16), slice(32, 64)), "1 pair": (slice(15, 16), slice(47, 48))}[extent]
    return Mutant(swap=(rows, cols), amp=share)


def scale(c, dtype, extent, share):
    S = C.loss_scale(c.cfg, c.B, dtype)
    sc = 1.0 / c.B

    def fn(stage, v, dev):
        if stage == "dml":
            mu, lv = dev["mu"], dev["lv"]
            lat = np.concatenate([-sc * S * mu, sc * S * 0.5 * (1 - np.exp(lv))], axis=1)   # LB, L = 1
            v[16:16 + extent] -= (share * lat[16:16 + extent] * (1 - 1 / S)).astype(v.dtype)
        return v
    return Mutant(fn)


def explv2(c, dtype, extent, share):
    return Mutant(std_fn=lambda lv: 1 + lv / 2 + (lv / 2) * (lv / 2) / 2, region=extent, amp=share)


def dropk(c, dtype, extent, share):
    return Mutant(drop_k=("gW2", extent, (c.cfg.L * c.B) % 32))


SHARES = tuple(0.5 ** k for k in range(1, 13))        # 1/2 .. 1/4096


def forms(extents, shares=SHARES):
    """Every extent at the mutant's full change, then the smallest extent at falling shares of it."""
    return [(e, 1.0) for e in extents] + [(extents[-1], s) for s in shares]


REGIONS = ("all", "tile", "4x4", "1")        # h16_stage_cases.region_mask

# mutant: (builder, the stages it is made in, its forms from the full one down, where it applies)
MUTANTS = {
    "corner": (corner, ("dA2",), forms((1,)), lambda cfg, B, dt: True),
    "tanh1": (tanh1, ("dA1",), forms(REGIONS), lambda cfg, B, dt: True),
    "swap": (swap, ("dA2", "dA6"), forms(("all", "16 rows", "1 row", "1 pair")), lambda cfg, B, dt: cfg.continuous),
    "scale": (scale, ("dml",), forms((16, 4, 1)), lambda cfg, B, dt: C.loss_scale(cfg, B, dt) != 1.0),
    "explv2": (explv2, ("z",), forms(REGIONS), lambda cfg, B, dt: True),
    "dropk": (dropk, ("gW2",), forms((16, 8, 4, 2, 1), ()), lambda cfg, B, dt: (cfg.L * B) % 32 != 0),
}
MUTANT_CASES = [(m, n, dt) for m, (_, _, _, ok) in MUTANTS.items() for n in X30_NAMES for dt in C.DTYPES
                if ok(C.config(n), C.batch(n), dt)]


def today(c, dtype, grads):
    """{block: norm-wise error against the rounded float64 oracle}: today's measure."""
    og, _ = C.oracle_grads(c, dtype)
    return {k: C.today_rel(grads[k], og[k]) for k in og}


# ------------------------------------------------------------------ 1. the inputs
@pytest.mark.parametrize("name,state", C.CASES, ids=C.CASE_IDS)
def test_fair_seed_exists(name, state):
    c = C.case(name, state)
    s = c.stats
    print(f"{name}-{state} (seed {c.seed}): " + " ".join(f"{k} {v:.3g}" for k, v in s.items()))
    assert C.SEED0 <= c.seed < C.SEED0 + C.MAX_SEEDS
    assert C.fair(name, state, c.seed)[0] == []
    assert s["store_max"] <= C.F16_MAX
    if state == "x30":
        # the conditions spelled out, so that a change to fair_reasons cannot empty them
        assert s["h_sat"] >= 0.05 and s["hd_sat"] >= 0.05 and s["hd_open"] >= 0.4
        assert 1.0 <= s["lv_max"] <= 8.0 and s["y_min"] < 0.2 and s["y_max"] > 0.8
        if c.cfg.continuous:
            assert s["a6_min"] < -1.0 and s["a6_max"] > 1.0 and max(-s["a6_min"], s["a6_max"]) <= 12.0
    else:
        assert s["h_sat"] == 0 and s["hd_sat"] == 0 and s["lv_max"] < 0.1 and s["y_off"] < 0.05
    assert all(np.all(a == np.float32(C.ACC0)) for a in c.acc)


@pytest.mark.parametrize("name", [n for n in C.SHAPES if C.config(n).Z >= C.W1_DAMP])
def test_w1_damping_is_needed(name):
    """The rule recorded in the helper for Z >= 128: without the further sqrt(64 / Z) on W1, b1 the
    decoder's hidden layer saturates (the share of |hd| < 0.99 is below 0.4 at the first seeds)."""
    damp, C.W1_DAMP = C.W1_DAMP, 1 << 30
    try:
        figures = [C.fair(name, "x30", seed) for seed in range(C.SEED0, C.SEED0 + 3)]
    finally:
        C.W1_DAMP = damp
    print(name, "without the damping: hd_open", [round(s["hd_open"], 3) for _, s in figures])
    assert all(s["hd_open"] < 0.4 for _, s in figures)
    assert C.case(name, "x30").stats["hd_open"] >= 0.4


def test_formats_round_like_the_oracle():
    rng = np.random.default_rng(0)
    a = np.concatenate([rng.standard_normal(4096) * 10.0 ** rng.integers(-9, 4, 4096), [0.0, 65504.0, 2.0 ** -14, 2.0 ** -24,
                        3 * 2.0 ** -25, 1.0, 1.0 - 2.0 ** -9, 1.0 + 2.0 ** -8]]).astype(np.float32)
    for dtype, q in (("bf16", C.O.bf16_round), ("fp16", C.O.fp16_round)):
        sel = a if dtype == "bf16" else a[np.abs(a) <= 65504.0]
        v = C.store16(sel, dtype)
        assert np.array_equal(v, q(sel.astype(np.float64)))
        t = sel.astype(np.float64)
        assert np.all(np.abs(v - t) <= 0.5 * C.ulp16(t, dtype))
        # the spacing itself: the next representable value above |v| is one ulp16 away
        u = C.to_bits(np.abs(sel), dtype)
        nxt = C.from_bits((u + 1).astype(np.uint16), dtype)
        ok = np.isfinite(nxt)
        assert np.array_equal((nxt - C.from_bits(u, dtype))[ok], C.ulp16(C.from_bits(u, dtype), dtype)[ok])


def test_deinterleave_follows_the_shadow_rule():
    D, rows = 96, 3
    dA = np.zeros((rows, 2 * D))
    for d in range(D):
        dA[:, 64 * (d // 32) + d % 32] = d           # h16_common.hpp ShadowMap::at, w6 = false
        dA[:, 64 * (d // 32) + 32 + d % 32] = 1000 + d
    a2, a6 = C.deinterleave(dA, D)
    assert np.array_equal(a2[0], np.arange(D)) and np.array_equal(a6[0], 1000 + np.arange(D))


# ------------------------------------------------------------------ 2. the criterion accepts the restatement
@CASE_DT
@pytest.mark.parametrize("name,state", C.CASES, ids=C.CASE_IDS)
def test_criterion_accepts_the_float32_restatement(name, state, dtype):
    c = C.case(name, state)
    dev, grads = C.simulate(c, dtype)
    f = C.judge(c, dtype, dev, grads)
    t = today(c, dtype, grads)
    print(C.table_line(f"{name}-{state}-{dtype} float32 stand-in", f) + f"  |  today's norm-wise {max(t.values()):.1e}")
    assert [x.stage for x in f if x.kind == "stored"] == [k for k in C.STORED if k != "dA6" or c.cfg.continuous]
    assert {x.stage for x in f if x.kind != "stored"} == {"mulv"} | {"g" + n for n in c.cfg.names}
    assert C.rejected(f) == [], [x.line() for x in C.rejected(f)]
    assert max(t.values()) <= C.TODAY_GRAD
    assert all(x.bound > 0 for x in f)


@CASE_DT
@pytest.mark.parametrize("name,state", C.CASES, ids=C.CASE_IDS)
def test_raised_tau_rests_on_the_kernels_tanh(name, state, dtype):
    """RAISED: the stand-in with the kernel's own tanh (ftanh_bf in float32 NumPy) exceeds the unraised
    tau exactly at the RAISED stages of the case (and nowhere at x30), by the figures recorded there, and
    passes with tau = MARGIN x that restatement's error."""
    c = C.case(name, state)
    dev, grads = C.simulate(c, dtype, Mutant(tanh=C.ftanh_bf))
    plain = {x.stage: x for x in C.judge(c, dtype, dev, grads, raised=False)}
    over = {s for s, x in plain.items() if not x.dev <= x.bound}
    want = {k[3] for k in C.RAISED if k[:3] == (name, state, dtype)}
    for s in sorted(over | want):
        print(f"{name}-{state}-{dtype} {s}: kernel tanh beyond half an ulp {plain[s].dev:.3e}, unraised tau {plain[s].bound:.3e}")
    assert over == want and (state == "theta0" or not want)
    f = {x.stage: x for x in C.judge(c, dtype, dev, grads)}
    assert C.rejected(list(f.values())) == []
    for s in want:
        which, err, tau0 = C.RAISED[(name, state, dtype, s)]
        assert which == "ftanh_bf"
        assert f[s].bound == C.MARGIN * f[s].restate and 0.8 * err <= f[s].restate <= 1.05 * err, (f[s].restate, err)
        assert abs(plain[s].bound - tau0) <= 0.25 * tau0, (plain[s].bound, tau0)      # (the record; float32 BLAS-dependent)
        assert f[s].restate <= 0.34 * 2.0 ** -18          # x^3 / 3 at 2^-6: what the kernel's comment claims


# ------------------------------------------------------------------ 3. the gap and the teeth
@pytest.mark.parametrize("mutant,name,dtype", MUTANT_CASES, ids=[f"{m}-{n}-{d}" for m, n, d in MUTANT_CASES])
def test_mutant_passes_today_and_fails_the_stage_criterion(mutant, name, dtype):
    build, stages, sizes, _ = MUTANTS[mutant]
    cx = C.case(name, "x30")
    used = None
    for size in sizes:                                   # the largest form today's criterion lets through
        dev, grads = C.simulate(cx, dtype, build(cx, dtype, *size))
        t = today(cx, dtype, grads)
        if max(t.values()) <= C.TODAY_GRAD:
            used = size
            break
        print(f"    {mutant} {name} {dtype}: form {size!r} is caught today ({max(t.values()):.1e} in {max(t, key=t.get)})")
    assert used is not None, "no form of the mutant passes today's criterion"
    dev0, grads0 = C.simulate(cx, dtype)
    assert any(not np.array_equal(dev[k], dev0[k]) for k in dev) or any(not np.array_equal(grads[k], grads0[k]) for k in grads)
    f = {x.stage: x for x in C.judge(c=cx, dtype=dtype, dev=dev, grads=grads)}
    bad = [x.stage for x in C.rejected(list(f.values()))]
    print(f"{mutant} {name} {dtype} form {used!r}: today's norm-wise {max(t.values()):.1e} in {max(t, key=t.get)} (accepted <= "
          f"2e-3; unmutated {max(today(cx, dtype, grads0).values()):.1e}); stage criterion rejects {bad}: "
          + "; ".join(f[s].line() for s in stages))
    assert max(t.values()) <= C.TODAY_GRAD
    assert set(stages) <= set(bad), (bad, [f[s].line() for s in stages])
    # teacher forcing: nothing downstream of the mutated buffer is blamed
    assert set(bad) == set(stages), bad
