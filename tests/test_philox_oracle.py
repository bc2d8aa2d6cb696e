"""The host Philox oracle (oracle/philox.py) on its own: the generator against published
known-answer vectors, the normals' moments, the disjointness of the counter domains, and the
proof that the GPU cases of tests/test_gpu_philox.py (which imports the case tables below) can
tell a mis-keyed draw site from a correct one."""
import collections

import numpy as np
import pytest

from oracle import philox as P
from oracle import vaeb_oracle as O

# ----------------------------------------------------------------- the GPU tests' cases
# Every Philox-mode case runs at batch index 2 with a step counter and a seed above 2^32, so
# a site that drops a high word, or keys by the local row, draws different numbers.
STEP = (1 << 33) + 5
IDX = 2

EpsCase = collections.namedtuple("EpsCase", "name kw B B_global row_offset seed")


def _case(name, kw, B, k, shard=False):
    # The seeds differ per case (high word k).  Two independent normals are within 0.1 of each
    # other with probability 5.6 %, so among the 7 elements of the single-row case one
    # coincidence already breaks the 90 % rule below, and among the 39 of odd_shapes four do:
    # for those cases k is the first of k0, k0 + 20, k0 + 40, ... at which every mis-keyed
    # variant passes (a property of the inputs, found on the host oracle alone).
    seed = (k << 32) | 0x7F4A7C15
    return EpsCase(name + ("_rank1" if shard else ""), kw, B, 2 * B if shard else B, B if shard else 0, seed)


# one case per latent form of the fp32 engine
FORMS = [
    ("fused", dict(D=784, H=500, Z=20), 100),
    ("generic_phases", dict(D=64, H=40, Z=40, L=2), 20),
    ("two_fx_slots", dict(D=784, H=128, Z=24, L=2), 100),
    ("odd_shapes", dict(D=37, H=19, Z=3), 13),
    ("single_row", dict(D=50, H=33, Z=7), 1),
]
SEED_K = {"fused": 1, "generic_phases": 2, "two_fx_slots": 3, "odd_shapes": 24, "single_row": 85,
          "fused_rank1": 6, "generic_phases_rank1": 7, "two_fx_slots_rank1": 8, "odd_shapes_rank1": 69,
          "single_row_rank1": 210, "frey2_gauss": 11, "latent28_LA_L2": 12,
          "bern_LB_tails": 13, "bern_LA_L2": 14, "thin_tails": 15, "trajectory": 16, "fvs_odd": 17}


def _mk(name, kw, B, shard=False):
    return _case(name, kw, B, SEED_K[name + ("_rank1" if shard else "")], shard)


# (a) the draws themselves: every form as a whole minibatch and as rank 1 of 2 (B_global = 2 B,
# row_offset = B: the only kind of case that can catch a dropped row_offset)
EPS_CASES = [_mk(*f) for f in FORMS] + [_mk(*f, shard=True) for f in FORMS]
# (b) the Philox-mode step against the float64 oracle
STEP_CASES = [_mk(*f) for f in FORMS] + [
    _mk("fused", dict(D=784, H=500, Z=20), 100, shard=True),
    _mk("frey2_gauss", dict(D=560, H=200, Z=2, continuous=True), 100),
    _mk("latent28_LA_L2", dict(D=200, H=96, Z=28, estimator="LA", L=2), 50),
]
# (f) the 16-bit engines' three draw sites, batch index 1
H16_IDX = 1
H16_CASES = [
    _mk("bern_LB_tails", dict(D=200, H=136, Z=24), 200),
    _mk("bern_LA_L2", dict(D=128, H=64, Z=16, estimator="LA", L=2), 136),
    _mk("thin_tails", dict(D=264, H=200, Z=128), 200),
]
# (c) several steps, (e) the FVS step
TRAJ_CASE = _mk("trajectory", dict(D=66, H=48, Z=12), 32)
FVS_CASE = _mk("fvs_odd", dict(D=37, H=19, Z=3, estimator="FVS"), 13)


def case_eps(c, step=STEP, idx=IDX):
    """The oracle's [L, B, Z] noise of one training step of case c."""
    return P.train_eps(c.seed, step, idx, c.B, c.B_global, c.row_offset, c.kw.get("L", 1), c.kw["Z"])


ALL_TRAIN = {c.name: (c, IDX) for c in EPS_CASES + STEP_CASES + [TRAJ_CASE, FVS_CASE]}
ALL_TRAIN.update({c.name: (c, H16_IDX) for c in H16_CASES})


# ------------------------------------------------------------------ known-answer vectors
KAT = [   # Random123 kat_vectors, philox4x32 10 rounds: counter, key -> output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox4x32_10_known_answers():
    for ctr, key, want in KAT:
        got = P.philox4x32_10(*ctr, *key)
        assert tuple(int(w[0]) for w in got) == want
    # vectorised: the three vectors in one call
    cols = [np.array(v, np.uint64) for v in zip(*[c + k for c, k, _ in KAT])]
    got = P.philox4x32_10(*cols)
    for i, (_, _, want) in enumerate(KAT):
        assert tuple(int(w[i]) for w in got) == want


def test_c23_mirrors_the_device_layout():
    assert int(P.c23(5, 0)) == 5
    assert int(P.c23(5, 1)) == 5 | (1 << 63)
    assert int(P.c23((1 << 33) + 5, 1 | (3 << 1))) == ((1 << 33) + 5) | (1 << 63) | (3 << 40)
    # a stream and a step >= 2^40 share bits (XOR): the documented limit
    assert int(P.c23(1 << 40, 1 | (1 << 1))) == 1 << 63


# ------------------------------------------------------------------------------- moments
def test_moments_of_2_pow_19_draws():
    """N = 2^19 draws of each kind.  For standard normals the standard errors are
    se(mean) = 1 / sqrt(N) = 1.38e-3, se(variance) = sqrt(2 / N) = 1.95e-3 and
    se(mean of x^4) = sqrt(96 / N) = 1.35e-2; every bound is 5 standard errors (the draws are
    deterministic, so this is a fixed check, not a flaky one).  The u1 in (0, 1] floor bounds
    |x| by sqrt(2 ln 2^24) = 5.77."""
    N = 1 << 19
    se_m, se_v, se_4 = 1 / np.sqrt(N), np.sqrt(2 / N), np.sqrt(96 / N)
    draws = {
        "train": P.train_eps((3 << 32) | 9, STEP, 1, 4096, 4096, 0, 1, 128).ravel(),
        "eval": P.eval_eps((3 << 32) | 9, STEP, 4096, 128, 2).ravel(),
        "fvs": P.fvs_zeta((3 << 32) | 9, STEP, N),
    }
    for what, x in draws.items():
        assert x.size == N and np.all(np.isfinite(x))
        assert abs(x.mean()) <= 5 * se_m, (what, x.mean())
        assert abs(x.var() - 1) <= 5 * se_v, (what, x.var())
        assert abs((x ** 4).mean() - 3) <= 5 * se_4, (what, (x ** 4).mean())
        assert np.abs(x).max() <= np.sqrt(2 * np.log(2.0 ** 24)) + 1e-12
    # the four normals of a weight-noise group are uncorrelated (cos / sin of one angle)
    z = draws["fvs"].reshape(-1, 4)
    for a, b in ((0, 1), (2, 3), (0, 2)):
        r = float((z[:, a] * z[:, b]).mean())
        assert abs(r) <= 5 / np.sqrt(z.shape[0]), (a, b, r)


# --------------------------------------------------------------------------- disjointness
def _as128(words):
    c0, c1, c2, c3 = [w.ravel() for w in words]
    return [int(a) | int(b) << 32 | int(c) << 64 | int(d) << 96 for a, b, c, d in zip(c0, c1, c2, c3)]


def test_counter_domains_are_pairwise_disjoint():
    """Same seed and step: training (L = 2), evaluation streams 0..3 and the weight noise never
    share a 128-bit counter, and no domain repeats one."""
    B, Z, L, n, Pn = 6, 5, 2, 12, 50     # training rows 6..11 (batch index 1) lie inside evaluation rows 0..11
    sets = {"train": _as128(P.train_counters(STEP, 1, B, B, 0, L, Z)),
            "fvs": _as128(P.fvs_counters(STEP, Pn))}
    for s in range(4):
        sets[f"eval{s}"] = _as128(P.eval_counters(STEP, n, Z, s))
    # the row and c1 ranges of the domains overlap, so only c1 bit 30 / the c23 bits separate them
    assert set(range(B, 2 * B)) <= set(range(n))
    for k, v in sets.items():
        assert len(set(v)) == len(v), k
    names = sorted(sets)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert not (set(sets[a]) & set(sets[b])), (a, b)


# ------------------------------------------------------------------------- discrimination
def _wrong_c1(c, idx):
    L, Z = c.kw.get("L", 1), c.kw["Z"]
    row = idx * c.B_global + c.row_offset + np.arange(c.B)
    j = np.broadcast_to(np.arange(Z)[None, None, :], (L, c.B, Z))
    return P.latent_normal(c.seed, row[None, :, None], j, STEP, 0)


MISTAKES = {
    # name: (expressible for this case?, the mis-keyed draw)
    "local_row": (lambda c: True,
                  lambda c, idx: P.train_eps(c.seed, STEP, 0, c.B, c.B_global, 0, c.kw.get("L", 1), c.kw["Z"])),
    "row_offset_dropped": (lambda c: c.row_offset > 0,
                           lambda c, idx: P.train_eps(c.seed, STEP, idx, c.B, c.B_global, 0, c.kw.get("L", 1), c.kw["Z"])),
    "step_low_word_only": (lambda c: True,
                           lambda c, idx: P.train_eps(c.seed, STEP & 0xFFFFFFFF, idx, c.B, c.B_global, c.row_offset,
                                                      c.kw.get("L", 1), c.kw["Z"])),
    "seed_low_word_only": (lambda c: True,
                           lambda c, idx: P.train_eps(c.seed & 0xFFFFFFFF, STEP, idx, c.B, c.B_global, c.row_offset,
                                                      c.kw.get("L", 1), c.kw["Z"])),
    "c1_without_l": (lambda c: c.kw.get("L", 1) > 1, _wrong_c1),
}
PAIRS = [(n, m) for n, (c, _) in ALL_TRAIN.items() for m, (ok, _) in MISTAKES.items() if ok(c)]


def test_every_mistake_is_expressible_in_some_case_of_every_gpu_test():
    assert STEP >> 32 and all(c.seed >> 32 for c, _ in ALL_TRAIN.values())
    assert all(idx > 0 for _, idx in ALL_TRAIN.values())
    for group in (EPS_CASES, STEP_CASES):
        for m, (ok, _) in MISTAKES.items():
            assert any(ok(c) for c in group), m
    # every form of (a) has its rank-1 twin
    assert {c.name for c in EPS_CASES if c.row_offset} == {c.name + "_rank1" for c in EPS_CASES if not c.row_offset}


@pytest.mark.parametrize("name,mistake", PAIRS, ids=[f"{n}-{m}" for n, m in PAIRS])
def test_gpu_cases_tell_a_mis_keyed_site_apart(name, mistake):
    """The mis-keyed draw differs from the oracle by more than 0.1 in >= 90 % of the elements
    (c1 = j is by construction the right key on sample plane l = 0: there the planes l >= 1 are
    the elements, and plane 0 must agree exactly)."""
    c, idx = ALL_TRAIN[name]
    good = case_eps(c, idx=idx)
    bad = MISTAKES[mistake][1](c, idx)
    assert bad.shape == good.shape
    if mistake == "c1_without_l":
        assert np.array_equal(bad[0], good[0])
        good, bad = good[1:], bad[1:]
    frac = float((np.abs(bad - good) > 0.1).mean())
    assert frac >= 0.9, frac


def test_evaluation_streams_differ_from_each_other_and_from_training():
    """A site that ignored the domain (validation drawing the training stream, or every sample
    the same stream) is told apart the same way."""
    seed, n, Z = (21 << 32) | 3, 77, 20
    ev = [P.eval_eps(seed, STEP, n, Z, s) for s in range(4)]
    tr = P.train_eps(seed, STEP, 0, n, n, 0, 1, Z)[0]
    al = ev + [tr]
    for i in range(len(al)):
        for k in range(i + 1, len(al)):
            assert float((np.abs(al[i] - al[k]) > 0.1).mean()) >= 0.9, (i, k)
    # chunk-local rows (a 32-row chunk restarting at row 0) differ from call-global rows
    local = np.concatenate([P.eval_eps(seed, STEP, min(32, n - r0), Z, 0) for r0 in range(0, n, 32)])
    assert float((np.abs(local[32:] - ev[0][32:]) > 0.1).mean()) >= 0.9


def test_fvs_case_tells_a_wrong_weight_noise_apart():
    """The FVS GPU test's three steps (sigma = 1e-3) with zeta drawn at the wrong step: more than
    half of mu' moves by more than 1e-3 lr, where the GPU test allows a 1e-3 fraction."""
    c = FVS_CASE
    cfg = O.Config(**c.kw)
    x = O.synthetic_mnist(n=8 * c.B, D=cfg.D, seed=0).astype(np.float64)
    rng = np.random.default_rng(21)
    theta = [(t + 0.05 * rng.standard_normal(t.shape)).astype(np.float64) for t in O.init_params(cfg)]
    Pn = O.num_params(cfg)
    assert Pn % 4 != 0
    mus = []
    for zstep in (STEP, STEP + 1):
        m, s = [t.copy() for t in theta], [np.full_like(t, 1e-3) for t in theta]
        am, as_ = [np.zeros_like(t) for t in theta], [np.zeros_like(t) for t in theta]
        for t, b in enumerate((IDX, 5, 1)):
            zeta = O.unflatten(P.fvs_zeta(c.seed, zstep + t, Pn), cfg)
            eps = P.train_eps(c.seed, STEP + t, b, c.B, c.B, 0, 1, cfg.Z)
            _, m, s, am, as_, _ = O.fvs_step(m, s, am, as_, x[b * c.B:(b + 1) * c.B], eps, zeta, cfg)
        mus.append(O.flatten(m))
    assert float((np.abs(mus[0] - mus[1]) > 1e-3 * cfg.lr).mean()) > 0.5
