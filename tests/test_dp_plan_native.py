"""The sharded data-parallel optimizer's index plan as the LIBRARY computes it (VERDICT r4,
"check the C++ plan, not its Python mirror").

`vaeb_dp_plan` (include/vaeb_diag.h) runs the same `dp_bucket_*_runs`, `dp_shard_len`,
`dp_opt_range` and `dp_foreign_range` a rank's step runs (dp_buckets.inc), on a host-only
context: no GPU call, so this is a CPU test of the shipped .so.  The plan splits the
reference's simultaneous Adagrad (VAEB.py:426-444) over ranks; checked here:
* it equals the Python mirror `vaeb_amd.dp.shard_plan` (which the gloo world-2 optimizer test
  uses) for worlds 1-8 on the MNIST, Frey, config-5 and an odd arena;
* over the ranks of a world every arena element is updated by exactly one owner or by every
  rank (the replicated remainders, identical on all ranks), never by two owners, never by none;
* each rank's own + remainders + foreign runs tile every run of the bucket exactly once;
* shards are 64-element aligned inside their run, remainders < 64 * world elements;
* only the bucket holding the last run books the SGVB slot (bucket B and "all");
* the owner of an element is the same whichever bucket form a step takes (A + B == all).
"""
import numpy as np
import pytest

from oracle import vaeb_oracle as O
from vaeb_amd import _lib
from vaeb_amd.dp import arena_runs, shard_plan

ARENAS = [
    ("mnist", 784, 500, 20, False),
    ("frey", 560, 200, 2, True),
    ("config5", 4096, 2048, 128, False),
    ("odd", 37, 19, 3, False),
]


def _offsets(D, H, Z, gauss):
    cfg = O.Config(D=D, H=H, Z=Z, continuous=gauss)
    offs = np.cumsum([0] + [int(np.prod(s)) for _, s in O.param_shapes(cfg)])
    return offs, int(offs[-1])


def _plan(D, H, Z, gauss, world, rank, bucket, sharded=True):
    return _lib.dp_plan(D, H, Z, world, rank, bucket=bucket, sharded=sharded,
                        decoder=_lib.DEC_GAUSSIAN if gauss else _lib.DEC_BERNOULLI)


@pytest.mark.parametrize("name,D,H,Z,gauss", ARENAS)
def test_native_plan_equals_python_mirror(name, D, H, Z, gauss):
    offs, P = _offsets(D, H, Z, gauss)
    runs_all = arena_runs(offs, P, gauss)
    for world in range(1, 9):
        for rank in range(world):
            pl = _plan(D, H, Z, gauss, world, rank, 2)
            assert pl["P"] == P
            assert [(lo, n) for lo, n, _ in pl["runs"]] == runs_all
            own, tails, foreign = shard_plan(runs_all, world, rank)
            # dp_opt_range lists per run: the shard, then the remainder
            want = []
            for lo, n in runs_all:
                want += [r for r in own if lo <= r[0] < lo + n] + [r for r in tails if lo <= r[0] < lo + n]
            assert pl["own"] == want, (name, world, rank)
            assert pl["foreign"] == foreign, (name, world, rank)
            assert pl["book"]
            for (lo, n, S) in pl["runs"]:
                assert S == (n // world) & ~63


@pytest.mark.parametrize("name,D,H,Z,gauss", ARENAS)
def test_native_plan_every_element_owned_once(name, D, H, Z, gauss):
    _, P = _offsets(D, H, Z, gauss)
    for world in range(1, 9):
        for bucket in (0, 1, 2):
            owners = np.zeros(P, np.int32)       # ranks that update the element as its owner
            everyone = None                      # elements every rank updates (remainders)
            covered = np.zeros(P, bool)
            for rank in range(world):
                pl = _plan(D, H, Z, gauss, world, rank, bucket)
                runs = pl["runs"]
                in_bucket = np.zeros(P, bool)
                for lo, n, _ in runs:
                    in_bucket[lo:lo + n] = True
                cover = np.zeros(P, np.int32)
                for lo, n in pl["own"] + pl["foreign"]:
                    cover[lo:lo + n] += 1
                # own + remainders + foreign tile the bucket's runs once, nothing outside them
                assert np.all(cover[in_bucket] == 1) and np.all(cover[~in_bucket] == 0), (name, world, bucket, rank)
                mine = np.zeros(P, bool)
                rem = np.zeros(P, bool)
                for lo, n, S in runs:
                    if S:
                        assert (rank * S) % 64 == 0
                        mine[lo + rank * S:lo + (rank + 1) * S] = True
                    assert n - world * S < 64 * world
                    rem[lo + world * S:lo + n] = True
                upd = np.zeros(P, bool)
                for lo, n in pl["own"]:
                    upd[lo:lo + n] = True
                assert np.array_equal(upd, mine | rem)
                owners += mine
                everyone = rem if everyone is None else (everyone & rem)
                if rank == 0:
                    rem0 = rem
                else:
                    assert np.array_equal(rem, rem0)   # the replicated remainders agree on all ranks
                covered |= upd
                # the SGVB slot rides the run that ends at P: buckets B and "all" only
                assert pl["book"] == (bucket != 0)
            assert np.all(owners[everyone] == 0)
            assert np.all(((owners == 1) | everyone)[covered])   # one owner, or every rank
            assert np.all(owners <= 1)
            assert np.array_equal(covered, in_bucket)            # and nothing in the bucket missed


@pytest.mark.parametrize("name,D,H,Z,gauss", ARENAS)
def test_native_plan_owner_independent_of_bucket_form(name, D, H, Z, gauss):
    _, P = _offsets(D, H, Z, gauss)
    for world in (2, 3, 8):
        for rank in range(world):
            a = _plan(D, H, Z, gauss, world, rank, 0)
            b = _plan(D, H, Z, gauss, world, rank, 1)
            al = _plan(D, H, Z, gauss, world, rank, 2)
            assert sorted(a["own"] + b["own"]) == sorted(al["own"])
            assert sorted(a["foreign"] + b["foreign"]) == sorted(al["foreign"])


def test_native_plan_replicated_form():
    """sharded = 0 (world 1, or VAEB_DP_SHARD=0): every rank updates the whole bucket."""
    _, P = _offsets(784, 500, 20, False)
    for world in (1, 4, 8):
        for rank in range(world):
            pl = _plan(784, 500, 20, False, world, rank, 2, sharded=False)
            assert sum(n for _, n in pl["own"]) == P and pl["foreign"] == []
            assert all(S == 0 for _, _, S in pl["runs"])


def test_native_plan_rejects_bad_arguments():
    with pytest.raises(_lib.VaebError):
        _lib.dp_plan(784, 500, 20, 2, 2)
    with pytest.raises(_lib.VaebError):
        _lib.dp_plan(784, 500, 20, 2, 0, bucket=3)
