"""Host oracle of the device noise (include/vaeb_hip.h "Noise"): Philox4x32-10
(Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC 2011) and the counter / key
layout every draw site of the library uses, in plain NumPy and float64.

One draw = one 128-bit counter (c0, c1, c2, c3) under the 64-bit key (seed lo, seed hi):

    c0       uint32 of the row (training: batch_index * B_global + row_offset + m; evaluation:
             the row's index in the x passed to the call) or, for the FVS weight noise, of the
             parameter group g = i >> 2
    c1       l * Z + j (latent noise, < 2^30) or 0x40000000 | (g >> 32) (weight noise)
    c2, c3   low / high word of c23 = step ^ (domain & 1) << 63 ^ (domain >> 1) << 40
             (domain 0 training, 1 | stream << 1 evaluation: stream 0 validate, stream s
             the s-th reconstruction / importance sample)

The latent normal is Box-Muller on output words 0 and 1; the weight noise uses all four.
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
_MUL0, _MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_S32, _S8 = np.uint64(32), np.uint64(8)


def _u64(a):
    """Integers (Python ints of any sign below 2^64, or arrays) as uint64, two's complement."""
    if isinstance(a, (int, np.integer)):
        return np.uint64(int(a) & 0xFFFFFFFFFFFFFFFF)
    a = np.asarray(a)
    return a.astype(np.int64).view(np.uint64) if a.dtype.kind == "i" else a.astype(np.uint64)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32 with 10 rounds.  Every argument is masked to 32 bits and broadcast; returns
    the four output words as uint64 arrays (values < 2^32)."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[np.atleast_1d(_u64(a)) & M32 for a in (c0, c1, c2, c3, k0, k1)])
    for _ in range(10):
        p0 = _MUL0 * c0          # 32 x 32 -> 64 bits, no overflow
        p1 = _MUL1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & M32, (p0 >> _S32) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + _W0) & M32
        k1 = (k1 + _W1) & M32
    return c0, c1, c2, c3


def c23(step, domain):
    """Counter words 2-3 as one 64-bit value: the step, the evaluation flag (domain bit 0) in
    bit 63, the sample stream (domain >> 1) from bit 40 up."""
    step, domain = _u64(step), int(domain)
    return step ^ np.uint64((domain & 1) << 63) ^ np.uint64(((domain >> 1) << 40) & 0xFFFFFFFFFFFFFFFF)


def _radius(w):
    return np.sqrt(-2.0 * np.log(((w >> _S8).astype(np.float64) + 1.0) / 16777216.0))    # u in (0, 1]


def _turn(w):
    return 2.0 * np.pi * ((w >> _S8).astype(np.float64) / 16777216.0)                     # u in [0, 1)


def latent_counters(row, c1, step, domain):
    """The four counter words (broadcast uint64 arrays) of latent draws."""
    c = c23(step, domain)
    return np.broadcast_arrays(_u64(row) & M32, _u64(c1) & M32, c & M32, c >> _S32)


def latent_normal(seed, row, c1, step, domain):
    """Standard normals (float64) of the counters (uint32 row, uint32 c1, c23(step, domain))
    under the key (seed lo, seed hi): sqrt(-2 ln u1) cos(2 pi u2)."""
    return _normal(seed, latent_counters(row, c1, step, domain))


def train_counters(step, batch_index, B, B_global, row_offset, L, Z):
    """Counter words, each [L, B, Z], of one training step's draws (domain 0)."""
    row = int(batch_index) * int(B_global) + int(row_offset) + np.arange(B, dtype=np.int64)
    c1 = np.arange(L, dtype=np.int64)[:, None, None] * Z + np.arange(Z, dtype=np.int64)[None, None, :]
    return latent_counters(row[None, :, None], c1, step, 0)


def eval_counters(step, n, Z, stream):
    """Counter words, each [n, Z], of one evaluation stream (domain 1 | stream << 1)."""
    row = np.arange(n, dtype=np.int64)[:, None]
    return latent_counters(row, np.arange(Z, dtype=np.int64)[None, :], step, 1 | (int(stream) << 1))


def _normal(seed, counters):
    seed = _u64(seed)
    w = philox4x32_10(*counters, seed & M32, seed >> _S32)
    return _radius(w[0]) * np.cos(_turn(w[1]))


def train_eps(seed, step, batch_index, B, B_global, row_offset, L, Z):
    """[L, B, Z]: the noise of one training step of a rank holding rows [row_offset, +B) of
    global minibatch batch_index (B_global rows): row = batch_index * B_global + row_offset + m,
    c1 = l * Z + j."""
    return _normal(seed, train_counters(step, batch_index, B, B_global, row_offset, L, Z))


def eval_eps(seed, step, n, Z, stream):
    """[n, Z]: evaluation noise of the n rows of one call, keyed by the row's index in the x
    passed to it.  Stream 0: validate; streams 1..S: sampled reconstruction; stream k + 1:
    importance sample k."""
    return _normal(seed, eval_counters(step, n, Z, stream))


def fvs_counters(step, P):
    g = np.arange((int(P) + 3) // 4, dtype=np.uint64)
    c = c23(step, 0)
    return np.broadcast_arrays(g & M32, np.uint64(0x40000000) | (g >> _S32), c & M32, c >> _S32)


def fvs_zeta(seed, step, P):
    """[P]: the VAEB_EST_FVS weight noise of one step, parameter i from group i >> 2."""
    seed = _u64(seed)
    w = philox4x32_10(*fvs_counters(step, P), seed & M32, seed >> _S32)
    r0, r1, t0, t1 = _radius(w[0]), _radius(w[2]), _turn(w[1]), _turn(w[3])
    return np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)], axis=1).ravel()[:int(P)]
