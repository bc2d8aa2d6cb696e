"""16-bit engine steps along the start-up trajectory of a training run -- TEST HELPER ONLY: the
case table, the input setup and the oracle runs shared by tests/test_h16_traj_host.py (no GPU)
and tests/test_gpu_h16_traj.py.

The state.  Every other oracle comparison of the 16-bit engine (bf16 / fp16 operands) is one step
from theta_0 with Adagrad accumulators preset to 1e-3.  A run of the benchmark or the CLI starts
from theta_0 with ZERO accumulators: the first Adagrad step then moves every parameter by
+-lr = +-0.01, coherently, and with H = 2048 hidden units the log-variance head reaches
|lv| ~ 19 by the third step (step index 2).  The float64 oracle stays finite there and recovers;
its [dMu | dLv] and dA3 reach ~1e8 and ~1e6, which bf16 (fp32's exponent range) stores and fp16
(largest finite value 65504) does not.  The fp16 engine must report that step
(VAEB_ERR_NUMERIC), not hand back a non-finite theta silently.

Trajectory cases (Bernoulli decoder, LB, L = 1; x ~ Bernoulli(0.5), 4 batches: binary with
D % 32 == 0, so the decoder takes its bit-tile path as in the benchmark; theta_0 = init_params,
accumulators zero; device Philox noise; batch order ORDER, 5 steps from step counter STEP0; the
noise of step t is oracle.philox.train_eps(seed, STEP0 + t, ORDER[t], B, B, 0, 1, Z)):

    wide_thin    1024-2048-128, B = 64   heads / dz on the thin launches (Z % 128 == 0)
    wide_split   2048-2048-32,  B = 64   split-K heads and dz plus the latent kernels
    narrow_thin  512-1024-128,  B = 64   inside fp16's range at every step

Gaussian cases (128-64-8, B = 72, synthetic_frey; ONE step from init_params with every b6 set to
the given value and accumulators 1e-3): the decoder's 1 / sigma^2 = e^-a6 scales dA2 and dA6.

    gauss_lowvar_out  b6 = -14   max(|dA2|, |dA6|) > 65504, the float64 ELBO finite
    gauss_lowvar_in   b6 = -12   both below 32768

The seed of a case is (k << 32) | SEED_LO with k the first of k0, k0 + 1, ... at which the
conditions of tests/test_h16_traj_host.py hold (a property of the inputs, found on the host
oracle alone; every case met them at its k0).

Per-step bounds.  The GPU test compares each step with the rounded oracle started from the
DEVICE's own state before that step (teacher forcing: free-running bf16 and float64 runs differ by
27 % in ELBO at the spike step and decorrelate afterwards) at the single-step tolerances of
tests/test_gpu_bf16.py / test_gpu_fp16.py (TOL).  A (case, dtype, step, quantity) may need more;
its bound is then raised in RAISED to at most 4 x the difference between the rounded oracle in
float32 and in float64 arithmetic from that same kind of state (fp32 accumulation is the only
thing the engine does that the float64 oracle does not), measured on the host and recorded
beside the entry.  No bound comes from the device.
"""
import collections

import numpy as np

from oracle import philox as P
from oracle import vaeb_oracle as O

SEED_LO = 0x7F4A7C15
STEP0 = (1 << 33) + 5            # a step counter above 2^32, as tests/test_philox_oracle.py
ORDER = (1, 3, 0, 2, 1)
NB = 4                           # batches of x
F16_MAX = 65504.0
STORES = ("z", "dA2", "dA6", "dA1", "dMu", "dLv", "dA3")   # the backward's and z's 16-bit stores

# the single-step tolerances of the 16-bit modules
TOL = {"elbo": 1e-4, "grad": 2e-3, "acc": 4e-3}

TrajCase = collections.namedtuple("TrajCase", "name kw B k")
GaussCase = collections.namedtuple("GaussCase", "name kw B k b6 idx")

TRAJ_CASES = [
    TrajCase("wide_thin", dict(D=1024, H=2048, Z=128), 64, 31),
    TrajCase("wide_split", dict(D=2048, H=2048, Z=32), 64, 32),
    TrajCase("narrow_thin", dict(D=512, H=1024, Z=128), 64, 33),
]
GAUSS_CASES = [
    GaussCase("gauss_lowvar_out", dict(D=128, H=64, Z=8, continuous=True), 72, 34, -14.0, 1),
    GaussCase("gauss_lowvar_in", dict(D=128, H=64, Z=8, continuous=True), 72, 35, -12.0, 1),
]
BY_NAME = {c.name: c for c in TRAJ_CASES + GAUSS_CASES}

# (case, dtype, step, quantity) -> (bound, the float32-vs-float64 rounded-oracle difference it
# rests on).  quantity: "elbo", "acc" or a parameter name (its data gradient).
RAISED = {}


def bound(case, dtype, step, quantity):
    kind = quantity if quantity in ("elbo", "acc") else "grad"
    return RAISED.get((case, dtype, step, quantity), (TOL[kind], None))[0]


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def seed_of(c):
    return (c.k << 32) | SEED_LO


def cfg_of(c):
    return O.Config(**c.kw)


def data_of(c):
    """The case's dataset, float32 [NB * B (trajectory) or 2 B (Gaussian), D]."""
    from vaeb_amd.synthetic import synth_like
    if isinstance(c, GaussCase):
        return O.synthetic_frey(n=2 * c.B, D=c.kw["D"])
    return synth_like(NB * c.B, D=c.kw["D"])


def eps_of(c, step, idx):
    """The oracle's [1, B, Z] draw of the device's Philox noise of one training step."""
    return P.train_eps(seed_of(c), step, idx, c.B, c.B, 0, 1, c.kw["Z"])


def theta0(c, dtype=np.float64):
    p = [a.astype(dtype) for a in O.init_params(cfg_of(c))]
    if isinstance(c, GaussCase):
        p[cfg_of(c).names.index("b6")][:] = c.b6
    return p


def acc0(c, dtype=np.float64):
    v = 1e-3 if isinstance(c, GaussCase) else 0.0
    return [np.full(a.shape, v, dtype) for a in O.init_params(cfg_of(c))]


def store_max(aux):
    """max |v| over each 16-bit storage point of one oracle step (values BEFORE rounding)."""
    with np.errstate(all="ignore"):
        return {k: float(np.max(np.abs(aux[k]))) if np.all(np.isfinite(aux[k])) else float("inf")
                for k in STORES if k in aux}


def in_f16_range(aux):
    return all(v <= F16_MAX for v in store_max(aux).values())


def oracle_step(c, params, acc, x, idx, step, q, dtype=np.float64):
    """One oracle step of case c on batch idx from (params, acc) with the Philox noise of `step`,
    in `dtype` arithmetic.  Returns O.step's (elbo, theta', acc', aux)."""
    cfg = cfg_of(c)
    xb = x[idx * c.B:(idx + 1) * c.B].astype(dtype)
    with np.errstate(all="ignore"):
        return O.step([p.astype(dtype) for p in params], [a.astype(dtype) for a in acc], xb,
                      eps_of(c, step, idx).astype(dtype), cfg, q=q)


Step = collections.namedtuple("Step", "elbo finite in_range store_max lv_max")


def free_run(c, q, dtype=np.float64):
    """The free-running oracle trajectory of a trajectory case: one Step per entry of ORDER."""
    x = data_of(c)
    p, a = theta0(c, dtype), acc0(c, dtype)
    out = []
    for t, idx in enumerate(ORDER):
        e, p, a, aux = oracle_step(c, p, a, x, idx, STEP0 + t, q, dtype)
        with np.errstate(all="ignore"):
            lv = float(np.max(np.abs(aux["lv"])))
        out.append(Step(float(e), all(np.isfinite(v).all() for v in p), in_f16_range(aux), store_max(aux), lv))
    return out
