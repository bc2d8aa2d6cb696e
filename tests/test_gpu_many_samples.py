"""The fp32 step past the kernels' windows, against the float64 oracle on identical theta / acc /
x / eps (host-injected), through the C ABI.

Two windows end above every shape the other parity tests use:
  * kLP = 4 (vaeb_amd/csrc/fused.hpp): the samples whose eps / z a latent kernel prefetches into
    registers or keeps in LDS.  From l = 4 on, every latent kernel re-reads eps_in, eps or z from
    global memory: the training forward reducer (latent.hpp), the folded backward
    (latent_bwd.hpp), the deferred backward reducer (kernels_aux.hpp), the unfolded backward and
    the evaluation forward (fused.hpp).
  * the column-tile windows of the hidden width: H > 512 (more than 32 column tiles: the second
    tile loop of heads_dechid_kernel, GCH = 8 for the decoder output), cdiv(H, 32) > 32 (the
    slab-summing encoder is off: the default step takes the ticket encoder).

Procedure and tolerances are those of tests/test_gpu_step.py::test_single_step_parity (its
header): ELBO 1e-4 relative; h, mu 1e-5 absolute; data gradients 1e-4 norm-wise per tensor;
check_theta; Adagrad state 1e-4.  In addition lv, z, hd are compared elementwise over all L
planes at the same 1e-5 (the project's activation tolerance), and the stored eps -- a copy of the
pushed float32 values -- exactly: a wrong l >= 4 plane shows there first.  The float32 NumPy
restatement of these steps is within 2.9e-6 (gradients), a 2.2e-5 check_theta fraction and
1.6e-3 lr of the float64 one, inside every cap above.

Recorded on the first run on an MI355X, the maximum over the eight cases and every switch
setting (each run prints its figures; -s shows them): ELBO 5.1e-8 relative, h 1.2e-7, mu 1.4e-8,
lv 1.6e-8, z 2.6e-7, hd 1.3e-7, eps equal, gradients 1.0e-6, Adagrad state 2.9e-7.
"""
import functools

import numpy as np
import pytest

from oracle import vaeb_oracle as O
from tests.test_gpu_step import check_theta, data_for, make_ctx, rel

pytestmark = pytest.mark.gpu

CASES = {
    # name: (config, B)
    "L5_LB_atomic": (dict(D=50, H=33, Z=7, L=5), 21),                       # backward fan-in 3 * 5 = 15: counted atomics
    "L6_LA_deferred": (dict(D=200, H=96, Z=28, estimator="LA", L=6), 50),   # NCT = 2, fan-in 36: deferred reducer, zpre
    "L5_gauss": (dict(D=45, H=30, Z=6, continuous=True, L=5), 17),          # odd D, the Gaussian halves
    "L5_wide_latent": (dict(D=64, H=40, Z=40, L=5), 20),                    # Z > 32: the generic phases
    "L9_LA_latent1": (dict(D=30, H=17, Z=1, estimator="LA", L=9), 5),       # two full windows plus one
    "H600": (dict(D=48, H=600, Z=8), 20),                                   # 38 column tiles, 19 encoder slabs
    "H1040": (dict(D=32, H=1040, Z=4), 16),                                 # cdiv(H, 32) = 33: the ticket encoder
    "H1040_gauss_L5": (dict(D=36, H=1040, Z=20, continuous=True, L=5), 19),  # both windows, NCT = 2
}
SWITCHES = ("VAEB_ATOMIC_HO", "VAEB_ENC_RED", "VAEB_FOLD_BWD", "VAEB_BWD_DEFER", "VAEB_DW2_DEFER")
# the settings tests/test_gpu_step.py::test_atomic_and_slab_handoffs_agree enumerates
MODES = {"atomic": ("1", "0", "1", "1", "1"), "slab": ("0", "0", "1", "1", "1"),
         "decred": ("1", "1", "1", "1", "1"), "unfolded": ("1", "0", "0", "1", "1"),
         "ticket": ("0", "0", "1", "0", "1"), "dw2now": ("1", "0", "1", "1", "0")}
SWITCH_CASES = ["L5_LB_atomic", "L6_LA_deferred", "L5_gauss", "L9_LA_latent1"]   # L > 4 and Z <= 32
IDX = 2


def r16(n):
    return (n + 15) // 16 * 16


@functools.lru_cache(maxsize=None)
def case(name):
    """(cfg, B, x, params, acc, eps, the oracle's step) as test_single_step_parity draws them;
    computed once per case and shared by every switch setting."""
    kw, B = CASES[name]
    cfg = O.Config(**kw)
    x = data_for(cfg, 4 * B)
    rng = np.random.default_rng(3)
    # non-zero biases so every bias path is exercised
    params = [p if p.ndim == 2 else (0.01 * rng.standard_normal(p.shape)).astype(np.float32)
              for p in O.init_params(cfg)]
    acc = [np.zeros_like(p) for p in params]
    eps = rng.standard_normal((cfg.L, B, cfg.Z)).astype(np.float32)
    xb = x[IDX * B:(IDX + 1) * B]
    p64 = [p.astype(np.float64) for p in params]
    a64 = [a.astype(np.float64) for a in acc]
    ref = O.step(p64, a64, xb.astype(np.float64), eps.astype(np.float64), cfg)
    for a in [x, eps] + params + acc:
        a.setflags(write=False)
    return cfg, B, x, params, acc, eps, ref


def run_and_check(name, use_graph=True, what=""):
    cfg, B, x, params, acc, eps, (ref_elbo, ref_p, ref_a, aux) = case(name)
    L, H, Z, Bp = cfg.L, cfg.H, cfg.Z, r16(B)
    ctx = make_ctx(cfg, B, use_graph=use_graph)
    try:
        ctx.set_data(x)
        ctx.set_params(O.flatten(params))
        ctx.set_adagrad_state(O.flatten(acc))
        ctx.set_eps_mode(1)
        ctx.push_eps(eps)
        elbo = ctx.update(IDX)
        got = {"h": ctx.activation("h", Bp * H).reshape(Bp, H)[:B],
               "mu": ctx.activation("mu", Bp * Z).reshape(Bp, Z)[:B],
               "lv": ctx.activation("lv", Bp * Z).reshape(Bp, Z)[:B],
               "eps": ctx.activation("eps", L * Bp * Z).reshape(L, Bp, Z)[:, :B],
               "z": ctx.activation("z", L * Bp * Z).reshape(L, Bp, Z)[:, :B],
               "hd": ctx.activation("hd", L * Bp * H).reshape(L, Bp, H)[:, :B]}
        g = ctx.get_grads()
        newp = ctx.get_params()
        newa = ctx.get_adagrad_state()
    finally:
        ctx.close()

    want = {"h": aux["h"], "mu": aux["mu"], "lv": aux["lv"], "eps": eps, "z": aux["z"],
            "hd": aux["hd"].reshape(L, B, H)}
    # per plane, so a wrong l >= kLP plane is named
    err = {k: (np.abs(got[k] - want[k]).reshape(L, -1).max(axis=1) if got[k].ndim == 3
               else np.abs(got[k] - want[k]).max()) for k in got}
    gerr = {n: rel(gg.reshape(s), rr)
            for (n, s), gg, rr in zip(O.param_shapes(cfg), O.unflatten(g, cfg), aux["data_grads"])}
    print(f"{name}{what}: ELBO rel {abs(elbo - ref_elbo) / abs(ref_elbo):.2e}; "
          + "; ".join(f"{k} {np.max(v):.2e}" for k, v in err.items())
          + f"; grads {max(gerr.values()):.2e}; acc {rel(newa, O.flatten(ref_a)):.2e}")

    assert abs(elbo - ref_elbo) <= 1e-4 * abs(ref_elbo), (elbo, ref_elbo)
    assert err["h"] <= 1e-5 and err["mu"] <= 1e-5 and err["lv"] <= 1e-5, err
    assert np.array_equal(got["eps"], eps), ("eps planes", err["eps"])
    assert np.all(err["z"] <= 1e-5), ("z planes", err["z"])
    assert np.all(err["hd"] <= 1e-5), ("hd planes", err["hd"])
    for n, e in gerr.items():
        assert e <= 1e-4, (n, e)
    check_theta(newp, O.flatten(ref_p), cfg.lr)
    assert rel(newa, O.flatten(ref_a)) <= 1e-4


@pytest.mark.parametrize("name", list(CASES))
def test_single_step_parity_past_the_windows(name):
    run_and_check(name)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", SWITCH_CASES)
def test_many_samples_under_every_switch_setting(name, mode, monkeypatch):
    """Each switch setting selects another kernel holding an l >= kLP branch (`unfolded` is the
    only way into fused.hpp's backward, `ticket` into the dhd launch's reducer at these shapes);
    a setting whose kernels a shape cannot use falls back to the default form.  The same oracle
    step and assertions as above; L6_LA_deferred also on a context without graphs."""
    for var, v in zip(SWITCHES, MODES[mode]):
        monkeypatch.setenv(var, v)
    run_and_check(name, what=f" [{mode}]")
    if name == "L6_LA_deferred":
        run_and_check(name, use_graph=False, what=f" [{mode}, no graph]")
