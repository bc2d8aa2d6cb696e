"""Host checks (no GPU) of the per-element gradient test of the layer-stack engine
(tests/ae_grad_cases.py, tests/test_gpu_ae_grads.py): that it can fail and that its inputs are fair.

Why the file exists.  tests/test_gpu_ae.py::test_ae_train_step_parity and
tests/test_gpu_vae_stack.py::test_vae_stack_step_parity_host_eps see the gradient only through
theta' after one AdaGrad step from acc = 1e-4 (which moves every element by ~ eta sign(g) whatever
|g|) and through one norm of the accumulator over all parameters.  A latent-layer bias gradient
20 % too large passes all three asserts of the frey_like_cont row
(test_todays_asserts_accept_a_wrong_bz_gradient keeps that on record); the per-block criterion
rejects it, and every other wrong gradient of MUTANTS, at the bound the GPU test uses.

The conditions on the inputs (test_inputs_are_fair): every bound (16 x the float32 restatement's
error) is <= 1e-4, the gradient cap of tests/test_gpu_many_samples.py; the scaled runs are off
theta_0; the relu rows have no float64 pre-activation within 1e-4 of the kink and 20-80 % dead
units.  -s prints the restatement table.
"""
import numpy as np
import pytest

from oracle import ae_oracle as A
from tests import ae_grad_cases as G
from tests import vae_stack_oracle as V
from tests.test_gpu_ae import CASES as AE_CASES
from tests.test_gpu_ae import check_theta, data_for

CASE_PARAMS = pytest.mark.parametrize("name,latent,scaled", G.CASES, ids=G.CASE_IDS)


# ------------------------------------------------------------------ 1. recovery and the table
@CASE_PARAMS
def test_restatement_recovers_the_float64_gradient(name, latent, scaled):
    """The float32 oracle step, recovered through sign(theta' - theta) sqrt(acc'), is the float64
    gradient within bound / 16 (by construction: this pins the recovery and prints the table), and
    the float32 value sits inside VALUE_RTOL."""
    st = G.case(name, latent, scaled)
    X = st.Xtr[st.idx]
    _, th, ac = G.restated_step(st.cfg, latent, st.params, X, st.eps)
    err = st.device_errors(th, ac)
    hi, lo = max(err, key=err.get), min(err, key=err.get)
    print(f"{name}-{latent}-{'x30' if scaled else 'theta0'} (seed {st.seed}): restatement error, largest "
          f"{hi} {err[hi]:.1e}, smallest {lo} {err[lo]:.1e}; value {st.restate_value:.1e}")
    assert set(err) == {n for n, _ in st.shapes}
    for n in err:
        assert err[n] == st.restate[n] and err[n] <= st.bound[n] / G.MARGIN * (1 + 1e-12), n
        assert err[n] > 0, n            # a zero restatement error would ask the device for bit equality
    assert st.restate_value <= G.VALUE_RTOL / G.MARGIN


def test_recover_is_exact_on_a_float32_adagrad_step():
    """recover() of a float32 AdaGrad step from zero: |g| to the rounding of g*g and its root, the
    sign wherever the step does not round away."""
    rng = np.random.default_rng(0)
    g = (rng.standard_normal(4096) * 10.0 ** rng.uniform(-7, 2, 4096)).astype(np.float32)
    th = rng.standard_normal(4096).astype(np.float32)
    (th1,), (ac1,) = A.adagrad([th], [np.zeros_like(th)], [g], np.float32(0.01))
    r = G.recover(th, th1, ac1)
    assert np.abs(r - g).max() <= 2.0 ** -23 * np.abs(g).max()
    assert np.all(np.abs(r - g) <= 2.0 ** -22 * np.abs(g))


# ------------------------------------------------------------------ 2. the inputs are fair
@CASE_PARAMS
def test_inputs_are_fair(name, latent, scaled):
    st = G.case(name, latent, scaled)
    cfg, out = st.cfg, st.out64
    assert max(st.bound.values()) <= G.GRAD_CAP, st.bound
    assert not np.array_equal(st.idx, np.sort(st.idx)) or len(st.idx) == 1
    assert st.Xtr.shape[0] > len(st.idx) == G.SHAPE[name].B
    h = np.concatenate([a.ravel() for a in G.hidden_acts(out)])
    xpr = out["Xpr"]
    if scaled:
        assert G.off_theta0(cfg, out)
        if cfg.act == "tanh":
            assert (np.abs(h) > 0.9).any()
            assert (np.abs(h) < 0.99).mean() >= 0.9          # mostly unsaturated
        if cfg.act == "sigmoid":
            assert ((h < 0.2) | (h > 0.8)).any()
        assert ((xpr < 0.2) | (xpr > 0.8)).any()
        assert xpr.min() > 1e-3 and xpr.max() < 1 - 1e-3
    else:
        assert np.abs(xpr - 0.5).max() < 0.05                # theta_0: what today's tests cover
    if cfg.act == "relu":
        pre = np.concatenate([a.ravel() for a in G.hidden_preacts(cfg, latent, [p.astype(np.float64) for p in st.params], out)])
        assert np.abs(pre).min() >= G.KINK
        assert 0.2 <= (pre <= 0).mean() <= 0.8
        assert 0.2 <= (h == 0).mean() <= 0.8


def test_case_table_reaches_the_sizes_it_claims():
    """The tile engine's switches, restated: chunk_group(K) is 8 for K > 512, else 4."""
    s = G.SHAPE
    c = s["k512_513"].cfg()
    assert c.Denc[-1] == 513 and c.Ddec[-1] == 512 and c.otype == "cont" and c.Dobs % 4
    assert s["batch_512"].B == 512 and s["batch_513"].B == 513
    assert s["batch_512"].kw == s["batch_513"].kw
    assert s["latent_deep_k"].cfg().Ddec[0] > 512 and s["latent_deep_k"].latents == ("gauss",)
    e = s["edge_cont_sigmoid"].cfg()
    assert e.Dobs % 4 and e.Dz % 4 and e.Dz > 16 and e.Denc[-1] % 16 == 0 and e.Ddec[-1] % 16 == 0
    assert s["edge_relu_b1"].B == 1 and s["edge_bin_tanh"].B == 17
    widths = set(s["edge_bin_tanh"].cfg().Denc) | set(s["edge_bin_tanh"].cfg().Ddec) | {s["edge_bin_tanh"].cfg().Dz}
    assert widths == {1, 15, 17, 31, 33}


# ------------------------------------------------------------------ 3. wrong gradients are rejected
def _layer_grad(kind):
    """oracle.ae_oracle.layer_grad with one tile-engine fault in it."""
    seen = {}

    def step(f, w, inp, d, back=True):
        gw, gb, d_in = A.layer_grad(f, w, inp, d, back)
        if kind == "drop_last_batch_row" and w == "Wdec0":
            gw = inp[:-1].T @ d[:-1]
        if kind == "bias_from_previous_tile_row" and w in ("Wout", "Wmu", "Wlogs2"):
            gb = gw[max(gw.shape[0] - 16, 0)].copy()        # row Kin of [in | 1]^T dout taken 16 rows up
        if kind == "quad_across_k1":      # the quad that straddles K1 = Dobs: its dA2 part read from dA
            seen[w] = d
            if w == "Wlogs2":
                q = (4 - f.cfg.Dobs % 4) % 4
                assert q
                d2 = d.copy()
                d2[:, :q] = seen["Wmu"][:, :q]
                d_in = d2 @ f.p[w].T
        return gw, gb, d_in
    return step


def _gauss_without_kl_term(f, dG):
    return [("Wzmu", dG - f.mu), ("Wzlv", 0.5 * dG * (f.Z - f.mu) + 0.0)]


# kind: the steps of the oracle's sweep it replaces
SUBSTITUTED = {
    "bias_from_previous_tile_row": dict(layer_grad=_layer_grad("bias_from_previous_tile_row")),
    "drop_last_batch_row": dict(layer_grad=_layer_grad("drop_last_batch_row")),
    "quad_across_k1": dict(layer_grad=_layer_grad("quad_across_k1")),
    "no_minus_z": dict(latent_deltas=lambda f, dG: [("Wz", dG)]),
    "dlv_without_kl_term": dict(latent_deltas=_gauss_without_kl_term),
    "dact_at_preact": dict(dact=lambda f, h, a: A.dact(f, a, a)),
}


def mutant_grads(st, kind=None):
    """The float64 gradient of st's step ({block: array}) from the oracle's sweep with one thing
    wrong (kind) -- or nothing (None: the oracle's)."""
    out = A.forward_backward([q.astype(np.float64) for q in st.params], st.Xtr[st.idx].astype(np.float64), st.cfg,
                             latent=st.latent, eps=None if st.eps is None else st.eps.astype(np.float64),
                             steps=SUBSTITUTED.get(kind))
    nm = [n for n, _ in st.shapes]
    g = {n: np.array(q) for n, q in zip(nm, out["data_grads" if kind == "no_prior" else "grads"])}
    wz, bz = ("Wzmu", "bzmu") if st.latent == "gauss" else ("Wz", "bz")
    if kind == "bz_x1.2":
        g[bz] *= 1.2
    if kind == "wz_last_column_x1.1":
        g[wz][:, -1] *= 1.1
    if kind == "wenc0_last_row_zeroed":
        g["Wenc0"][-1, :] = 0.0
    return g


# kind: (latents, applies(cfg, scaled))
MUTANTS = {
    "bz_x1.2": (("point", "gauss"), lambda c, sc: True),
    "wz_last_column_x1.1": (("point", "gauss"), lambda c, sc: True),
    "wenc0_last_row_zeroed": (("point", "gauss"), lambda c, sc: True),
    "bias_from_previous_tile_row": (("point", "gauss"), lambda c, sc: True),
    "no_prior": (("point", "gauss"), lambda c, sc: True),
    "drop_last_batch_row": (("point", "gauss"), lambda c, sc: True),
    "no_minus_z": (("point",), lambda c, sc: True),
    "dlv_without_kl_term": (("gauss",), lambda c, sc: True),
    "quad_across_k1": (("point", "gauss"), lambda c, sc: c.otype == "cont" and c.Dobs % 4 != 0),
    # relu's f' is the same read at a or at h; tanh' at theta_0 is 1 - a^2 against 1 - h^2 with
    # |a| <= 0.15: they differ by 2 a^4 / 3 <= 4e-4 of a factor that is itself ~1, on a few units only --
    # below what float32 resolves after the layer sums.  This one needs the scaled weights.
    "dact_at_preact": (("point", "gauss"), lambda c, sc: c.act == "sigmoid" or (c.act == "tanh" and sc)),
}
MUTANT_CASES = [(k, n, lat, sc) for k, (lats, ok) in MUTANTS.items() for n, lat, sc in G.CASES
                if lat in lats and ok(G.SHAPE[n].cfg(), sc)]


@CASE_PARAMS
def test_mutant_restatement_with_nothing_wrong_is_the_oracle(name, latent, scaled):
    st = G.case(name, latent, scaled)
    g = mutant_grads(st, None)
    for n in st.g64:
        assert np.array_equal(g[n], st.g64[n]), n


@pytest.mark.parametrize("kind,name,latent,scaled", MUTANT_CASES,
                         ids=[f"{k}-{n}-{lat}-{'x30' if sc else 'theta0'}" for k, n, lat, sc in MUTANT_CASES])
def test_wrong_gradient_is_rejected(kind, name, latent, scaled):
    st = G.case(name, latent, scaled)
    err = G.block_errors(mutant_grads(st, kind), st.g64)
    bad = G.rejected(err, st.bound)
    assert bad, (kind, max(err.values()), st.bound)


def test_every_listed_mutant_runs_somewhere():
    ran = {k for k, _, _, _ in MUTANT_CASES}
    assert ran == set(MUTANTS) and len(MUTANTS) == 10


# ------------------------------------------------------------------ 4. the reason for this file
def test_todays_asserts_accept_a_wrong_bz_gradient():
    """frey_like_cont of tests/test_gpu_ae.py with the float64 oracle's bz gradient x 1.2: the
    value, check_theta after AdaGrad from acc = 1e-4 and the accumulator norm all pass; the
    per-block criterion at this input's own bound rejects it, in bz alone."""
    name, kw, B = AE_CASES[1]
    assert name == "frey_like_cont"
    cfg = A.AEConfig(**kw)
    X = data_for(cfg, 4 * B)
    params = A.init_params(cfg)
    idx = np.random.default_rng(2).choice(X.shape[0], size=B, replace=False).astype(np.int32)
    p64 = [q.astype(np.float64) for q in params]
    a64 = [np.full(q.shape, 1e-4) for q in p64]
    ref, ref_p, ref_a, aux = A.train_step(p64, a64, X.astype(np.float64), idx, cfg)
    nm = [n for n, _ in A.param_shapes(cfg)]
    wrong = [g * 1.2 if n == "bz" else g for n, g in zip(nm, aux["grads"])]
    bad_p, bad_a = A.adagrad(p64, a64, wrong, cfg.eta)
    # today's three asserts (tests/test_gpu_ae.py::test_ae_train_step_parity), the value untouched
    check_theta(A.flatten(bad_p), A.flatten(ref_p), cfg.eta)
    na, ra = A.flatten(bad_a).astype(np.float64), A.flatten(ref_a).astype(np.float64)
    assert np.linalg.norm(na - ra) <= 1e-4 * np.linalg.norm(ra)
    # the per-block criterion
    st = G.make_step(cfg, "point", params, X, idx, None)
    assert max(st.bound.values()) <= G.GRAD_CAP
    err = G.block_errors(dict(zip(nm, wrong)), st.g64)
    assert G.rejected(err, st.bound) == ["bz"]
    assert not G.rejected(G.block_errors(st.g64, st.g64), st.bound)


def test_gauss_helper_names_line_up():
    cfg = G.SHAPE["edge_cont_sigmoid"].cfg()
    assert G.names(cfg, "gauss") == V.names(cfg)
    kin = G.layer_inputs(cfg, "gauss")
    assert kin["Wzlv"] == kin["bzlv"] == 32 and kin["Wmu"] == kin["blogs2"] == 16 and kin["benc0"] == 37
    c2 = G.SHAPE["k512_513"].cfg()
    p = G.oracle("point").init_params(c2)
    s = dict(zip(G.names(c2, "point"), G.scale_params(c2, p, "point")))
    u = dict(zip(G.names(c2, "point"), p))
    assert np.allclose(s["Wenc0"], 30 * u["Wenc0"]) and np.allclose(s["Wz"], 30 * np.sqrt(64 / 513) * u["Wz"])
    assert np.allclose(s["bmu"], 30 * np.sqrt(64 / 512) * u["bmu"])
