"""Host checks (no GPU) of the layer-stack engine's training step on the importance-weighted bound
(vaeb_ae_config.iw_samples; tests/vae_stack_iwtrain_oracle.py, tests/test_gpu_vae_stack_iwtrain.py):
the oracle is pinned to float64 torch autograd of L_K, the GPU cases' inputs and bounds are built
and shown to be fair, and eleven kinds of wrong gradient each miss the bounds.

The GPU cases are defined here so both files share them.  Shapes are those of
tests/ae_grad_cases.py; every case runs at theta_0 and at IW-SCALED weights: every layer x
s min(1, sqrt(64 / Kin)), s the first of SCALES for which the float64 weights meet the band

    1.25 <= median over rows of K max_k wn_mk <= 0.8 K

(theta_0 gives 1.00-1.10, uniform weights, where a wrong weight cannot show; the x 30 of
ae_grad_cases gives ~K, one plane taking everything, where the step is a one-sample step).  The seed of
a case is the first for which the relu conditions of ae_grad_cases hold on every plane (no float64
hidden pre-activation within 1e-4 of the kink, 20-80 % dead) and, scaled, some s meets the band.

Bounds are those of ae_grad_cases: per parameter block 16 x the error of the float32 restatement
of the step, recovered from a zero accumulator; every bound <= GRAD_CAP; the restatement's value
within VALUE_RTOL.  No bound comes from the device.  -s prints the tables.
"""
import functools

import numpy as np
import pytest

from oracle import ae_oracle as A
from oracle import philox
from tests import ae_grad_cases as G
from tests import vae_stack_iwtrain_oracle as T
from tests import vae_stack_oracle as V
from tests.test_vae_stack_host import SEED, STEP

SCALES = (6.0, 10.0, 15.0, 20.0)
BAND_LO = 1.25
BAND_HI = 0.8              # x K

# name: (shape of ae_grad_cases, M, K)
IW_CASES = {
    "bin": ("edge_bin_tanh", 17, 3),          # partial last row tile, Dz = 1
    "cont": ("edge_cont_sigmoid", 15, 2),     # scaled [dA | dA2]; Dz = 17 over two column tiles
    "relu": ("edge_relu_b1", 1, 5),           # plane stride 1; encoder wgrad K = 1, decoder K = 5
    "deep": ("batch_512", 3, 171),            # 513 stacked rows: the deep weight-gradient loop
    "full": ("edge_cont_sigmoid", 16, 2),     # stacked rows = max_batch = two full tiles
    "stale11": ("k512_513", 11, 3),           # the stale-rows pair: 33 stacked rows, then stale_small()
}
GPU_CASES = [(n, sc) for n in ("bin", "cont", "relu", "deep", "full") for sc in (False, True)]
GPU_IDS = [f"{n}-{'iwscale' if sc else 'theta0'}" for n, sc in GPU_CASES]
ALL_CASES = [(n, sc) for n in IW_CASES for sc in (False, True)]
ALL_IDS = [f"{n}-{'iwscale' if sc else 'theta0'}" for n, sc in ALL_CASES]


def iw_scale(cfg, params, s):
    kin = G.layer_inputs(cfg, "gauss")
    return [(p * (s * min(1.0, (G.WIDE / kin[n]) ** 0.5))).astype(np.float32) for n, p in zip(V.names(cfg), params)]


def band_figure(out):
    """median over rows of K max_k wn_mk."""
    wn = out["wn"]
    return float(np.median(wn.shape[0] * wn.max(0)))


def in_band(fig, K):
    return BAND_LO <= fig <= BAND_HI * K


def fwd64(cfg, params, X, eps):
    return T.forward_backward([p.astype(np.float64) for p in params], X.astype(np.float64), eps.astype(np.float64),
                              cfg, need_grad=False)


def relu_fair(cfg, params, out):
    if cfg.act != "relu":
        return True
    pre = np.concatenate([a.ravel() for a in G.hidden_preacts(cfg, "gauss", [p.astype(np.float64) for p in params], out)])
    return float(np.abs(pre).min()) >= G.KINK and 0.2 <= float((pre <= 0).mean()) <= 0.8


def restated_step(cfg, params, X, eps):
    """One float32 step of the oracle from a zero accumulator: (value, theta' flat, acc' flat)."""
    assert all(p.dtype == np.float32 for p in params)
    out = T.forward_backward(params, X.astype(np.float32), eps.astype(np.float32), cfg)
    new_p, new_a = A.adagrad(params, [np.zeros_like(p) for p in params], out["grads"], np.float32(cfg.eta))
    assert new_p[0].dtype == np.float32
    return out["iw"] / X.shape[0], A.flatten(new_p), A.flatten(new_a)


def make_iw_step(cfg, params, Xtr, idx, eps, seed=0):
    """ae_grad_cases.Step of one importance-weighted step (eps [K, M, Dz]): the float64 oracle, the
    float32 restatement's per-block error and the bounds."""
    shapes = V.param_shapes(cfg)
    X = Xtr[idx]
    out64 = T.forward_backward([p.astype(np.float64) for p in params], X.astype(np.float64), eps.astype(np.float64), cfg)
    g64 = dict(zip([n for n, _ in shapes], out64["grads"]))
    v32, th32, ac32 = restated_step(cfg, params, X, eps)
    restate = G.block_errors(G.blocks(G.recover(A.flatten(params), th32, ac32), shapes), g64)
    value64 = out64["iw"] / len(idx)
    return G.Step(cfg, "gauss", seed, Xtr, idx, eps, params, shapes, out64, value64, g64, restate,
                  {n: G.MARGIN * e for n, e in restate.items()}, abs(v32 - value64) / abs(value64))


def draw(cfg, M, K, seed):
    params = V.init_params(cfg, seed=15485863 + seed)
    Xtr = G.data_for(cfg, 2 * M + 16, seed)
    rng = np.random.default_rng(100 + seed)
    idx = rng.choice(Xtr.shape[0], size=M, replace=False).astype(np.int32)
    eps = rng.standard_normal((K, M, cfg.Dz)).astype(np.float32)
    return params, Xtr, idx, eps


@functools.lru_cache(maxsize=None)
def case(name, scaled):
    """(Step, s) of one table case; s is None at theta_0."""
    shape, M, K = IW_CASES[name]
    cfg = G.SHAPE[shape].cfg()
    for seed in range(G.MAX_SEEDS):
        params, Xtr, idx, eps = draw(cfg, M, K, seed)
        if not scaled:
            if relu_fair(cfg, params, fwd64(cfg, params, Xtr[idx], eps)):
                return make_iw_step(cfg, params, Xtr, idx, eps, seed), None
            continue
        for s in SCALES:
            ps = iw_scale(cfg, params, s)
            out = fwd64(cfg, ps, Xtr[idx], eps)
            if in_band(band_figure(out), K):
                if relu_fair(cfg, ps, out):
                    return make_iw_step(cfg, ps, Xtr, idx, eps, seed), s
                break
    raise AssertionError(f"{name}: no fair seed below {G.MAX_SEEDS}")


@functools.lru_cache(maxsize=None)
def philox_sibling(name):
    """The scaled case with the device's Philox training noise in the place of its drawn eps."""
    st, _ = case(name, True)
    K = IW_CASES[name][2]
    eps = T.train_eps(SEED, st.idx, st.cfg.Dz, STEP, K).astype(np.float32)
    return make_iw_step(st.cfg, st.params, st.Xtr, st.idx, eps, st.seed)


@functools.lru_cache(maxsize=None)
def stale_small(scaled):
    """The second step of the stale-rows pair: 5 other rows of stale11's Xtr at the same weights
    (the first draw whose bounds, from the float32 restatement, are all <= GRAD_CAP)."""
    big, _ = case("stale11", scaled)
    rest = np.setdiff1d(np.arange(big.Xtr.shape[0]), big.idx)
    for seed in range(7, 7 + G.MAX_SEEDS):
        rng = np.random.default_rng(seed)
        idx5 = rng.choice(rest, size=5, replace=False).astype(np.int32)
        eps5 = rng.standard_normal((3, 5, big.cfg.Dz)).astype(np.float32)
        st = make_iw_step(big.cfg, big.params, big.Xtr, idx5, eps5, seed)
        if max(st.bound.values()) <= G.GRAD_CAP:
            return st
    raise AssertionError("stale_small: no draw inside GRAD_CAP")


# the Philox step and the epoch trajectory of the GPU file
PHILOX_KW = dict(Dobs=37, Denc=(29, 17), Dz=5, Ddec=(13, 21), otype="binary", s2=2.0)
PHILOX_M, PHILOX_K = 9, 3


def philox_setup():
    """cfg, Xtr, params (every layer x 6), acc = 1e-4, idx with one dataset row twice."""
    cfg = A.AEConfig(**PHILOX_KW)
    X = G.data_for(cfg, 4 * PHILOX_M, 5)
    params = [(p * 6).astype(np.float32) for p in V.init_params(cfg, seed=11)]
    acc = [np.full(p.shape, 1e-4, np.float32) for p in params]
    idx = np.random.default_rng(6).choice(X.shape[0], size=PHILOX_M, replace=False).astype(np.int32)
    idx[-1] = idx[2]
    return cfg, X, params, acc, idx


def step64(cfg, X, params, acc, idx, eps):
    return T.train_step([p.astype(np.float64) for p in params], [a.astype(np.float64) for a in acc],
                        X.astype(np.float64), idx, np.asarray(eps, np.float64), cfg)


# ------------------------------------------------------------------ 1. the oracle's gradient
def torch_bound(tp, X, eps, cfg):
    """L_K + the theta prior in float64 torch, eps [K, M, Dz]."""
    import torch
    act = {"tanh": torch.tanh, "sigmoid": torch.sigmoid, "relu": torch.relu}[cfg.act]
    h = X
    for i in range(len(cfg.Denc)):
        h = act(h @ tp[f"Wenc{i}"] + tp[f"benc{i}"])
    mu = h @ tp["Wzmu"] + tp["bzmu"]
    lv = h @ tp["Wzlv"] + tp["bzlv"]
    lws = []
    for e in eps:
        z = mu + torch.exp(lv / 2) * e
        g = z
        for i in range(len(cfg.Ddec)):
            g = act(g @ tp[f"Wdec{i}"] + tp[f"bdec{i}"])
        if cfg.otype == "binary":
            P = torch.sigmoid(g @ tp["Wout"] + tp["bout"])
            ll = (X * torch.log(P + A.EPS_LOG) + (1 - X) * torch.log(1 - P + A.EPS_LOG)).sum(1)
        else:
            xm = torch.sigmoid(g @ tp["Wmu"] + tp["bmu"])
            ls2 = g @ tp["Wlogs2"] + tp["blogs2"]
            ll = (-0.5 * (A.LOG2PI + ls2 + (X - xm) ** 2 / torch.exp(ls2))).sum(1)
        lws.append(ll + 0.5 * (e * e + lv - z * z).sum(1))
    LK = (torch.logsumexp(torch.stack(lws), 0) - np.log(len(eps))).sum()
    prior = sum(-0.5 * (q * q / cfg.s2 + np.log(2 * np.pi * cfg.s2)).sum() for q in tp.values())
    return LK + prior, LK


AUTOGRAD_CASES = [(ot, act, K) for ot in ("binary", "cont") for act in ("tanh", "sigmoid", "relu") for K in (2, 5)]


def autograd_setup(otype, act, K):
    cfg = A.AEConfig(Dobs=23, Denc=(19, 11), Dz=5, Ddec=(13, 17), otype=otype, act=act, s2=2.0)
    M = 7
    X = G.data_for(cfg, M, 3).astype(np.float64)
    p64 = [(p * 10).astype(np.float64) for p in V.init_params(cfg, seed=4)]
    eps = np.random.default_rng(K).standard_normal((K, M, cfg.Dz))
    return cfg, X, p64, eps


@pytest.mark.parametrize("otype,act,K", AUTOGRAD_CASES, ids=[f"{o}-{a}-K{k}" for o, a, k in AUTOGRAD_CASES])
def test_oracle_gradient_matches_autograd(otype, act, K):
    import torch
    cfg, X, p64, eps = autograd_setup(otype, act, K)
    out = T.forward_backward(p64, X, eps, cfg)
    tp = {n: torch.tensor(p, dtype=torch.float64, requires_grad=True) for n, p in zip(V.names(cfg), p64)}
    f, LK = torch_bound(tp, torch.tensor(X), torch.tensor(eps), cfg)
    f.backward()
    assert abs(out["iw"] - LK.item()) <= 1e-9 * abs(LK.item())
    assert abs(out["f"] - f.item()) <= 1e-9 * abs(f.item())
    assert np.abs(out["rows"] - T.marginal_rows(p64, X, eps, cfg)).max() <= 1e-12 * np.abs(out["rows"]).max()
    fig = band_figure(out)
    assert fig > 1.05, fig               # the weights are not uniform: the check sees them
    for n, g in zip(V.names(cfg), out["grads"]):
        ref = tp[n].grad.numpy()
        assert np.abs(g - ref).max() <= 1e-9 * np.abs(ref).max(), n


@pytest.mark.parametrize("otype,act", [("binary", "tanh"), ("cont", "sigmoid"), ("binary", "relu")])
def test_identical_planes_give_the_one_sample_gradient(otype, act):
    """K planes of the same eps: wn = 1 / K and L_K = log w, whose gradient is the K = 1 gradient."""
    cfg, X, p64, eps = autograd_setup(otype, act, 5)
    one = T.forward_backward(p64, X, eps[:1], cfg)
    five = T.forward_backward(p64, X, np.repeat(eps[:1], 5, 0), cfg)
    assert abs(five["iw"] - one["iw"]) <= 1e-12 * abs(one["iw"])
    for n, a, b in zip(V.names(cfg), five["grads"], one["grads"]):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), n


# ------------------------------------------------------------------ 2. inputs and bounds
@pytest.mark.parametrize("name,scaled", ALL_CASES, ids=ALL_IDS)
def test_case_inputs_and_bounds(name, scaled):
    st, s = case(name, scaled)
    shape, M, K = IW_CASES[name]
    fig = band_figure(st.out64)
    hi = max(st.restate, key=st.restate.get)
    print(f"{name}-{'iwscale' if scaled else 'theta0'} (seed {st.seed}, s {s}): K max wn {fig:.2f}; restatement "
          f"error largest {hi} {st.restate[hi]:.1e}; value {st.restate_value:.1e}")
    assert st.eps.shape == (K, M, st.cfg.Dz) and len(st.idx) == M and st.Xtr.shape[0] > M
    if scaled:
        assert s in SCALES and in_band(fig, K), fig
        for s0 in SCALES[:SCALES.index(s)]:      # s is the first that meets the band
            assert not in_band(band_figure(fwd64(st.cfg, iw_scale(st.cfg, draw(st.cfg, M, K, st.seed)[0], s0),
                                                 st.Xtr[st.idx], st.eps)), K)
    else:
        assert 1.0 <= fig <= 1.10, fig       # near-uniform weights (1.10: the largest of 171)
    assert max(st.bound.values()) <= G.GRAD_CAP, st.bound
    assert all(e > 0 for e in st.restate.values())
    assert st.restate_value <= G.VALUE_RTOL
    assert relu_fair(st.cfg, st.params, st.out64)


def test_case_table_reaches_the_sizes_it_claims():
    km = {n: m * k for n, (_, m, k) in IW_CASES.items()}
    assert km == {"bin": 51, "cont": 30, "relu": 5, "deep": 513, "full": 32, "stale11": 33}
    for sc in (False, True):
        small = stale_small(sc)
        assert len(small.idx) == 5 and not set(small.idx.tolist()) & set(case("stale11", sc)[0].idx.tolist())
        assert max(small.bound.values()) <= G.GRAD_CAP and small.restate_value <= G.VALUE_RTOL
    assert G.SHAPE["edge_bin_tanh"].cfg().Dz == 1 and G.SHAPE["edge_cont_sigmoid"].cfg().Dz == 17
    assert km["deep"] > 512 and km["full"] % 16 == 0 and km["bin"] % 16


def test_philox_case_in_float32_sits_inside_the_gpu_caps():
    from tests.test_vae_stack_host import assert_step_close
    cfg, X, params, acc, idx = philox_setup()
    assert len(set(idx.tolist())) == len(idx) - 1
    eps = T.train_eps(SEED, idx, cfg.Dz, STEP, PHILOX_K)
    assert np.array_equal(eps[0], V.train_eps(SEED, idx, cfg.Dz, STEP))        # sample 0: the ELBO draw
    assert np.array_equal(eps[:, -1], eps[:, 2]) and not np.array_equal(eps[0], eps[1])
    rv, rp, ra, aux = step64(cfg, X, params, acc, idx, eps)
    gv, gp, ga, _ = T.train_step(params, acc, X, idx, eps.astype(np.float32), cfg)
    assert_step_close((gv, gp, ga), (rv, rp, ra), cfg.eta)
    assert band_figure(aux) > 1.1


EPOCH_KW = dict(Dobs=96, Denc=(40,), Dz=6, Ddec=(40,), otype="binary")
EPOCH_N, EPOCH_B, EPOCH_K = 70, 20, 3


def epoch_setup():
    """cfg, Xtr, params (every layer x 6), the batches of two epochs (20, 20, 20, 10 each) and the
    host eps of each epoch [K, n, Dz]."""
    cfg = A.AEConfig(**EPOCH_KW)
    X = G.data_for(cfg, EPOCH_N, 9)
    params = [(p * 6).astype(np.float32) for p in V.init_params(cfg)]
    rs = np.random.RandomState(15485863)
    epochs = [A.epoch_batches(EPOCH_N, EPOCH_B, rs), A.epoch_batches(EPOCH_N, EPOCH_B, rs)]
    rng = np.random.default_rng(12)
    eps = [rng.standard_normal((EPOCH_K, EPOCH_N, cfg.Dz)).astype(np.float32) for _ in epochs]
    return cfg, X, params, epochs, eps


def epoch_trajectory(cfg, X, params, epochs, eps, dtype):
    """(values, theta flat) of the oracle over the two epochs from a zero accumulator in dtype."""
    p = [q.astype(dtype) for q in params]
    a = [np.zeros_like(q) for q in p]
    vals = []
    for batches, e in zip(epochs, eps):
        lb = 0
        for b in batches:
            v, p, a, _ = T.train_step(p, a, X.astype(dtype), b, e[:, lb:lb + len(b)].astype(dtype), cfg)
            vals.append(v)
            lb += len(b)
    return vals, V.flatten(p)


def assert_epoch_close(vals, theta, ref_vals, ref_theta, eta):
    """The epoch caps of tests/test_gpu_vae_stack.py."""
    for g, r in zip(vals, ref_vals):
        assert abs(g - r) <= 1e-4 * abs(r), (g, r)
    d = np.abs(np.asarray(theta, np.float64) - np.asarray(ref_theta, np.float64))
    assert float((d > 1e-2 * eta).mean()) <= 1e-3, float((d > 1e-2 * eta).mean())


def test_float32_epoch_trajectory_sits_inside_the_gpu_caps():
    cfg, X, params, epochs, eps = epoch_setup()
    assert [len(b) for b in epochs[0]] == [20, 20, 20, 10]
    rv, rt = epoch_trajectory(cfg, X, params, epochs, eps, np.float64)
    gv, gt = epoch_trajectory(cfg, X, params, epochs, eps, np.float32)
    assert len(rv) == 8
    assert_epoch_close(gv, gt, rv, rt, cfg.eta)


# ------------------------------------------------------------------ 3. wrong gradients are rejected
def _keyed(idx_like, Dz, K, dom):
    j = np.arange(Dz, dtype=np.int64)[None, :]
    return np.stack([philox.latent_normal(SEED, np.asarray(idx_like(k), np.int64)[:, None], j, STEP, dom(k))
                     for k in range(K)]).astype(np.float32)


def wrong_grads(kind, name):
    """(gradient blocks, Step they are judged against) of one wrong step on a scaled case."""
    K = IW_CASES[name][2]
    if kind in T.WRONG or kind in ("stacked_m_major", "y_by_position"):
        st, _ = case(name, True)
    else:
        st = philox_sibling(name)
    cfg, M = st.cfg, len(st.idx)
    X = st.Xtr[st.idx].astype(np.float64)
    eps, Y, wrong = st.eps, None, None
    if kind in T.WRONG:
        wrong = kind
    elif kind == "stacked_m_major":        # the pushed row k M + m read as m K + k
        flat = st.eps.reshape(K * M, cfg.Dz)
        eps = np.stack([flat[np.arange(M) * K + k] for k in range(K)])
    elif kind == "y_by_position":          # Y gathered by m instead of idx[m]
        Y = st.Xtr[:M].astype(np.float64)
    elif kind == "eps_by_stacked_row":
        eps = _keyed(lambda k: k * M + np.arange(M), cfg.Dz, K, lambda k: k << 1)
    elif kind == "eps_by_position":
        eps = _keyed(lambda k: np.arange(M), cfg.Dz, K, lambda k: k << 1)
    elif kind == "eps_stream_k_plus_1":
        eps = _keyed(lambda k: st.idx, cfg.Dz, K, lambda k: (k + 1) << 1)
    elif kind == "eps_eval_domain":
        eps = _keyed(lambda k: st.idx, cfg.Dz, K, lambda k: 1 | (k << 1))
    else:
        raise ValueError(kind)
    out = T.forward_backward([p.astype(np.float64) for p in st.params], X, np.asarray(eps, np.float64), cfg, Y=Y,
                             wrong=wrong)
    return dict(zip([n for n, _ in st.shapes], out["grads"])), st


KINDS = list(T.WRONG) + ["stacked_m_major", "y_by_position", "eps_by_stacked_row", "eps_by_position",
                         "eps_stream_k_plus_1", "eps_eval_domain"]


@pytest.mark.parametrize("kind", KINDS)
def test_wrong_gradient_misses_the_bound_in_a_scaled_case(kind):
    hit = []
    for name in IW_CASES:
        g, st = wrong_grads(kind, name)
        err = G.block_errors(g, st.g64)
        if G.rejected(err, st.bound):
            hit.append(name)
    print(f"{kind}: rejected in {hit}")
    assert hit, kind


def test_nothing_wrong_is_accepted():
    for name in IW_CASES:
        for st in (case(name, True)[0], philox_sibling(name)):
            out = T.forward_backward([p.astype(np.float64) for p in st.params], st.Xtr[st.idx].astype(np.float64),
                                     st.eps.astype(np.float64), st.cfg)
            err = G.block_errors(dict(zip([n for n, _ in st.shapes], out["grads"])), st.g64)
            assert not G.rejected(err, st.bound) and max(st.bound.values()) <= G.GRAD_CAP


def test_there_are_eleven_kinds():
    assert len(KINDS) == len(set(KINDS)) == 11
