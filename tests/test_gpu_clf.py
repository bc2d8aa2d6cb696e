"""The softmax MLP classifier on the device (vaeb_clf_*, vaeb_amd/csrc/engine_clf.inc, clf_softmax.hpp,
ae_mlp.hpp PAeWgradT<RULE, MASK>) against the float64 oracle of tests/clf_oracle.py.

Bounds: a gradient block is inside MARGIN (16) x the float32 restatement's error of the same block, a
value within VALUE_RTOL, P within 16 x the restatement's max |P32 - P64| (all from
tests/ae_grad_cases.py through tests/clf_oracle.py; tests/test_clf_host.py holds the conditions the
cases meet).  No bound comes from the device.  The gradient is read out of state slot 0 under
GradientAscent(eta, momentum 0), as on vaeb_ae.
"""
import ctypes

import numpy as np
import pytest

from tests import ae_optim_cases as AO
from tests import clf_oracle as C
from tests import optim_oracle as OO
from tests.test_gpu_ae import check_theta

pytestmark = pytest.mark.gpu

ACC_RTOL = 1e-4   # tests/test_gpu_ae.py: the accumulator after a step


def make_ctx(cfg, max_batch, **kw):
    from vaeb_amd import _lib
    return _lib.CLFContext(cfg.Din, cfg.Dh, cfg.Dout, act=cfg.act, loss=cfg.loss, prior=cfg.prior, s2=cfg.s2,
                           eta=cfg.eta, max_batch=max_batch, **kw)


def loaded(step, max_batch=None, **kw):
    ctx = make_ctx(step.cfg, max_batch or len(step.idx), **kw)
    ctx.set_data(step.Xtr, step.Ytr)
    ctx.set_params(step.theta())
    return ctx


def assert_gradient(step, ctx, label):
    """One SGA(momentum 0) step on step.idx: the value and slot 0 against the oracle."""
    ctx.set_optimizer("sga", step.cfg.eta)
    v = ctx.train(step.idx)
    err, bad_zero = C.device_errors(step, ctx.get_opt_state(0))
    for n in err:
        print(f"{label} {n}: device {err[n]:.2e} restatement {step.restate[n]:.2e} bound {step.bound[n]:.2e}")
    print(f"{label} value: device {abs(v - step.value64) / abs(step.value64):.2e} restatement {step.restate_value:.2e}")
    assert np.isfinite(v) and abs(v - step.value64) <= C.VALUE_RTOL * abs(step.value64), (v, step.value64)
    assert not bad_zero, bad_zero
    bad = {n: (err[n], step.bound[n]) for n in err if not err[n] <= step.bound[n]}
    assert not bad, bad


# ------------------------------------------------------------------ 1. gradient read-out
@pytest.mark.parametrize("name,scaled,loss", C.CASES, ids=C.CASE_IDS)
def test_gradient_value_and_prediction(name, scaled, loss):
    step = C.case(name, scaled, loss)
    ctx = loaded(step)
    try:
        P = ctx.predict(step.Xtr[step.idx])
        dP = float(np.abs(P - step.out64["P"]).max())
        print(f"P: device {dP:.2e} restatement {step.restate_P:.2e}")
        assert dP <= C.MARGIN * step.restate_P
        assert ctx.get_step() == 0
        assert_gradient(step, ctx, C.CASE_IDS[C.CASES.index((name, scaled, loss))])
        assert ctx.get_step() == 1 and ctx.get_opt_step() == 1   # the Philox step advances on a MAP context too
    finally:
        ctx.close()


# ------------------------------------------------------------------ 2. the update rules
@pytest.mark.parametrize("loss", C.LOSSES)
def test_adagrad_step_and_epoch_track_the_oracle(loss):
    """One AdaGrad step from a small accumulator, then a 4-step train_many whose last batch is partial."""
    cfg = C.cfg_of("edge", loss, prior=True, s2=2.0)
    Xtr, Ytr = C.data_for(cfg, 57, 5)
    params = C.scale_params(cfg, C.init_params(cfg, 3))
    acc = [np.full(p.shape, 1e-4, np.float32) for p in params]
    rng = np.random.default_rng(2)
    first = rng.choice(57, size=17, replace=False).astype(np.int32)
    epoch = rng.permutation(57).astype(np.int32)
    batches = [first] + [epoch[lb:lb + 17] for lb in range(0, 57, 17)]
    assert [len(b) for b in batches] == [17, 17, 17, 17, 6]
    h = OO.adagrad_hyper(cfg.eta)
    none = [None] * len(params)
    ctx = make_ctx(cfg, 17)
    try:
        ctx.set_data(Xtr, Ytr)
        ctx.set_params(C.flatten(params))
        ctx.set_opt_state(0, C.flatten(acc))
        v0 = ctx.train(first)
        r0, p1, a1, _ = C.trajectory(cfg, params, acc, none, Xtr, Ytr, batches[:1], h, 0, np.float64)
        assert abs(v0 - r0[0]) <= C.VALUE_RTOL * abs(r0[0]), (v0, r0)
        check_theta(ctx.get_params(), C.flatten(p1), cfg.eta)
        na, ra = ctx.get_opt_state(0), C.flatten(a1)
        assert np.linalg.norm(na - ra) <= ACC_RTOL * np.linalg.norm(ra)
        got = ctx.train_many(epoch, 17)
        ref, p5, a5, _ = C.trajectory(cfg, p1, a1, none, Xtr, Ytr, batches[1:], h, 1, np.float64)
        assert len(got) == 4 and ctx.get_opt_step() == 5 and ctx.get_step() == 5
        for g, r in zip(got, ref):
            assert abs(g - r) <= 1e-4 * abs(r), (g, r)
        d = np.abs(ctx.get_params() - C.flatten(p5))
        assert float((d > 1e-2 * cfg.eta).mean()) <= 1e-3
        na, ra = ctx.get_opt_state(0), C.flatten(a5)
        assert np.linalg.norm(na - ra) <= 10 * ACC_RTOL * np.linalg.norm(ra)
    finally:
        ctx.close()


@pytest.mark.parametrize("key", AO.STEP_RULES)
def test_one_conditioned_step_of_the_other_rules(key):
    """tests/ae_optim_cases.py's criterion on `edge`: dtheta and the state slots of one step at t = T0 + 1
    from conditioned state inside MARGIN x the float32 restatement of the same step."""
    step = C.case("edge", True, "bernoulli")
    h = AO.HYPERS[key]
    names = C.names(step.cfg)
    g64 = [step.g64[n] for n in names]
    S0, S1 = AO.conditioned(h.rule, g64)
    X, Y = step.Xtr[step.idx], step.Ytr[step.idx]
    runs = {}
    for dt in (np.float64, np.float32):
        p = OO.as_dtype(step.params, dt)
        out = C.forward_backward(p, X, Y, step.cfg)
        runs[dt] = AO.step_arrays(step.params, *OO.apply(p, OO.as_dtype(S0, dt), OO.as_dtype(S1, dt), out["grads"], h, AO.T0 + 1))
    restate = AO.errors(runs[np.float32], runs[np.float64], names)
    bound = {k: {n: C.MARGIN * e for n, e in restate[k].items()} for k in restate}
    ctx = loaded(step)
    try:
        ctx.set_optimizer(*h.abi())
        ctx.set_opt_state(0, C.flatten(S0))
        if OO.SLOTS[h.rule] == 2:
            ctx.set_opt_state(1, C.flatten(S1))
        ctx.set_opt_step(AO.T0)
        ctx.train(step.idx)
        assert ctx.get_opt_step() == AO.T0 + 1
        new_p = C.unflatten(ctx.get_params(), step.cfg)
        new_s0 = C.unflatten(ctx.get_opt_state(0), step.cfg)
        new_s1 = C.unflatten(ctx.get_opt_state(1), step.cfg) if OO.SLOTS[h.rule] == 2 else [None] * len(new_p)
        err = AO.errors(AO.step_arrays(step.params, new_p, new_s0, new_s1), runs[np.float64], names)
        print({k: max(err[k].values()) for k in err}, {k: max(restate[k].values()) for k in restate})
        assert not AO.over(err, bound), AO.over(err, bound)
    finally:
        ctx.close()


# ------------------------------------------------------------------ 3. saturation
@pytest.mark.parametrize("loss", C.LOSSES)
def test_saturated_logits(loss):
    """Logits of order 60.  Both losses: everything finite, rows of P sum to 1 and P is the oracle's
    within 1e-6.  The value and the gradients are held to the oracle for the CATEGORICAL form only: the
    Bernoulli form is ill-conditioned here by construction (1 - P + 1e-7 cancels where P is 1 up to
    rounding; its float32 restatement is itself ~1e-5 off in value and ~1e-3 in gradient), so for it
    only finiteness and P are asserted."""
    step = C.saturated(loss)
    ctx = loaded(step)
    try:
        P = ctx.predict(step.Xtr)
        assert np.isfinite(P).all()
        print("P", float(np.abs(P - step.out64["P"]).max()), float(np.abs(P.sum(axis=1, dtype=np.float64) - 1).max()))
        assert np.abs(P.sum(axis=1, dtype=np.float64) - 1).max() <= C.SAT_P_ATOL
        assert np.abs(P - step.out64["P"]).max() <= C.SAT_P_ATOL
        if loss == "categorical":
            assert_gradient(step, ctx, "saturated")
        else:
            ctx.set_optimizer("sga", step.cfg.eta)
            v = ctx.train(step.idx)
            assert np.isfinite(v) and np.isfinite(ctx.get_opt_state(0)).all() and np.isfinite(ctx.get_params()).all()
    finally:
        ctx.close()


# ------------------------------------------------------------------ 4. the dropout mask
@pytest.mark.parametrize("keep", [0.5, 0.9])
def test_draw_mask_is_the_host_mask(keep):
    """Arenas of 578 (b1) and 1585 (d17) parameters: no multiple of 4 (the last Philox block is partial)
    or of 256."""
    for name in ("b1", "d17"):
        cfg = C.cfg_of(name)
        ctx = make_ctx(cfg, 4, dropout=True, keep=keep)
        try:
            assert ctx.P % 4 != 0 and ctx.P % 256 != 0
            ctx.set_seed(C.MASK_SEED)
            for step, draw in ((0, -1), (7, -1), (0, 0), (0, 3), (7, 3)):
                got = ctx.draw_mask(step, draw)
                assert np.array_equal(got, C.host_mask(C.MASK_SEED, step, draw, ctx.P, keep)), (name, step, draw)
            assert ctx.get_step() == 0
        finally:
            ctx.close()


# ------------------------------------------------------------------ 5. the dropout gradient
@pytest.mark.parametrize("name,scaled,loss", C.CASES, ids=C.CASE_IDS)
def test_dropout_gradient(name, scaled, loss):
    """The gradient under the host mask of (MASK_SEED, MASK_STEP) at keep 0.5.  A block whose float64
    gradient is identically zero (b1: every unit of b0 dropped or dead) must be exactly zero on the
    device; so must every dropped element of the other blocks (no prior)."""
    step = C.case(name, scaled, loss, True)
    ctx = loaded(step, dropout=True, keep=C.KEEP)
    try:
        ctx.set_seed(C.MASK_SEED)
        ctx.set_step(C.MASK_STEP)
        assert_gradient(step, ctx, "dropout")
        g = ctx.get_opt_state(0)
        assert np.all(g[C.flatten(step.masks) == 0] == 0)
        assert ctx.get_step() == C.MASK_STEP + 1
    finally:
        ctx.close()


def test_dropped_elements_read_the_prior_alone():
    step = C.case("edge", True, "bernoulli", True, True)
    ctx = loaded(step, dropout=True, keep=C.KEEP)
    try:
        ctx.set_seed(C.MASK_SEED)
        ctx.set_step(C.MASK_STEP)
        assert_gradient(step, ctx, "dropout+prior")
        g, m, th = ctx.get_opt_state(0), C.flatten(step.masks), step.theta()
        want = -th[m == 0].astype(np.float64) / step.cfg.s2
        assert np.abs(g[m == 0] - want).max() <= 2.0 ** -23 * np.abs(want).max()   # one float32 rounding
    finally:
        ctx.close()


# ------------------------------------------------------------------ 6. keep = 1 is the MAP context
def _five_steps(step, seed, start, **kw):
    ctx = loaded(step, max_batch=4, **kw)
    try:
        ctx.set_optimizer("adam", 1e-3, 0.9, 0.999)
        ctx.set_seed(seed)
        ctx.set_step(start)
        v = ctx.train_many(np.concatenate([step.idx, step.idx[:2]]), 4)
        assert len(v) == 5
        return b"".join(a.tobytes() for a in (v, ctx.get_params(), ctx.get_opt_state(0), ctx.get_opt_state(1)))
    finally:
        ctx.close()


def test_keep_one_is_the_map_context_bitwise_and_seeds_matter():
    step = C.case("edge", True, "bernoulli", False, True)
    assert len(step.idx) == 17
    ref = _five_steps(step, 0, 0)
    assert _five_steps(step, 5, 3, dropout=True, keep=1.0) == ref
    a = _five_steps(step, 5, 3, dropout=True, keep=0.5)
    assert a != ref
    assert _five_steps(step, 5, 3, dropout=True, keep=0.5) == a
    assert _five_steps(step, 6, 3, dropout=True, keep=0.5) != a
    assert _five_steps(step, 5, 4, dropout=True, keep=0.5) != a


# ------------------------------------------------------------------ 7. Monte-Carlo prediction
@pytest.mark.parametrize("L", [1, 5])
def test_mc_prediction(L):
    step = C.case("edge", True, "bernoulli")
    X, Y = step.Xtr, step.Ytr
    n = X.shape[0]
    ctx = loaded(step, max_batch=2 * n // 3, dropout=True, keep=C.KEEP)    # two chunks
    try:
        ctx.set_seed(C.MASK_SEED)
        ctx.set_step(9)
        P64, P32 = np.zeros((n, step.cfg.Dout)), np.zeros((n, step.cfg.Dout), np.float32)
        p64 = [p.astype(np.float64) for p in step.params]
        for l in range(L):
            masks = C.split_mask(C.host_mask(C.MASK_SEED, 9, l, ctx.P, C.KEEP), step.cfg)
            P64 += C.forward_backward(p64, X, Y, step.cfg, masks, need_grad=False)["P"] / L
            P32 += C.forward_backward(step.params, X, Y, step.cfg, masks, need_grad=False)["P"]
        restate = float(np.abs(P32 * np.float32(1.0 / L) - P64).max())
        P = ctx.predict(X, draws=L)
        print(f"L {L}: device {np.abs(P - P64).max():.2e} restatement {restate:.2e}")
        assert np.abs(P - P64).max() <= C.MARGIN * restate
        assert np.abs(P.sum(axis=1, dtype=np.float64) - 1).max() <= 1e-6
        assert ctx.get_step() == 9
        assert np.array_equal(ctx.predict(X, draws=L), P)
        ll = ctx.loglik(X, Y, draw=L - 1)
        masks = C.split_mask(C.host_mask(C.MASK_SEED, 9, L - 1, ctx.P, C.KEEP), step.cfg)
        ref = float(C.forward_backward(p64, X, Y, step.cfg, masks, need_grad=False)["value"])
        assert abs(ll - ref) <= C.VALUE_RTOL * abs(ref)
    finally:
        ctx.close()


def test_draws_on_a_map_context_are_refused():
    from vaeb_amd import _lib
    step = C.case("edge", True, "bernoulli")
    ctx = loaded(step)
    try:
        L, X = ctx.lib, np.ascontiguousarray(step.Xtr[:3])
        out = np.zeros((3, step.cfg.Dout), np.float32)
        n = ctypes.c_int64()
        s = ctypes.c_double()
        assert L.vaeb_clf_predict(ctx.h, _lib.fptr(X), 3, 1, _lib.fptr(out)) == -1
        assert L.vaeb_clf_predict(ctx.h, _lib.fptr(X), 3, -1, _lib.fptr(out)) == -1
        Y = np.ascontiguousarray(step.Ytr[:3])
        assert L.vaeb_clf_accuracy(ctx.h, _lib.fptr(X), _lib.fptr(Y), 3, 2, ctypes.byref(n)) == -1
        assert L.vaeb_clf_loglik(ctx.h, _lib.fptr(X), _lib.fptr(Y), 3, 0, ctypes.byref(s)) == -1
        assert L.vaeb_clf_draw_mask(ctx.h, 0, -1, np.zeros(ctx.P, np.uint8).ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))) == -1
        assert L.vaeb_clf_predict(ctx.h, _lib.fptr(X), 3, 0, _lib.fptr(out)) == 0
    finally:
        ctx.close()


# ------------------------------------------------------------------ 8. accuracy and loglik
@pytest.mark.parametrize("name,loss", [("d17", "bernoulli"), ("d65", "categorical"), ("d257", "bernoulli")])
def test_accuracy_and_loglik_over_chunks(name, loss):
    """n = 2 max_batch + 3 rows.  The count must equal numpy.argmax counting on the downloaded P exactly.
    Columns 2 and Dout - 1 carry equal weights and biases, so they tie in every row; Dout - 1 is lane 16
    (d17: another 16-lane row), lane 0's second column (d65) or its fifth (d257: the looping scan), and
    their bias is lifted (from the float64 logits, on the host) so that the pair is the arg-max in about
    half of the rows: there the lowest index must win.  The other rows keep their own arg-max."""
    step = C.case(name, True, loss)
    cfg = step.cfg
    B = 20
    n = 2 * B + 3
    j1, j2 = 2, cfg.Dout - 1
    X, Y = C.data_for(cfg, n, 11)
    params = [p.copy() for p in step.params]
    params[-2][:, j2] = params[-2][:, j1]
    params[-1][j2] = params[-1][j1]
    A = C.forward_backward([p.astype(np.float64) for p in params], X, Y, cfg, need_grad=False)["A"]
    others = np.delete(A, [j1, j2], axis=1).max(axis=1)
    params[-1][[j1, j2]] += np.float32(np.median(others - A[:, j1]))
    ctx = make_ctx(cfg, B)
    try:
        ctx.set_params(C.flatten(params))
        P = ctx.predict(X)
        am = P.argmax(axis=1)
        tie = (P[:, j1] == P[:, j2]) & (am == j1)
        assert tie.sum() >= 3 and len(set(am[~tie])) >= 2, (int(tie.sum()), sorted(set(am)))   # a condition on the inputs
        assert not (am == j2).any()
        # labels: tie rows alternate between the winning and the losing column; every third other row
        # is labelled with its arg-max, the rest keep their random label
        rows = np.flatnonzero(tie)
        Y[rows] = 0
        Y[rows[::2], j1] = 1
        Y[rows[1::2], j2] = 1
        hit = np.flatnonzero(~tie)[::3]
        Y[hit] = 0
        Y[hit, am[hit]] = 1
        got = ctx.accuracy(X, Y)
        assert got == C.accuracy(Y, P), (got, C.accuracy(Y, P))
        assert len(rows[::2]) + len(hit) <= got <= n - len(rows[1::2]) and 0 < got < n
        out = C.forward_backward([p.astype(np.float64) for p in params], X, Y, cfg, need_grad=False)
        ll = ctx.loglik(X, Y)
        assert abs(ll - float(out["value"])) <= C.VALUE_RTOL * abs(float(out["value"])), (ll, out["value"])
    finally:
        ctx.close()


# ------------------------------------------------------------------ 9. it learns
def _learn(bayesian):
    from vaeb_amd import infalg, mlp
    Xtr, Ytr, Xte, Yte, theta0 = C.learn_setup()
    state = np.random.get_state()
    np.random.seed(C.LEARN_SEED)
    mlp.GenerateGaussians(1000, 1000)
    build = mlp.ConstructBayesianMLPClassifier if bayesian else mlp.ConstructPMLPClassifier
    buildtraining, predict, logjoint, theta = build(2, list(C.LEARN_DH), 2, "tanh", 1.0, infalg.AdaGrad(C.LEARN_ETA))
    np.random.set_state(state)
    assert all(np.array_equal(t.get_value(), t0) for t, t0 in zip(theta, theta0))
    train = buildtraining(Xtr, Ytr)
    rows = np.arange(1000)
    ll0 = None if bayesian else logjoint(Xtr[:100], Ytr[:100])
    vals = [train(0, 100)] + train.many(rows[100:], C.LEARN_BATCH).tolist()   # the first epoch, through both doors
    assert bayesian or abs(vals[0] - ll0) <= 1e-6 * abs(ll0)                  # train(lb, ub) returns the sum it ascends
    for _ in range(C.LEARN_EPOCHS - 1):
        vals.extend(train.many(rows, C.LEARN_BATCH).tolist())
    draws = 20 if bayesian else 0
    acc = train.ctx.accuracy(Xte, Yte, draws) / 1000, train.ctx.accuracy(Xtr, Ytr, draws) / 1000
    train.ctx.close()
    return vals, acc


def test_it_learns():
    """GenerateGaussians(1000, 1000) at seed 15485863, Dh = [32], AdaGrad(0.1), batch 100, 5 epochs.
    MAP: the device's test accuracy is within 0.02 (20 of the 1000 test rows flipping on float32
    trajectories) of the float64 oracle's, which tests/test_clf_host.py holds to >= 0.95.
    Measured: oracle 0.994 test / 0.999 train (CPU, float64); MI355X 0.994 test / 0.999 train (MAP) and
    0.996 test / 0.999 train (dropout).  The figures are printed.
    Dropout (keep 0.5, L = 20): finite values and accuracy >= 0.90; it has no oracle trajectory --
    Philox masks over 50 steps on the host cost too much for a test."""
    te64, tr64, v64 = C.learn_oracle()
    vals, (te, tr) = _learn(False)
    print(f"MAP: device test {te:.3f} train {tr:.3f}; oracle test {te64:.3f} train {tr64:.3f}")
    assert np.isfinite(vals).all() and len(vals) == 50
    assert abs(vals[0] - v64[0]) <= C.VALUE_RTOL * abs(v64[0])
    assert te >= te64 - 0.02
    vals, (te, tr) = _learn(True)
    print(f"dropout: device test {te:.3f} train {tr:.3f}")
    assert np.isfinite(vals).all() and te >= 0.90


# ------------------------------------------------------------------ 10. error codes that need a device
def test_error_codes_on_a_live_context():
    from vaeb_amd import _lib
    step = C.case("edge", False, "bernoulli")
    ctx = loaded(step, max_batch=8)
    try:
        L, h = ctx.lib, ctx.h
        I32 = ctypes.POINTER(ctypes.c_int32)
        idx = np.arange(9, dtype=np.int32)
        out = np.zeros(4, np.float32)
        theta = ctx.get_params()
        assert L.vaeb_clf_train(h, idx.ctypes.data_as(I32), 9, _lib.fptr(out)) == -1           # n > max_batch
        assert L.vaeb_clf_train_many(h, idx.ctypes.data_as(I32), 9, 9, _lib.fptr(out)) == -1   # batch > max_batch
        bad = np.array([0, step.Xtr.shape[0]], np.int32)
        assert L.vaeb_clf_train(h, bad.ctypes.data_as(I32), 2, _lib.fptr(out)) == -1           # an index out of range
        assert L.vaeb_clf_train(h, np.array([-1], np.int32).ctypes.data_as(I32), 1, _lib.fptr(out)) == -1
        p = np.zeros(ctx.P + 1, np.float32)
        assert L.vaeb_clf_set_params(h, _lib.fptr(p), ctx.P + 1) == -1
        assert L.vaeb_clf_get_params(h, _lib.fptr(p), ctx.P - 1) == -1
        assert L.vaeb_clf_set_opt_state(h, 0, _lib.fptr(p), ctx.P + 1) == -1
        assert L.vaeb_clf_get_opt_state(h, 1, _lib.fptr(p), ctx.P) == -1                       # AdaGrad: one slot
        assert L.vaeb_clf_set_opt_step(h, -1) == -1 and L.vaeb_clf_set_step(h, -1) == -1
        o = _lib.AEOptimizerC(0, 0.01, 0.0, 0.0, 1e-3)
        assert L.vaeb_clf_set_optimizer(h, ctypes.byref(o)) == -1                              # AdaGrad's eps is fixed
        assert ctx.get_optimizer()[0] == "adagrad" and ctx.get_step() == 0 and ctx.get_opt_step() == 0
        assert np.array_equal(ctx.get_params(), theta) and not ctx.get_opt_state(0).any()
        assert np.isfinite(ctx.train(idx[:8]))
    finally:
        ctx.close()


# ------------------------------------------------------------------ 11. the Python mirror on a live context
def test_train_object_reads_the_rule_and_the_gradient():
    """mlp.py's train under GradientAscent(momentum 0): optimizer, set_eta and last_gradient() (state
    slot 0, one array per parameter); an Adam construction goes through bind_rule and steps."""
    from vaeb_amd import infalg, mlp
    step = C.case("edge", True, "bernoulli")
    cfg = step.cfg
    state = np.random.get_state()
    try:
        np.random.seed(4)
        build, predict, logjoint, theta = mlp.ConstructPMLPClassifier(cfg.Din, list(cfg.Dh), cfg.Dout, "tanh", 1.0,
                                                                      infalg.GradientAscent(1e-3, momentum=0.0))
        build2, predict2, elbo2, theta2 = mlp.ConstructBayesianMLPClassifier(cfg.Din, list(cfg.Dh), cfg.Dout, "tanh", 1.0,
                                                                             infalg.Adam(1e-3), keep=0.9)
    finally:
        np.random.set_state(state)
    train = build(step.Xtr, step.Ytr)
    try:
        f32 = lambda v: float(np.float32(v))   # noqa: E731
        assert tuple(train.optimizer) == ("sga", f32(1e-3), 0.0, 0.0, 0.0)
        v = train.idx(step.idx)
        g = train.last_gradient()
        assert [a.shape for a in g] == [t.shape for t in theta] == [s for _, s in C.param_shapes(cfg)]
        flat = train.ctx.get_opt_state(0)
        assert np.array_equal(np.concatenate([a.ravel() for a in g]), flat) and np.abs(flat).max() > 0
        assert np.isfinite(v) and predict(step.Xtr[:5]).shape == (5, cfg.Dout)
        train.set_eta(5e-4)
        assert train.optimizer.eta == f32(5e-4) and train.optimizer.rule == "sga" and train.ctx.get_opt_step() == 1
    finally:
        train.ctx.close()
    train2 = build2(step.Xtr, step.Ytr)
    try:
        assert tuple(train2.optimizer) == ("adam", f32(1e-3), f32(0.9), f32(0.999), f32(1e-8))
        vals = train2.many(np.arange(step.Xtr.shape[0]), 17)
        assert np.isfinite(vals).all() and train2.ctx.get_opt_step() == len(vals) == train2.ctx.get_step()
        assert train2.ctx.get_opt_state(1).max() > 0
        assert predict2(step.Xtr[:5], 3).shape == (5, cfg.Dout) and np.isfinite(elbo2(step.Xtr, step.Ytr, 1))
    finally:
        train2.ctx.close()


@pytest.mark.parametrize("bayesian", [0, 1], ids=["map", "bayesian"])
def test_learn_function_runs_and_reports(bayesian, capsys):
    """LearnMLPracticalClassification (mlp.py:332-388) for 2 epochs on 300 rows: the reference's printed
    lines (MAP, verbose) or silence (bayesian, verbose=False, Adam, L = 3), theta in the reference's
    order, and accuracies that are the device's counts."""
    from vaeb_amd import infalg, mlp
    Xtr, Ytr, Xte, Yte, _ = C.learn_setup()
    Xtr, Ytr, Xte, Yte = Xtr[:300], Ytr[:300], Xte[:250], Yte[:250]
    state = np.random.get_state()
    try:
        np.random.seed(5)
        infer = infalg.Adam(1e-2) if bayesian else infalg.AdaGrad(0.1)
        theta = mlp.LearnMLPracticalClassification(Xtr, Ytr, Xte, Yte, bayesian=bayesian, epochs=2, Dh=[16, 8], infer=infer,
                                                   L=3, verbose=not bayesian)
    finally:
        np.random.set_state(state)
    try:
        out = capsys.readouterr().out.splitlines()
        tr, te = theta.accuracy
        if bayesian:
            assert out == []
        else:
            assert out[:3] == ["Building classifier graph.", "Compiling MLP.", "Performing inference."]
            assert [l.split(".")[0] for l in out[3:5]] == ["Epoch 0", "Epoch 1"] and "logjoint = " in out[3]
            assert out[5:] == ["Computing predictions under posterior.", "training accuracy = " + str(tr),
                               "testing accuracy = " + str(te)]
        assert isinstance(theta, list) and [t.shape for t in theta] == [(2, 16), (16, 8), (16,), (8,), (8, 2), (2,)]
        assert len(theta.logp) == 6 and np.isfinite(theta.logp).all()
        ctx = theta.train.ctx
        draws = 3 if bayesian else 0
        assert tr == ctx.accuracy(Xtr, Ytr, draws) / 300 and te == ctx.accuracy(Xte, Yte, draws) / 250
        assert ctx.get_optimizer()[0] == ("adam" if bayesian else "adagrad") and ctx.get_opt_step() == 6
    finally:
        theta.train.ctx.close()


def test_command_line_runs(capsys):
    """python -m vaeb_amd.mlp, in process: the dropout classifier under Adam on the synthetic data."""
    from vaeb_amd import mlp
    state = np.random.get_state()
    try:
        mlp.main(["--synthetic", "--bayesian", "--L", "3", "--keep", "0.9", "--optimizer", "adam", "--eta", "1e-2",
                  "--hidden", "16,8", "--epochs", "2", "--loss", "categorical"])
    finally:
        np.random.set_state(state)
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "Building classifier graph." and out[-2].startswith("training accuracy = ")
    assert 0.0 <= float(out[-1].split("= ")[1]) <= 1.0
