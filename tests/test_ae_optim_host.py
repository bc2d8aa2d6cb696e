"""Host side of the layer-stack engine's update rules (no GPU): the oracle rules
(tests/optim_oracle.py) against torch.optim, the conditions the inputs of
tests/test_gpu_ae_optim.py meet, wrong rules landing past the bounds those tests use, the infalg
classes and bind_rule, and the ABI (include/vaeb_hip.h vaeb_ae_optimizer and its six calls).
"""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import ae_grad_cases as G
from tests import ae_optim_cases as C
from tests import optim_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the oracle against torch.optim
def _toy():
    rng = np.random.default_rng(1)
    th = rng.standard_normal((5, 3))
    A_ = rng.standard_normal((3, 3))
    A_ = A_ @ A_.T + np.eye(3)
    b = rng.standard_normal((5, 3))
    return th, (lambda x: -(x @ A_) + b)   # gradient of the concave -1/2 tr(x A x^T) + <b, x>


@pytest.mark.parametrize("key", ["sga0", "sga", "adadelta", "adam"])
def test_oracle_rules_match_torch_optim(key):
    import torch
    h = C.HYPERS[key]
    th0, grad = _toy()
    p = torch.tensor(th0, dtype=torch.float64, requires_grad=True)
    if h.rule == "sga":
        opt = torch.optim.SGD([p], lr=h.eta, momentum=h.beta1, maximize=True)
    elif h.rule == "adadelta":
        opt = torch.optim.Adadelta([p], lr=h.eta, rho=h.beta1, eps=h.eps, maximize=True)
    else:
        opt = torch.optim.Adam([p], lr=h.eta, betas=(h.beta1, h.beta2), eps=h.eps, maximize=True)
    th, s0 = th0.copy(), np.zeros_like(th0)
    s1 = np.zeros_like(th0) if O.SLOTS[h.rule] == 2 else None
    for t in range(1, 6):
        p.grad = torch.tensor(grad(p.detach().numpy()))
        opt.step()
        th, s0, s1 = O.RULE_FN[h.rule](th, s0, s1, grad(th), h, t)
        assert np.abs(th - p.detach().numpy()).max() <= 1e-12, (key, t)


def test_adagrad_rule_is_the_oracles():
    from oracle import ae_oracle as A
    th0, grad = _toy()
    acc = np.abs(th0) + 0.1
    (p,), (a,) = A.adagrad([th0], [acc], [grad(th0)], 0.25)
    q, b, _ = O.adagrad(th0, acc, None, grad(th0), O.adagrad_hyper(0.25), 1)   # a float32 value: Hyper rounds eta once
    assert np.array_equal(p, q) and np.array_equal(a, b)


# ------------------------------------------------------------------ the conditions on the GPU test's inputs
@pytest.mark.parametrize("name,latent,scaled", G.CASES, ids=G.CASE_IDS)
def test_restatement_is_inside_every_cap(name, latent, scaled):
    """Every bound of the read-out and the conditioned steps is <= its cap, none is zero, and the
    restated arrays are float32 throughout."""
    for key, zero in [("sga0", True)] + [(k, False) for k in C.STEP_RULES]:
        rs = C.rule_step(name, latent, scaled, key, zero)
        assert set(rs.bound) == {"dtheta", "s0"} | ({"s1"} if O.SLOTS[rs.h.rule] == 2 else set())
        assert C.caps_hold(rs.bound), (key, {k: max(v.values()) for k, v in rs.bound.items()})
        assert all(b > 0 for v in rs.bound.values() for b in v.values())
        assert all(s.dtype == np.float32 for s in rs.S0)
    assert C.grads32(name, latent, scaled)[0].dtype == np.float32


def test_first_step_cases_cover_every_shape_and_latent():
    cases, ids = C.first_step_cases()
    # all but the Dz = 1 shape (one-element blocks) and the two batch_51x-point-theta0 cases
    assert {(n, lat) for n, lat, _ in cases} == {(n, lat) for n, lat, _ in G.CASES if n != "edge_bin_tanh"}
    assert len(cases) == len(G.CASES) - 6 and len(ids) == len(cases)


@pytest.mark.parametrize("model", [m.name for m in C.MODELS])
@pytest.mark.parametrize("key", C.STEP_RULES)
def test_restated_trajectory_is_inside_every_cap(model, key):
    tr = C.trajectory(model, key)
    assert C.caps_hold(tr.bound), {k: max(v.values()) for k, v in tr.bound.items()}
    assert len(tr.values64) == C.STEPS and len(tr.idx) % tr.model.B != 0
    assert np.isfinite(tr.values64).all()


# ------------------------------------------------------------------ wrong rules land past the bounds
def _adam_no_bias_correction(th, s0, s1, g, h, t):
    dt = th.dtype.type
    m = dt(h.beta1) * s0 + (dt(1) - dt(h.beta1)) * g
    v = dt(h.beta2) * s1 + (dt(1) - dt(h.beta2)) * (g * g)
    return th + dt(h.eta) * m / (np.sqrt(v) + dt(h.eps)), m, v


def _adam_t_one_behind(th, s0, s1, g, h, t):
    return O.adam(th, s0, s1, g, h, t - 1)


def _adadelta_dx_ac_first(th, s0, s1, g, h, t):
    """dx_ac updated before it is read: dx from the new accumulator (solved by one fixed-point pass)."""
    dt = th.dtype.type
    rho, eps = dt(h.beta1), dt(h.eps)
    g_ac = rho * s0 + (dt(1) - rho) * (g * g)
    dx0 = np.sqrt(s1 + eps) * g / np.sqrt(g_ac + eps)
    new1 = rho * s1 + (dt(1) - rho) * (dx0 * dx0)
    dx = np.sqrt(new1 + eps) * g / np.sqrt(g_ac + eps)
    return th + dt(h.eta) * dx, g_ac, new1


def _momentum_on_the_sum(th, s0, s1, g, h, t):
    dt = th.dtype.type
    v = dt(h.beta1) * (s0 + g)
    return th + dt(h.eta) * v, v, s1


def _slots_swapped(th, s0, s1, g, h, t):
    with np.errstate(invalid="ignore"):   # Adam: the square root of a first moment
        a, b, c = O.RULE_FN[h.rule](th, s1, s0, g, h, t)
    return a, c, b


WRONG = [("adam", _adam_no_bias_correction), ("adam", _adam_t_one_behind), ("adadelta", _adadelta_dx_ac_first),
         ("sga", _momentum_on_the_sum), ("adam", _slots_swapped), ("adadelta", _slots_swapped)]


@pytest.mark.parametrize("key,fn", WRONG, ids=[f"{k}-{f.__name__.strip('_')}" for k, f in WRONG])
@pytest.mark.parametrize("name,latent,scaled", G.CASES, ids=G.CASE_IDS)
def test_wrong_rule_misses_the_bounds(name, latent, scaled, key, fn):
    """The wrong rule, run in float32 on the float32 gradient as the device would run it, is past
    the bound of some array in some block, at every case the GPU test uses."""
    rs = C.rule_step(name, latent, scaled, key)
    got = C.step_arrays(rs.st.params, *O.apply(rs.st.params, rs.S0, rs.S1, C.grads32(name, latent, scaled), rs.h,
                                               rs.t0 + 1, fn))
    assert C.over(C.errors(got, rs.ref, rs.names), rs.bound)


# ------------------------------------------------------------------ infalg
class _P:
    def __init__(self, name, shape):
        self.name, self.shape = name, shape


class _Owner:
    def __init__(self, params):
        self.s = {(k, id(p)): np.zeros(p.shape, np.float32) for p in params for k in (0, 1)}

    def _acc_get(self, p):
        return self.s[0, id(p)].copy()

    def _acc_set(self, p, v):
        self.s[0, id(p)][...] = v

    def _state_get(self, slot, p):
        return self.s[slot, id(p)].copy()

    def _state_set(self, slot, p, v):
        self.s[slot, id(p)][...] = v


def _setup():
    theta = [_P("W3", (4, 3)), _P("b3", (3,))]
    return theta, _Owner(theta)


def test_construct_pair_order_and_bind_rule():
    from vaeb_amd import infalg as I
    theta, own = _setup()
    ups = I.GradientAscent(1e-3, 0.9).construct(own, theta)
    assert [type(r) for _, r in ups] == [I.Velocity, I.AscentStep] * 2
    assert ups[1][0] is theta[0] and ups[0][0].slot == 0 and ups[1][1].velocity is ups[0][0]
    assert I.bind_rule(own, theta, ups) == I.BoundRule("sga", 1e-3, 0.9, 0.0, 0.0)
    ups = I.AdaDelta().construct(own, theta)                                   # infalg.py:102-104
    assert [type(r) for _, r in ups] == [I.DecayedSq, I.AdaDeltaStep, I.DecayedSqStep] * 2
    assert (ups[0][0].slot, ups[2][0].slot) == (0, 1) and ups[1][0] is theta[0]
    assert I.bind_rule(own, theta, ups) == I.BoundRule("adadelta", 1.0, 0.95, 0.0, 1e-6)
    ups = I.Adam().construct(own, theta)
    assert [type(r) for _, r in ups] == [I.FirstMoment, I.SecondMoment, I.AdamStep] * 2
    assert I.bind_rule(own, theta, ups) == I.BoundRule("adam", 1e-3, 0.9, 0.999, 1e-8)
    assert I.bind_rule(own, theta, I.AdaGrad(0.05).construct(own, theta)) == I.BoundRule("adagrad", 0.05, 0.0, 0.0,
                                                                                          I.ADAGRAD_EPS)
    for cls in (I.GradientAscent, I.AdaDelta, I.Adam):
        assert issubclass(cls, I.InferenceAlgorithm)
    assert I.GradientAscent(0.1).getinputs() == [0.1] and I.AdaDelta().getinputs() == [] and I.Adam().getinputs() == []
    assert I.AdaDelta().name() == "AdaDelta (Zeiler 2012)" and I.GradientAscent(1).name() == "(Stochastic) Gradient Ascent"
    assert "Adam" in I.Adam().name()


def test_state_views_are_live():
    from vaeb_amd import infalg as I
    theta, own = _setup()
    ups = I.Adam().construct(own, theta)
    m, v = ups[0][0], ups[1][0]
    v.set_value(np.full((4, 3), 2.5))
    assert np.all(own.s[1, id(theta[0])] == 2.5) and np.all(own.s[0, id(theta[0])] == 0)
    assert np.all(v.get_value() == 2.5) and np.all(m.get_value() == 0)


def test_setters():
    from vaeb_amd import infalg as I
    d = I.AdaDelta()
    d.rho = 0.9                                      # the setter the reference's `rho > 0 and rho > 1` meant
    assert (d.rho, d.epsilon, d.eta) == (0.9, 1e-6, 1.0)
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="rho must be greater than zero and less than one"):
            d.rho = bad
    with pytest.raises(ValueError, match="epsilon must be greater than zero"):
        d.epsilon = 0.0
    with pytest.raises(ValueError, match="eta must be greater than zero"):
        I.GradientAscent(0.0)
    with pytest.raises(ValueError, match="momentum"):
        I.GradientAscent(0.1, momentum=1.0)
    assert I.GradientAscent(0.1).momentum == 0.0
    a = I.Adam()
    a.eta, a.beta1 = 3e-4, 0.0
    assert (a.eta, a.beta1, a.beta2, a.epsilon) == (3e-4, 0.0, 0.999, 1e-8)
    for k in ("beta1", "beta2"):
        with pytest.raises(ValueError, match=k):
            setattr(a, k, 1.0)


def test_bind_rule_rejections():
    from vaeb_amd import infalg as I
    theta, own = _setup()
    ups = I.Adam().construct(own, theta)
    with pytest.raises(ValueError, match="cover every parameter"):
        I.bind_rule(own, theta, ups[:3])
    with pytest.raises(ValueError, match="twice"):
        I.bind_rule(own, theta, ups + ups[:1])
    with pytest.raises(ValueError, match="one set of hyper-parameters"):
        I.bind_rule(own, theta, ups[:3] + I.Adam(2e-3).construct(own, theta)[3:])
    with pytest.raises(ValueError, match="does not belong"):
        I.bind_rule(own, theta, I.Adam().construct(_Owner(theta), theta))
    with pytest.raises(ValueError, match="does not own"):
        I.bind_rule(own, theta[:1], ups)
    with pytest.raises(NotImplementedError, match="one rule per model"):
        I.bind_rule(own, theta, ups[:3] + I.AdaDelta().construct(own, theta)[3:])
    with pytest.raises(NotImplementedError):
        I.bind_rule(own, theta, [(theta[0], ("theta + eta * g",))])
    with pytest.raises(ValueError, match="is not slot"):
        I.bind_rule(own, theta, [(ups[1][0], ups[0][1])] + ups[1:])
    # AdaDelta's two accumulators decay with one rho
    dd = I.AdaDelta().construct(own, theta)
    dd[2] = (dd[2][0], I.DecayedSqStep(theta[0], 0.5))
    with pytest.raises(ValueError, match="one set of hyper-parameters"):
        I.bind_rule(own, theta, dd)


def test_bind_updates_still_refuses_other_rules():
    from vaeb_amd import infalg as I
    theta, own = _setup()
    for inf in (I.GradientAscent(1e-3), I.AdaDelta(), I.Adam()):
        with pytest.raises(NotImplementedError, match="AdaGrad rule only"):
            I.bind_updates(own, theta, inf.construct(own, theta))


def test_cli_optimizer_args():
    from vaeb_amd import infalg as I
    from vaeb_amd import vanilla_ae as V
    d = V.optimizer_args(None, None)
    assert isinstance(d, I.AdaGrad) and d.eta == 0.01
    a = V.optimizer_args("adam", None)
    assert isinstance(a, I.Adam) and a.eta == 1e-3
    s = V.optimizer_args("sga", 0.5)
    assert isinstance(s, I.GradientAscent) and (s.eta, s.momentum) == (0.5, 0.9)
    assert isinstance(V.optimizer_args("adadelta", None), I.AdaDelta)
    with pytest.raises(ValueError, match="--optimizer"):
        V.optimizer_args("lbfgs", None)


# ------------------------------------------------------------------ the ABI
def test_optimizer_abi():
    from vaeb_amd import _lib
    assert ctypes.sizeof(_lib.AEOptimizerC) == 20
    assert ctypes.sizeof(_lib.AEConfigC) == 120
    assert [f[0] for f in _lib.AEOptimizerC._fields_] == ["rule", "eta", "beta1", "beta2", "eps"]
    assert _lib.AE_RULE == {"adagrad": 0, "sga": 1, "adadelta": 2, "adam": 3}
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vaeb_hip.h")).read(), flags=re.S)
    src = " ".join(src.split())
    for decl in ["int vaeb_ae_set_optimizer(vaeb_ae* ae, const vaeb_ae_optimizer* opt);",
                 "int vaeb_ae_get_optimizer(vaeb_ae* ae, vaeb_ae_optimizer* out);",
                 "int vaeb_ae_set_opt_state(vaeb_ae* ae, int32_t slot, const float* flat, int64_t n);",
                 "int vaeb_ae_get_opt_state(vaeb_ae* ae, int32_t slot, float* flat, int64_t n);",
                 "int vaeb_ae_set_opt_step(vaeb_ae* ae, int64_t t);",
                 "int vaeb_ae_get_opt_step(vaeb_ae* ae, int64_t* t);",
                 "enum vaeb_ae_rule { VAEB_AE_RULE_ADAGRAD = 0, VAEB_AE_RULE_SGA = 1, VAEB_AE_RULE_ADADELTA = 2, "
                 "VAEB_AE_RULE_ADAM = 3 };",
                 "typedef struct vaeb_ae_optimizer { int32_t rule; float eta, beta1, beta2, eps; } vaeb_ae_optimizer;"]:
        assert decl in src, decl
    L = _lib.load()
    P, F, I64 = ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_int64
    want = {"vaeb_ae_set_optimizer": [P, ctypes.POINTER(_lib.AEOptimizerC)],
            "vaeb_ae_get_optimizer": [P, ctypes.POINTER(_lib.AEOptimizerC)],
            "vaeb_ae_set_opt_state": [P, ctypes.c_int32, F, I64], "vaeb_ae_get_opt_state": [P, ctypes.c_int32, F, I64],
            "vaeb_ae_set_opt_step": [P, I64], "vaeb_ae_get_opt_step": [P, ctypes.POINTER(I64)]}
    for name, args in want.items():
        fn = getattr(L, name)
        assert list(fn.argtypes) == args and fn.restype is ctypes.c_int
    # argument checks come before the device is touched: a null context is VAEB_ERR_ARG
    o = _lib.AEOptimizerC(0, 0.01, 0.0, 0.0, 1e-6)
    assert L.vaeb_ae_set_optimizer(None, ctypes.byref(o)) == -1
    assert L.vaeb_ae_get_opt_step(None, None) == -1
