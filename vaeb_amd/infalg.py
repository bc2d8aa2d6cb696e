"""Optimizer plug-in mirror of /root/reference/degenerate-vae/infalg.py.

The reference's contract (infalg.py:9-41): an `InferenceAlgorithm` has `name()`,
`construct(f, theta) -> updates` (a list of (shared, new value) pairs that Theano applies
simultaneously after evaluating f) and `getinputs()` (the extra run-time inputs).
`AdaGrad.construct` (infalg.py:148-164) appends, per parameter, a fresh zero accumulator
g_ac with the pair (g_ac, g_ac + g^2) and the pair (theta, theta + eta*g/(sqrt(g_ac') + 1e-6)).

Here the arithmetic of those pairs runs inside the HIP kernels (fused into the
weight-gradient epilogues of libvaeb_hip.so, over one flat accumulator arena), so
`construct` returns the same list shape with symbolic right-hand sides -- `AccumulateSq`
and `AdaGradStep` records naming the parameter, eta and eps -- and the objective the list
is built for (`f`: a `VAEB` / `VAE` model or the AE engine) BINDS it: it checks that the
pairs cover each of its parameters exactly once with one (eta, eps), that the pairs are the
engine's own accumulators and parameters, and takes eta as its learning rate.  The
accumulator of the pair is a live view of the engine's arena (`get_value` / `set_value`),
the object Theano's `shared(np.zeros(...))` was.  The same rule is VAEB.getUpdates
(VAEB.py:426-444), and it is the only rule of the fp32 and 16-bit `vaeb_update` engines:
`bind_updates` accepts nothing else.

The layer-stack engine (vaeb_amd/ae.py, csrc/ae_mlp.hpp PAeWgradT<RULE>) applies four rules, all
ascending, chosen per context (include/vaeb_hip.h vaeb_ae_set_optimizer): `AdaGrad`, and the
reference's other two optimisers plus the one a VAE trainer is expected to have:
  * `GradientAscent(eta, momentum=0.0)` (infalg.py:44-74, plus momentum): v' = mu v + g,
    theta' = theta + eta v'.  The state slot 0 is v; with momentum 0 it holds the step's gradient.
  * `AdaDelta(rho=0.95, epsilon=1e-6, eta=1.0)` (infalg.py:80-137 with the rho its setter meant:
    Appendix B, the reference's test `rho > 0 and rho > 1` admits no valid rho): slot 0 g_ac, slot 1 dx_ac.
  * `Adam(eta=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8)` with bias correction: slot 0 m, slot 1 v.
Each `construct` returns the reference's pair-list shape with symbolic right-hand sides, the state
objects being `StateView`s of the engine's slot-0 / slot-1 arenas, and `bind_rule` is what the layer
stack does with the list: the checks of `bind_updates` for any of the four rules, returning the rule
and its numbers (`BoundRule`).  The reference's HMC is unfinished and is not provided.
"""
from __future__ import annotations

import abc
from typing import NamedTuple

import numpy as np

ADAGRAD_EPS = 1e-6   # infalg.py:158


class AccumulateSq(NamedTuple):
    """Right-hand side g_ac + T.sqr(T.grad(f, theta)) (infalg.py:157)."""
    param: object


class AdaGradStep(NamedTuple):
    """Right-hand side theta + eta * g / (T.sqrt(g_ac_new) + eps) (infalg.py:158)."""
    param: object
    accumulator: object
    eta: float
    eps: float


class Accumulator:
    """The g_ac shared variable of one parameter (infalg.py:153): a view of the engine's
    Adagrad arena.  `owner` provides `_acc_slice(param) -> (get, set)`."""

    def __init__(self, owner, param):
        self._owner, self.param = owner, param
        self.name = "g_ac_" + str(getattr(param, "name", "theta"))

    def get_value(self, borrow=False):
        return self._owner._acc_get(self.param)

    def set_value(self, value, borrow=False):
        self._owner._acc_set(self.param, np.asarray(value, np.float32))

    def __repr__(self):
        return f"Accumulator({self.name})"


class InferenceAlgorithm(abc.ABC):
    """infalg.py:9-41."""

    @abc.abstractmethod
    def name(self) -> str: ...

    @abc.abstractmethod
    def construct(self, f, theta) -> list: ...

    @abc.abstractmethod
    def getinputs(self) -> list: ...


class AdaGrad(InferenceAlgorithm):
    """infalg.py:141-183."""

    def __init__(self, eta):
        self.eta = eta

    def name(self):
        return "AdaGrad"

    def construct(self, f, theta):
        """infalg.py:148-164: per parameter, (g_ac, g_ac + g^2) then (theta, theta + dx).
        `f` is the objective's owner (it holds the accumulator arena)."""
        updates = []
        for t in theta:
            g_ac = Accumulator(f, t)
            updates.append((g_ac, AccumulateSq(t)))
            updates.append((t, AdaGradStep(t, g_ac, self.eta, ADAGRAD_EPS)))
        return updates

    def getinputs(self):
        return []

    @property
    def eta(self):
        return self._eta

    @eta.setter
    def eta(self, eta):
        if not eta > 0:
            raise ValueError("eta must be greater than zero and less than one.")   # infalg.py:174-176
        self._eta = float(eta)

    def rule(self):
        """The update the kernels apply, as (eta, eps)."""
        return self._eta, ADAGRAD_EPS


def bind_updates(owner, params, updates):
    """What an engine does with `construct`'s list: check that it is the fused AdaGrad rule
    over exactly `params` (each once, with its own accumulator of `owner`) and return
    (eta, eps).  Anything else -- another rule, a foreign parameter, a missing or repeated
    pair, mixed learning rates -- raises, since the kernels apply only that rule."""
    ids = {id(p): p for p in params}
    acc_seen, step_seen, rates = set(), set(), set()
    for lhs, rhs in updates:
        if isinstance(rhs, AccumulateSq):
            if not isinstance(lhs, Accumulator) or lhs._owner is not owner or lhs.param is not rhs.param:
                raise ValueError(f"accumulator pair {lhs!r} does not belong to this engine")
            key, seen = id(rhs.param), acc_seen
        elif isinstance(rhs, AdaGradStep):
            if lhs is not rhs.param or rhs.accumulator._owner is not owner:
                raise ValueError(f"update pair for {lhs!r} does not step that parameter")
            key, seen = id(rhs.param), step_seen
            rates.add((rhs.eta, rhs.eps))
        else:
            raise NotImplementedError(f"the HIP engines apply the AdaGrad rule only, not {type(rhs).__name__}")
        if key not in ids:
            raise ValueError(f"update targets a parameter this engine does not own: {rhs.param!r}")
        if key in seen:
            raise ValueError(f"parameter {rhs.param!r} updated twice")
        seen.add(key)
    if acc_seen != set(ids) or step_seen != set(ids):
        raise ValueError("updates must cover every parameter once (accumulator and step)")
    if len(rates) != 1:
        raise ValueError(f"one (eta, eps) per engine, got {sorted(rates)}")
    return rates.pop()


# ---------------------------------------------------------------- the layer stack's other rules
class StateView(Accumulator):
    """A state variable of one parameter in slot 0 or 1 of the layer-stack engine's optimiser
    state (the reference's `shared(np.zeros(...))`: v; g_ac and dx_ac; m and v): a live view.
    `owner` provides `_state_get(slot, param)` and `_state_set(slot, param, value)`."""

    def __init__(self, owner, param, slot, prefix):
        super().__init__(owner, param)
        self.slot = slot
        self.name = prefix + "_" + str(getattr(param, "name", "theta"))

    def get_value(self, borrow=False):
        return self._owner._state_get(self.slot, self.param)

    def set_value(self, value, borrow=False):
        self._owner._state_set(self.slot, self.param, np.asarray(value, np.float32))

    def __repr__(self):
        return f"StateView({self.name}, slot {self.slot})"


class Velocity(NamedTuple):
    """Right-hand side mu * v + T.grad(f, theta) (slot 0)."""
    param: object
    mu: float


class AscentStep(NamedTuple):
    """Right-hand side theta + eta * v_new (infalg.py:53 at mu = 0)."""
    param: object
    velocity: object
    eta: float


class DecayedSq(NamedTuple):
    """Right-hand side rho * g_ac + (1 - rho) * g ** 2 (infalg.py:98; slot 0)."""
    param: object
    rho: float


class AdaDeltaStep(NamedTuple):
    """Right-hand side theta + eta * T.sqrt(dx_ac + eps) * g / T.sqrt(g_ac_new + eps)
    (infalg.py:99,103; eta = 1 there)."""
    param: object
    g_ac: object
    dx_ac: object
    eta: float
    eps: float


class DecayedSqStep(NamedTuple):
    """Right-hand side rho * dx_ac + (1 - rho) * dx ** 2 (infalg.py:104; slot 1)."""
    param: object
    rho: float


class FirstMoment(NamedTuple):
    """Right-hand side beta1 * m + (1 - beta1) * g (slot 0)."""
    param: object
    beta1: float


class SecondMoment(NamedTuple):
    """Right-hand side beta2 * v + (1 - beta2) * g ** 2 (slot 1)."""
    param: object
    beta2: float


class AdamStep(NamedTuple):
    """Right-hand side theta + eta * (m_new / (1 - beta1^t)) / (T.sqrt(v_new / (1 - beta2^t)) + eps)."""
    param: object
    m: object
    v: object
    eta: float
    eps: float


class BoundRule(NamedTuple):
    """What `bind_rule` returns: the engine's rule name and vaeb_ae_optimizer's numbers."""
    rule: str
    eta: float
    beta1: float
    beta2: float
    eps: float


def _unit(name, v, low_open=False):
    if not (0 <= v < 1) or (low_open and not v > 0):
        raise ValueError(f"{name} must be greater than zero and less than one." if low_open
                         else f"{name} must be in [0, 1).")
    return float(v)


def _positive(name, v):
    if not v > 0:
        raise ValueError(f"{name} must be greater than zero.")   # infalg.py:62-66, 123-127
    return float(v)


class GradientAscent(InferenceAlgorithm):
    """infalg.py:44-74, with momentum: v' = mu v + g, theta' = theta + eta v'."""

    def __init__(self, eta, momentum=0.0):
        self.eta = eta
        self.momentum = momentum

    def name(self):
        return "(Stochastic) Gradient Ascent"

    def construct(self, f, theta):
        """Per parameter, (v, mu v + g) then (theta, theta + eta v')."""
        updates = []
        for t in theta:
            v = StateView(f, t, 0, "v")
            updates.append((v, Velocity(t, self.momentum)))
            updates.append((t, AscentStep(t, v, self.eta)))
        return updates

    def getinputs(self):
        return [self.eta]   # infalg.py:58-59

    eta = property(lambda self: self._eta, lambda self, v: setattr(self, "_eta", _positive("eta", v)))
    momentum = property(lambda self: self._mu, lambda self, v: setattr(self, "_mu", _unit("momentum", v)))


class AdaDelta(InferenceAlgorithm):
    """infalg.py:80-137 (Zeiler 2012, ascending); eta scales dx (1: the reference's rule)."""

    def __init__(self, rho=0.95, epsilon=1e-6, eta=1.0):
        self.rho = rho
        self.epsilon = epsilon
        self.eta = eta

    def name(self):
        return "AdaDelta (Zeiler 2012)"

    def construct(self, f, theta):
        """infalg.py:88-106: per parameter, (g_ac, ...), (theta, theta + dx), (dx_ac, ...)."""
        updates = []
        for t in theta:
            g_ac, dx_ac = StateView(f, t, 0, "g_ac"), StateView(f, t, 1, "dx_ac")
            updates.append((g_ac, DecayedSq(t, self.rho)))
            updates.append((t, AdaDeltaStep(t, g_ac, dx_ac, self.eta, self.epsilon)))
            updates.append((dx_ac, DecayedSqStep(t, self.rho)))
        return updates

    def getinputs(self):
        return []

    rho = property(lambda self: self._rho, lambda self, v: setattr(self, "_rho", _unit("rho", v, low_open=True)))
    epsilon = property(lambda self: self._eps, lambda self, v: setattr(self, "_eps", _positive("epsilon", v)))
    eta = property(lambda self: self._eta, lambda self, v: setattr(self, "_eta", _positive("eta", v)))


class Adam(InferenceAlgorithm):
    """Kingma & Ba 2015, ascending, with bias correction from the engine's optimiser-step counter."""

    def __init__(self, eta=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8):
        self.eta = eta
        self.beta1 = beta1
        self.beta2 = beta2
        self.epsilon = epsilon

    def name(self):
        return "Adam (Kingma & Ba 2015)"

    def construct(self, f, theta):
        """Per parameter, (m, ...), (v, ...) then (theta, theta + eta m_hat / (sqrt(v_hat) + eps))."""
        updates = []
        for t in theta:
            m, v = StateView(f, t, 0, "m"), StateView(f, t, 1, "v")
            updates.append((m, FirstMoment(t, self.beta1)))
            updates.append((v, SecondMoment(t, self.beta2)))
            updates.append((t, AdamStep(t, m, v, self.eta, self.epsilon)))
        return updates

    def getinputs(self):
        return []

    eta = property(lambda self: self._eta, lambda self, v: setattr(self, "_eta", _positive("eta", v)))
    beta1 = property(lambda self: self._b1, lambda self, v: setattr(self, "_b1", _unit("beta1", v)))
    beta2 = property(lambda self: self._b2, lambda self, v: setattr(self, "_b2", _unit("beta2", v)))
    epsilon = property(lambda self: self._eps, lambda self, v: setattr(self, "_eps", _positive("epsilon", v)))


# rule -> {right-hand side: (state slot or None for the parameter's own pair, its views' fields,
#                            {vaeb_ae_optimizer field: the record's field})}
_RULE_PAIRS = {
    "sga": {Velocity: (0, (), {"beta1": "mu"}), AscentStep: (None, ("velocity",), {"eta": "eta"})},
    "adadelta": {DecayedSq: (0, (), {"beta1": "rho"}),
                 AdaDeltaStep: (None, ("g_ac", "dx_ac"), {"eta": "eta", "eps": "eps"}),
                 DecayedSqStep: (1, (), {"beta1": "rho"})},
    "adam": {FirstMoment: (0, (), {"beta1": "beta1"}), SecondMoment: (1, (), {"beta2": "beta2"}),
             AdamStep: (None, ("m", "v"), {"eta": "eta", "eps": "eps"})},
}


def bind_rule(owner, params, updates):
    """What the layer-stack engine does with `construct`'s list: `bind_updates`' checks for any of
    its four rules -- every parameter once per pair kind, the state views being `owner`'s own, one
    set of hyper-parameters, one rule -- and the `BoundRule` to hand to vaeb_ae_set_optimizer."""
    updates = list(updates)
    kinds = {type(rhs) for _, rhs in updates}
    if kinds <= {AccumulateSq, AdaGradStep}:
        eta, eps = bind_updates(owner, params, updates)
        return BoundRule("adagrad", eta, 0.0, 0.0, eps)
    rule = next((r for r, pairs in _RULE_PAIRS.items() if kinds and kinds <= set(pairs)), None)
    if rule is None:
        raise NotImplementedError("the layer-stack engine applies AdaGrad, GradientAscent, AdaDelta or Adam, "
                                  f"one rule per model, not {sorted(k.__name__ for k in kinds)}")
    ids = {id(p): p for p in params}
    seen = {k: set() for k in _RULE_PAIRS[rule]}
    hyper = {"eta": set(), "beta1": set(), "beta2": set(), "eps": set()}
    for lhs, rhs in updates:
        slot, views, fields = _RULE_PAIRS[rule][type(rhs)]
        if slot is None:
            if lhs is not rhs.param:
                raise ValueError(f"update pair for {lhs!r} does not step that parameter")
            states = [getattr(rhs, v) for v in views]
        else:
            if not isinstance(lhs, StateView) or lhs.slot != slot or lhs.param is not rhs.param:
                raise ValueError(f"state pair {lhs!r} is not slot {slot} of its parameter")
            states = [lhs]
        if any(not isinstance(s, StateView) or s._owner is not owner for s in states):
            raise ValueError(f"state of the pair for {rhs.param!r} does not belong to this engine")
        key = id(rhs.param)
        if key not in ids:
            raise ValueError(f"update targets a parameter this engine does not own: {rhs.param!r}")
        if key in seen[type(rhs)]:
            raise ValueError(f"parameter {rhs.param!r} updated twice")
        seen[type(rhs)].add(key)
        for k, f in fields.items():
            hyper[k].add(getattr(rhs, f))
    if any(s != set(ids) for s in seen.values()):
        raise ValueError("updates must cover every parameter once (each state and the step)")
    if any(len(v) > 1 for v in hyper.values()):
        raise ValueError(f"one set of hyper-parameters per engine, got {({k: sorted(v) for k, v in hyper.items()})}")
    return BoundRule(rule, *(float(next(iter(hyper[k]), 0.0)) for k in ("eta", "beta1", "beta2", "eps")))
