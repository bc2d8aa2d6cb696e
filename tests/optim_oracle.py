"""The layer-stack engine's update rules (vaeb_amd/csrc/ae_mlp.hpp PAeWgradT<RULE>, include/vaeb_hip.h
enum vaeb_ae_rule) in NumPy -- TEST HELPER ONLY.

Each rule is a dtype-generic function  (theta, s0, s1, g, hyper, t) -> (theta', s0', s1')  on one
array; all ASCEND the objective whose gradient g = oracle.ae_oracle.forward_backward(...)["grads"]
is (the prior's -theta / s2 included).  The dtype of theta is the dtype of the arithmetic: fed
float64 arrays a rule is the oracle, fed float32 arrays (float32 gradients from the float32-fed
forward_backward) it is the float32 restatement of the device's epilogue, operation by operation.

  adagrad   (infalg.py:148-164)  s0' = s0 + g^2;  theta' = theta + eta g / (sqrt(s0') + 1e-6)
  sga       (infalg.py:44-74, plus momentum)  s0' = mu s0 + g;  theta' = theta + eta s0'
  adadelta  (infalg.py:88-106)   s0' = rho s0 + (1 - rho) g^2;  dx = sqrt(s1 + eps) g / sqrt(s0' + eps);
                                 theta' = theta + eta dx;  s1' = rho s1 + (1 - rho) dx^2
  adam      s0' = b1 s0 + (1 - b1) g;  s1' = b2 s1 + (1 - b2) g^2;
            theta' = theta + eta (s0' / bc1) / (sqrt(s1' / bc2) + eps),  bc_i = 1 - b_i^t

The hyper-parameters are the ABI's: float32 values (Hyper rounds them once), so the float64 oracle
and the device start from the same numbers, as they do from the same float32 theta.  bc1 / bc2 are
formed in double from the float32 beta and the optimiser step t (the first step is t = 1) and then
cast to the dtype of the run: the engine forms them on the host in double and passes floats.
One-slot rules return s1 unchanged (None stays None).
"""
import dataclasses

import numpy as np

from oracle import ae_oracle as A

RULES = ("adagrad", "sga", "adadelta", "adam")
ADAGRAD_EPS = 1e-6
SLOTS = {"adagrad": 1, "sga": 1, "adadelta": 2, "adam": 2}


def _f32(x):
    return float(np.float32(x))


@dataclasses.dataclass(frozen=True)
class Hyper:
    """(rule, eta, beta1, beta2, eps) as vaeb_ae_optimizer holds them: beta1 is mu (sga), rho
    (adadelta) or beta1 (adam); unused fields are 0 (adagrad: eps 1e-6)."""
    rule: str
    eta: float
    beta1: float = 0.0
    beta2: float = 0.0
    eps: float = 0.0

    def __post_init__(self):
        assert self.rule in RULES
        for k in ("eta", "beta1", "beta2", "eps"):
            object.__setattr__(self, k, _f32(getattr(self, k)))

    def abi(self):
        return self.rule, self.eta, self.beta1, self.beta2, self.eps


def adagrad_hyper(eta):
    return Hyper("adagrad", eta, eps=ADAGRAD_EPS)


def bias_corrections(h, t):
    """(bc1, bc2) in double from the float32 betas."""
    return 1.0 - h.beta1 ** int(t), 1.0 - h.beta2 ** int(t)


def adagrad(th, s0, s1, g, h, t):
    dt = th.dtype.type
    a2 = s0 + g * g
    return th + dt(h.eta) * g / (np.sqrt(a2) + dt(1e-6)), a2, s1


def sga(th, s0, s1, g, h, t):
    dt = th.dtype.type
    v = dt(h.beta1) * s0 + g
    return th + dt(h.eta) * v, v, s1


def adadelta(th, s0, s1, g, h, t):
    dt = th.dtype.type
    rho, eps = dt(h.beta1), dt(h.eps)
    g_ac = rho * s0 + (dt(1) - rho) * (g * g)
    dx = np.sqrt(s1 + eps) * g / np.sqrt(g_ac + eps)
    return th + dt(h.eta) * dx, g_ac, rho * s1 + (dt(1) - rho) * (dx * dx)


def adam(th, s0, s1, g, h, t):
    dt = th.dtype.type
    b1, b2 = dt(h.beta1), dt(h.beta2)
    bc1, bc2 = (dt(b) for b in bias_corrections(h, t))
    m = b1 * s0 + (dt(1) - b1) * g
    v = b2 * s1 + (dt(1) - b2) * (g * g)
    return th + dt(h.eta) * (m / bc1) / (np.sqrt(v / bc2) + dt(h.eps)), m, v


RULE_FN = {"adagrad": adagrad, "sga": sga, "adadelta": adadelta, "adam": adam}


def apply(params, S0, S1, grads, h, t, fn=None):
    """One optimiser step at step number t on lists of arrays of one dtype: (theta', S0', S1').
    fn: another rule function in place of h's own (the wrong rules of the host test)."""
    fn = fn or RULE_FN[h.rule]
    dt = params[0].dtype
    out = ([], [], [])
    for th, s0, s1, g in zip(params, S0, S1, grads):
        assert th.dtype == s0.dtype == g.dtype == dt and (s1 is None or s1.dtype == dt)
        for lst, a in zip(out, fn(th, s0, s1, g, h, t)):
            lst.append(a if a is None else np.asarray(a, dt))
    return out


def as_dtype(arrays, dt):
    return [None if a is None else np.asarray(a, dt) for a in arrays]


def trajectory(cfg, params, S0, S1, Xtr, batches, h, t0, dt, eps=None, **kw):
    """len(batches) steps of rule h from (params, S0, S1) in dtype dt, the first at step number
    t0 + 1.  eps: None, [n x Dz] (row i of the concatenated batches) or [K x n x Dz] (the
    importance-weighted form); kw: forward_backward's (latent=...).  Returns (values / M, theta,
    S0, S1)."""
    p, s0, s1 = as_dtype(params, dt), as_dtype(S0, dt), as_dtype(S1, dt)
    X = np.asarray(Xtr, dt)
    vals, lb = [], 0
    for j, b in enumerate(batches):
        e = None if eps is None else np.asarray(eps[..., lb:lb + len(b), :], dt)
        ekw = {} if e is None else {"eps": e}
        out = A.forward_backward(p, X[np.asarray(b)], cfg, **kw, **ekw)
        vals.append(out["value"] / len(b))
        p, s0, s1 = apply(p, s0, s1, out["grads"], h, t0 + 1 + j)
        lb += len(b)
    return vals, p, s0, s1
