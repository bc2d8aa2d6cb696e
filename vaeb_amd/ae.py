"""Host mirror of /root/reference/degenerate-vae/ae.py over the HIP autoencoder engine.

`ConstructAE(Xtr, Denc, Dz, Ddec, f, s2, inf, otype)` keeps the reference's signature and
returns the same five things (ae.py:41-117): `train(idx)` (one AdaGrad step on the rows
Xtr[idx], returning loglik / len(idx)), `reconstruct(X)`, `encode(X)`, `decode(Z)` and
`theta`, a list of parameters with `get_value()` / `set_value()` in the reference order.
All compute runs in libvaeb_hip.so (vaeb_ae_*, vaeb_amd/csrc/ae_mlp.hpp); there is no CPU
fallback.  Initialisation draws every weight and bias from the GLOBAL numpy RNG in the
reference's construction order (mlp.py:36-49), so `numpy.random.seed(s)` before
ConstructAE reproduces the reference's theta_0.

`ConstructVAE` (extension) is the same constructor with a Gaussian latent: mu and log-variance
heads, z = mu + exp(lv / 2) eps with device Philox noise, and train(idx) returning
(loglik - KL) / len(idx) (include/vaeb_hip.h enum vaeb_ae_latent).

`ConstructVanillaAE` mirrors the reference's vanilla-ae/ae.py:45-112, the squared-error baseline of
its report: the code goes through f, Z = f(Hz Wz + bz), there is no prior on Z, the output is
Xpr = sigmoid(.), logjoint = -se + weight decay, and train(idx) returns se / len(idx).

Denoising training (extension; the reference report's "Scheduled VAEB" follow-up): each constructor
takes `corruption=` "mask" | "saltpepper" | "gauss" or (kind, level) and an optional
`corruption_seed`.  The encoder then reads the rows corrupted at the current noise level while the
output is scored on the clean rows (include/vaeb_hip.h enum vaeb_ae_corruption): the denoising
autoencoder, and with ConstructVAE the denoising VAE.  train.set_noise(level), train.noise and
train.corrupt(idx) steer and show the corruption; noise_schedule and train_epochs(noise=...) run a
schedule of falling levels.

Two-mode latent prior (extension; the report's "Latent space priors" follow-up): ConstructVAE takes
`prior=` "twomode", ("twomode", width) or ("twomode", mean1, width).  Each latent dimension then has
the prior 1/2 N(0, width^2) + 1/2 N(mean1, width^2) (include/vaeb_hip.h enum vaeb_ae_prior), which
pulls the posterior means towards {0, mean1}; train.code(X) truncates them to Dz bits per row and
train.decode_code(bits) decodes such codes.  train.set_prior(width=...) between epochs runs a schedule
of falling widths.

Update rules (the reference's other optimisers, infalg.py:44-137, and Adam): each constructor's `inf`
may be infalg.AdaGrad (the default, AdaGrad(0.01), with theta_0, the context and the steps as ever),
GradientAscent(eta, momentum), AdaDelta(rho, epsilon, eta) or Adam(eta, beta1, beta2, epsilon); the rule
runs in the weight-gradient kernels' epilogue (include/vaeb_hip.h enum vaeb_ae_rule).  Every train has
train.optimizer (the rule and its numbers as the engine holds them), train.set_eta(eta) (a step-size
schedule between calls; the optimiser state is kept) and, under GradientAscent(eta, momentum=0),
train.last_gradient() (the last step's gradient, one array per parameter).
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .infalg import AdaGrad, BoundRule, bind_rule

_ACT_NAMES = {"tanh": "tanh", "sigmoid": "sigmoid", "logistic": "sigmoid", "relu": "relu"}


def _act_name(f):
    key = f if isinstance(f, str) else getattr(f, "__name__", str(f))
    key = key.split(".")[-1].lower()
    if key not in _ACT_NAMES:
        raise ValueError(f"activation {f!r} not supported (tanh | sigmoid | relu)")
    return _ACT_NAMES[key]


def _values(X):
    return np.asarray(X.get_value() if hasattr(X, "get_value") else X, np.float32)


def param_shapes(Dobs, Denc, Dz, Ddec, otype, latent="point"):
    """theta order of ae.py:51,56,64,72; latent="gauss": [Wz, bz] become
    [Wzmu, Wzlv, bzmu, bzlv] (the cont output's convention); latent="act" (the vanilla autoencoder's
    activated code) has the point layout, otype="se" the binary tail [Wout, bout]."""
    d_in = [Dobs] + list(Denc)
    shp = [(f"W{i}", (d_in[i], d_in[i + 1])) for i in range(len(Denc))]
    shp += [(f"b{i}", (Denc[i],)) for i in range(len(Denc))]
    if latent == "gauss":
        shp += [("Wzmu", (Denc[-1], Dz)), ("Wzlv", (Denc[-1], Dz)), ("bzmu", (Dz,)), ("bzlv", (Dz,))]
    elif latent in ("point", "act"):
        shp += [("Wz", (Denc[-1], Dz)), ("bz", (Dz,))]
    else:
        raise ValueError(f"latent {latent!r} not supported (point | gauss | act)")
    d_dec = [Dz] + list(Ddec)
    shp += [(f"W{i}", (d_dec[i], d_dec[i + 1])) for i in range(len(Ddec))]
    shp += [(f"b{i}", (Ddec[i],)) for i in range(len(Ddec))]
    if otype in ("binary", "se"):
        shp += [("Wout", (Ddec[-1], Dobs)), ("bout", (Dobs,))]
    else:
        shp += [("Wmu", (Ddec[-1], Dobs)), ("Wlogs2", (Ddec[-1], Dobs)), ("bmu", (Dobs,)), ("blogs2", (Dobs,))]
    return shp


class SharedParam:
    """A slice of the device parameter arena with the Theano shared-variable accessors."""

    def __init__(self, ctx, name, shape, offset):
        self.ctx, self.name, self.shape, self.offset = ctx, name, shape, offset
        self.size = int(np.prod(shape))

    def get_value(self):
        return self.ctx.get_params()[self.offset:self.offset + self.size].reshape(self.shape).copy()

    def set_value(self, v):
        flat = self.ctx.get_params()
        flat[self.offset:self.offset + self.size] = np.asarray(v, np.float32).ravel()
        self.ctx.set_params(flat)

    def __repr__(self):
        return f"SharedParam({self.name}, {self.shape})"


class _AccArena:
    """Owner of the optimiser state `inf.construct` hands out: views of the engine's state arenas,
    one slice per SharedParam -- slot 0 (the AdaGrad accumulators; v; g_ac; m) and slot 1 (dx_ac; v)."""

    def __init__(self, ctx):
        self.ctx = ctx

    def _acc_get(self, p):
        return self.ctx.get_adagrad_state()[p.offset:p.offset + p.size].reshape(p.shape).copy()

    def _acc_set(self, p, value):
        flat = self.ctx.get_adagrad_state()
        flat[p.offset:p.offset + p.size] = value.ravel()
        self.ctx.set_adagrad_state(flat)

    def _state_get(self, slot, p):
        return self.ctx.get_opt_state(slot)[p.offset:p.offset + p.size].reshape(p.shape).copy()

    def _state_set(self, slot, p, value):
        flat = self.ctx.get_opt_state(slot)
        flat[p.offset:p.offset + p.size] = value.ravel()
        self.ctx.set_opt_state(slot, flat)


CORRUPTIONS = ("mask", "saltpepper", "gauss")


def _corruption(corruption):
    """(kind, level) of a constructor's corruption argument: None, a kind, or (kind, level)."""
    if corruption is None:
        return "none", 0.0
    kind, level = (corruption, 0.0) if isinstance(corruption, str) else corruption
    if kind not in CORRUPTIONS:
        raise ValueError(f"corruption {kind!r} not supported (mask | saltpepper | gauss)")
    return kind, float(level)


class _Train:
    """train(idx): one step of the engine on the rows Xtr[idx], returning its value; with the
    update rule of the steps to come (optimizer / set_eta) and the gradient read-out."""

    def __init__(self, ctx, theta):
        self.ctx, self._theta = ctx, theta

    def __call__(self, idx):
        return self.ctx.train(np.asarray(idx, np.int32))

    @property
    def optimizer(self):
        """BoundRule(rule, eta, beta1, beta2, eps) as the engine holds it."""
        return BoundRule(*self.ctx.get_optimizer())

    def set_eta(self, eta):
        """The step size of the steps to come, state and step counter kept: a schedule."""
        rule, _, b1, b2, eps = self.ctx.get_optimizer()
        self.ctx.set_optimizer(rule, eta, b1, b2, eps)

    def last_gradient(self):
        """The last step's gradient of the objective (the prior on theta included), one array per
        parameter: what GradientAscent(momentum=0) leaves in state slot 0."""
        o = self.optimizer
        if o.rule != "sga" or o.beta1 != 0:
            raise ValueError("last_gradient() needs inf=GradientAscent(eta, momentum=0): only that rule stores the gradient")
        flat = self.ctx.get_opt_state(0)
        return [flat[p.offset:p.offset + p.size].reshape(p.shape).copy() for p in self._theta]


class _DenoisingTrain(_Train):
    """train(idx) of a corrupting context: with the noise level of the steps to come (set_noise /
    noise) and the corrupted rows a step would read."""

    def set_noise(self, level):
        self.ctx.set_corruption_level(level)

    @property
    def noise(self):
        return self.ctx.get_corruption_level()

    def corrupt(self, idx):
        return self.ctx.corrupt(np.asarray(idx, np.int32))


def _prior(prior):
    """(mean1, width) of ConstructVAE's prior argument, None for the N(0, 1) prior: None, "twomode",
    ("twomode", width) or ("twomode", mean1, width)."""
    if prior is None:
        return None
    name, *rest = (prior,) if isinstance(prior, str) else tuple(prior)
    if name != "twomode" or len(rest) > 2:
        raise ValueError(f"prior {prior!r} not supported (None | 'twomode' | ('twomode', width) | "
                         "('twomode', mean1, width))")
    mean1, width = {0: (1.0, 0.25), 1: (1.0, *rest), 2: tuple(rest)}[len(rest)]
    return float(mean1), float(width)


class _TwoModeTrain:
    """train(idx) of a context with the two-mode latent prior: the wrapped train function (its
    attributes included) with the prior of the steps to come (set_prior / prior) and the binary
    codes (code / decode_code / code_bits_per_row)."""

    def __init__(self, train, ctx):
        self._train, self.ctx = train, ctx
        self.code_bits_per_row = ctx.Dz

    def __call__(self, idx):
        return self._train(idx)

    def __getattr__(self, name):   # only what the instance itself lacks: set_noise, noise, corrupt
        return getattr(self._train, name)

    def set_prior(self, mean1=None, width=None):
        a, s = self.ctx.get_prior()
        self.ctx.set_prior(a if mean1 is None else mean1, s if width is None else width)

    @property
    def prior(self):
        """(mean1, width)."""
        return self.ctx.get_prior()

    def code(self, X):
        """bool [n x Dz]: encode(X) >= mean1 / 2, the posterior mean truncated to its nearer mode."""
        words = self.ctx.encode_bits(_values(X))
        j = np.arange(self.ctx.Dz)
        return ((words[:, j // 32] >> (j % 32).astype(np.uint32)) & 1).astype(bool)

    def decode_code(self, bits):
        """The decoder's output [n x Dobs] for codes [n x Dz] (bool or 0 / 1): z = mean1 where set, else 0."""
        bits = np.asarray(bits)
        if bits.ndim != 2 or bits.shape[1] != self.ctx.Dz or not np.isin(bits, (0, 1)).all():
            raise ValueError(f"codes must be a bool or 0 / 1 array [n x {self.ctx.Dz}]")
        j = np.arange(self.ctx.Dz)
        words = np.zeros((bits.shape[0], -(-self.ctx.Dz // 32)), np.uint32)
        np.bitwise_or.at(words, (slice(None), j // 32), bits.astype(np.uint32) << (j % 32).astype(np.uint32))
        return self.ctx.decode_bits(words)


def _construct(latent, Xtr, Denc, Dz, Ddec, f, s2, inf, otype, max_batch, device, iw_samples=1, corruption=None,
               corruption_seed=0, prior="normal"):
    """The shared body of ConstructAE / ConstructVAE / ConstructVanillaAE; returns (train, ctx, theta),
    train(idx) being one step of the engine on the rows Xtr[idx] with train.ctx = ctx."""
    kind, level = _corruption(corruption)
    if otype not in ("binary", "cont") and (latent, otype) != ("act", "se"):
        raise ValueError("otype currently only supports binary.")   # ae.py:74-75 (and cont)
    inf = inf if inf is not None else AdaGrad(0.01)
    Xtr = _values(Xtr)
    Denc, Ddec = list(Denc), list(Ddec)
    Dobs = Xtr.shape[1]
    shapes = param_shapes(Dobs, Denc, Dz, Ddec, otype, latent)
    # mlp.WeightMatrix / BiasVector: N(0, 0.01) from the global RNG, construction order
    theta0 = [np.random.normal(0.0, 0.01, size=s).astype(np.float32) for _, s in shapes]
    K = max(1, int(iw_samples))   # the K sample planes of a step are stacked inside max_batch
    mb = int(max_batch) if max_batch else max(100 * K, min(4096, Xtr.shape[0]))
    ctx = _lib.AEContext(Dobs, Denc, Dz, Ddec, otype=otype, act=_act_name(f), s2=s2, eta=inf.eta, max_batch=mb,
                         device=device, latent=latent, iw_samples=iw_samples, corruption=kind, prior=prior)
    ctx.set_data(Xtr)
    ctx.set_params(np.concatenate([t.ravel() for t in theta0]))
    offs = np.cumsum([0] + [int(np.prod(s)) for _, s in shapes])
    theta = [SharedParam(ctx, n, s, int(o)) for (n, s), o in zip(shapes, offs[:-1])]
    # ae.py:80: updates = inf.construct(logjoint, theta), bound to the engine's fused rule.  AdaGrad
    # is the context's own from vaeb_ae_create (eta above); any other rule is set once
    arena = _AccArena(ctx)
    updates = inf.construct(arena, theta)
    bound = bind_rule(arena, theta, updates)
    if bound.rule != "adagrad":
        ctx.set_optimizer(*bound)

    if kind != "none":
        ctx.set_corruption_noise(_lib.EPS_PHILOX, corruption_seed)
        ctx.set_corruption_level(level)
        return _DenoisingTrain(ctx, theta), ctx, theta
    return _Train(ctx, theta), ctx, theta


def ConstructAE(Xtr, Denc=(500,), Dz=20, Ddec=(500,), f="tanh", s2=1.0, inf=None, otype="binary",
                max_batch=None, device=0, corruption=None, corruption_seed=0):
    """ae.py:41-117.  Returns (train, reconstruct, encode, decode, theta).  corruption: the denoising
    autoencoder (module docstring); None: the reference's model, theta_0 and steps."""
    train, ctx, theta = _construct("point", Xtr, Denc, Dz, Ddec, f, s2, inf, otype, max_batch, device,
                                   corruption=corruption, corruption_seed=corruption_seed)
    return train, ctx.reconstruct, ctx.encode, ctx.decode, theta


def ConstructVAE(Xtr, Denc=(500,), Dz=20, Ddec=(500,), f="tanh", s2=1.0, inf=None, otype="binary", seed=10,
                 max_batch=None, device=0, iw_samples=1, corruption=None, corruption_seed=0, prior=None):
    """ConstructAE with a Gaussian latent: the same five return values, theta in the order
    [..., Wzmu, Wzlv, bzmu, bzlv, ...].  train(idx) takes one AdaGrad step on the ELBO of the
    rows Xtr[idx] (one Philox draw per row and latent, keyed by `seed`, the dataset row and the
    step) and returns (loglik - KL) / len(idx); encode(X) is mu, reconstruct(X) decodes z = mu.
    train.ctx is the engine context; train.elbo(X) the forward-only sum of loglik - KL;
    train.marginal_ll(X, K, rows=False) the K-sample importance-weighted estimate of
    sum_i log p(x_i) with the encoder as the proposal (forward only; rows=True: (sum, per-row
    values) -- the figure that ranks a deep model against the one-hidden-layer VAEB's
    marginal_likelihood).  iw_samples = K >= 2: train(idx) steps on the K-sample importance-weighted
    bound instead (K draws per row, sample stream k) and returns that bound / len(idx); a step needs
    K * len(idx) <= max_batch, which defaults to max(100 K, min(4096, N)).  train.iw_samples is K.
    corruption: the denoising VAE (the encoder sees the corrupted rows, the bound is scored on the clean
    ones; `corruption_seed` keys the corruption, `seed` the latent noise).
    prior: "twomode", ("twomode", width) or ("twomode", mean1, width) (defaults 1 and 0.25): the
    two-mode latent prior of the module docstring, with every iw_samples and corruption.  train(idx)
    then returns (loglik + latent_row) / len(idx), the prior term taken at the step's sample, and
    train gains set_prior(mean1=None, width=None), prior, code(X), decode_code(bits) and
    code_bits_per_row (= Dz).  None: the N(0, 1) prior, with theta_0, context and steps as ever."""
    two = _prior(prior)   # raises before a context is made
    train, ctx, theta = _construct("gauss", Xtr, Denc, Dz, Ddec, f, s2, inf, otype, max_batch, device, iw_samples,
                                   corruption=corruption, corruption_seed=corruption_seed,
                                   prior="twomode" if two else "normal")
    if two:
        ctx.set_prior(*two)
        train = _TwoModeTrain(train, ctx)
    ctx.set_eps_mode(_lib.EPS_PHILOX, seed)
    train.iw_samples = ctx.iw_samples
    train.elbo = lambda X: ctx.elbo(_values(X))
    train.marginal_ll = lambda X, K, rows=False: ctx.marginal_ll(_values(X), K, rows=rows)
    return train, ctx.reconstruct, ctx.encode, ctx.decode, theta


def ConstructVanillaAE(Xtr, Denc=(500,), Dz=20, Ddec=(500,), f="tanh", s2=1.0, inf=None, max_batch=None, device=0,
                       corruption=None, corruption_seed=0):
    """vanilla-ae/ae.py:45-112.  Returns (train, reconstruct, encode, decode, theta): train(idx) takes
    one AdaGrad step up -se + weight decay on the rows Xtr[idx] and returns se / len(idx) (positive);
    encode(X) is the activated code f(Hz Wz + bz).  theta_0 is drawn from the global numpy RNG in the
    order of ConstructAE with a binary output.  train.ctx is the engine context; train.mse(X) is
    mse(X, reconstruct(X)) computed on the device (vaeb_ae_sq_error), nothing but the sum coming back.
    corruption: the denoising autoencoder; train.mse(X) stays the clean reconstruction error."""
    train, ctx, theta = _construct("act", Xtr, Denc, Dz, Ddec, f, s2, inf, "se", max_batch, device,
                                   corruption=corruption, corruption_seed=corruption_seed)

    def device_mse(X):
        X = _values(X)
        return ctx.sq_error(X) / X.shape[0]

    train.mse = device_mse
    return train, ctx.reconstruct, ctx.encode, ctx.decode, theta


def mse(X, Xpr):
    """vanilla-ae/ae.py:120-121."""
    return float(np.mean(np.sum((X - Xpr) ** 2, 1)))


def rmse(X, Xpr):
    """ae.py:121-122."""
    return float(np.sqrt(np.mean(np.sum((X - Xpr) ** 2, 1))))


def noise_schedule(levels, epochs):
    """The per-epoch noise levels of a schedule of len(levels) stages over `epochs` epochs: epoch e
    uses levels[min(len(levels) - 1, e * len(levels) // epochs)]."""
    levels = list(levels)
    if not levels:
        raise ValueError("noise_schedule needs at least one level")
    return [levels[min(len(levels) - 1, e * len(levels) // epochs)] for e in range(epochs)]


def train_epochs(train, Ntr, epochs, batch_size=100, verbose=True, noise=None):
    """The LearnMNIST / LearnFreyFace loop (ae.py:140-151, 179-190): a fresh global-RNG
    permutation per epoch, batches of batch_size with the last partial batch kept.  The
    whole epoch is enqueued with one host sync (vaeb_ae_train_many).  noise: one level per epoch
    (noise_schedule), set before the epoch's steps on a train built with a corruption."""
    if noise is not None and len(noise) != epochs:
        raise ValueError(f"noise holds {len(noise)} levels for {epochs} epochs")
    loglik = []
    for i in range(epochs):
        if noise is not None:
            train.set_noise(noise[i])
        idx = np.random.permutation(np.arange(Ntr)).astype(np.int32)
        loglik.extend(train.ctx.train_many(idx, batch_size).tolist())
        if verbose:
            print("Epoch " + str(i) + ". mean loglik = " + str(loglik[-1]))
    return loglik


def LearnAE(Xtr, Xte, epochs, Dz, hidden, otype, batch_size=100, verbose=True):
    """Shared body of LearnFreyFace (ae.py:130-162) / LearnMNIST (ae.py:169-201), minus the
    matplotlib learning-curve file; returns (reconstruct, encode, decode, loglik, rmse_tr, rmse_te)."""
    train, reconstruct, encode, decode, theta = ConstructAE(Xtr, Denc=[hidden], Dz=Dz, Ddec=[hidden], otype=otype,
                                                            inf=AdaGrad(0.01))
    if verbose:
        print("Training the autoencoder.")
    loglik = train_epochs(train, Xtr.shape[0], epochs, batch_size, verbose)
    rtr, rte = rmse(Xtr, reconstruct(Xtr)), rmse(Xte, reconstruct(Xte))
    if verbose:
        print("training rmse = " + str(rtr))
        print("testing rmse = " + str(rte))
    return reconstruct, encode, decode, loglik, rtr, rte
