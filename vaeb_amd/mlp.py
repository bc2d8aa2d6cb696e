"""Host mirror of the reference's degenerate-vae/mlp.py classifiers over the HIP layer-stack engine
(vaeb_clf_*, vaeb_amd/csrc/engine_clf.inc, clf_softmax.hpp); there is no CPU fallback.

`ConstructPMLPClassifier(Din, Dh, Dout, f, s2, inf)` (mlp.py:104-153) is the MAP classifier: hidden
layers of f, a softmax output, logjoint = bernoulli(Y, Ypr) summed over the rows -- the reference
builds the N(0, s2) prior and leaves it out of logjoint, so `prior=False` is the default and
`prior=True` the extension that adds it.  It returns the reference's four things:
`buildtraining(Xtr, Ytr)` -> `train(lb, ub)` (one step on the contiguous rows [lb, ub), returning the
step's log-likelihood sum), `predict(X)`, `computelogjoint(X, Y)` and `theta`, a list of parameters
with get_value() / set_value() in the reference order W0.., b0.., Wout, bout.

`ConstructBayesianMLPClassifier(..., keep=0.5, seed=15485863)` (mlp.py:263-329) multiplies every
weight and bias by a fresh Bernoulli(keep) draw per call (device Philox keyed by `seed`): its
`predict(X, L=1)` is the mean over L stochastic passes and `computeelbo(X, Y, draw=0)` one such pass.

Every array of theta_0 is N(0, 0.01) from the GLOBAL numpy RNG in construction order (all W, all b,
then Wout, bout; WeightMatrices / BiasVectors below), so numpy.random.seed(s) before a constructor
reproduces the reference's theta_0.  `inf` is any of infalg.AdaGrad | GradientAscent | AdaDelta | Adam.
Beyond the reference, train has .idx(idx) (any row list), .many(idx, batch) (an epoch with one host
sync), .optimizer, .set_eta(eta) and .last_gradient(), as the autoencoders' train has; loss="categorical"
scores the softmax with sum Y log P instead.

    python -m vaeb_amd.mlp --synthetic [--bayesian --L 20 --keep 0.5 --optimizer adam --eta 1e-3
                                        --hidden 500,300 --epochs N --loss categorical]
"""
from __future__ import annotations

import argparse

import numpy as np

from . import _lib
from .ae import SharedParam, _AccArena, _Train, _act_name, _values
from .infalg import AdaDelta, AdaGrad, Adam, GradientAscent, bind_rule

SEED = 15485863   # the reference's stream seed (mlp.py:18)


def WeightMatrix(Din, Dout, name=None):
    """mlp.py:48-49: N(0, 0.01) [Din x Dout] from the global RNG."""
    return np.random.normal(0.0, 0.01, size=(Din, Dout)).astype(np.float32)


def BiasVector(D, name=None):
    """mlp.py:36-37."""
    return np.random.normal(0.0, 0.01, size=(D)).astype(np.float32)


def WeightMatrices(D):
    """mlp.py:43-44: one matrix per consecutive pair of the sizes D, drawn in that order."""
    out = []
    for k, (rows, cols) in enumerate(zip(D[:-1], D[1:])):
        out.append(WeightMatrix(rows, cols, f"W{k}"))
    return out


def BiasVectors(D):
    """mlp.py:31-32: one vector per size in D, drawn in that order."""
    out = []
    for k, width in enumerate(D):
        out.append(BiasVector(width, f"b{k}"))
    return out


def param_shapes(Din, Dh, Dout):
    """theta order of mlp.py:113 / :277."""
    d = [Din] + list(Dh)
    shp = [(f"W{i}", (d[i], d[i + 1])) for i in range(len(Dh))]
    shp += [(f"b{i}", (Dh[i],)) for i in range(len(Dh))]
    return shp + [("Wout", (Dh[-1], Dout)), ("bout", (Dout,))]


class _ClfTrain(_Train):
    """train(lb, ub): one step on the resident rows [lb, ub) (mlp.py:133), returning the step's
    log-likelihood sum; .idx(idx) the same on any row list, .many(idx, batch) consecutive batches of
    a list with one host sync (the last partial one kept)."""

    def __call__(self, lb, ub):
        return self.ctx.train(np.arange(int(lb), int(ub), dtype=np.int32))

    def idx(self, idx):
        return self.ctx.train(np.asarray(idx, np.int32))

    def many(self, idx, batch):
        return self.ctx.train_many(np.asarray(idx, np.int32), batch)


def _construct(Din, Dh, Dout, f, s2, inf, dropout, keep, seed, loss, prior, max_batch, device):
    Dh = list(Dh)
    inf = inf if inf is not None else AdaGrad(0.01)
    s2 = float(np.ravel(s2)[0])   # the reference passes one variance per parameter, all equal
    theta0 = WeightMatrices([Din] + Dh) + BiasVectors(Dh) + [WeightMatrix(Dh[-1], Dout, "Wout"), BiasVector(Dout, "bout")]
    ctx = _lib.CLFContext(Din, Dh, Dout, act=_act_name(f), loss=loss, prior=prior, s2=s2, eta=inf.eta,
                          max_batch=max_batch, device=device, dropout=dropout, keep=keep)
    ctx.set_seed(seed)
    ctx.set_params(np.concatenate([t.ravel() for t in theta0]))
    shapes = param_shapes(Din, Dh, Dout)
    offs = np.cumsum([0] + [int(np.prod(s)) for _, s in shapes])
    theta = [SharedParam(ctx, n, s, int(o)) for (n, s), o in zip(shapes, offs[:-1])]
    arena = _AccArena(ctx)
    bound = bind_rule(arena, theta, inf.construct(arena, theta))
    if bound.rule != "adagrad":
        ctx.set_optimizer(*bound)

    def buildtraining(Xtr, Ytr):
        ctx.set_data(_values(Xtr), _values(Ytr))
        return _ClfTrain(ctx, theta)

    buildtraining.ctx = ctx
    return buildtraining, ctx, theta


def ConstructPMLPClassifier(Din, Dh, Dout, f="tanh", s2=1.0, inf=None, loss="bernoulli", prior=False,
                            max_batch=4096, device=0):
    """mlp.py:104-153.  Returns (buildtraining, predict, computelogjoint, theta); buildtraining.ctx is
    the engine context.  computelogjoint(X, Y) is the log-likelihood sum (no prior term, as the
    reference's logjoint)."""
    buildtraining, ctx, theta = _construct(Din, Dh, Dout, f, s2, inf, False, 1.0, 0, loss, prior, max_batch, device)
    return buildtraining, (lambda X: ctx.predict(_values(X))), \
        (lambda X, Y: ctx.loglik(_values(X), _values(Y))), theta


def ConstructBayesianMLPClassifier(Din, Dh, Dout, f="tanh", s2=1.0, inf=None, keep=0.5, seed=SEED, loss="bernoulli",
                                   prior=False, max_batch=4096, device=0):
    """mlp.py:263-329 (weight dropout; the reference's keep is 0.5).  Returns (buildtraining, predict,
    computeelbo, theta): predict(X, L=1) the mean of softmax over L dropout draws, computeelbo(X, Y,
    draw=0) the log-likelihood sum under evaluation draw `draw` (the reference's priordkl is 0)."""
    buildtraining, ctx, theta = _construct(Din, Dh, Dout, f, s2, inf, True, keep, seed, loss, prior, max_batch, device)
    return buildtraining, (lambda X, L=1: ctx.predict(_values(X), draws=L)), \
        (lambda X, Y, draw=0: ctx.loglik(_values(X), _values(Y), draw=draw)), theta


class LearnedTheta(list):
    """The theta list LearnMLPracticalClassification returns, with the run it came from: train, logp
    and accuracy (training, testing)."""


def LearnMLPracticalClassification(Xtr, Ytr, Xte, Yte, bayesian=0, epochs=100, Dh=[500, 500, 500], infer=None, L=1,
                                   keep=0.5, loss="bernoulli", verbose=True):
    """mlp.py:332-388 without the matplotlib file: batches of 100 contiguous rows, the reference's
    printed lines, accuracies counted on the device (MAP: under theta; bayesian: the mean of L
    dropout passes).  Returns theta, the reference's list, which here also carries the run: theta.train
    (the train function; theta.train.ctx the engine context), theta.logp (the step values) and
    theta.accuracy = (training, testing)."""
    say = print if verbose else (lambda *a: None)
    infer = infer if infer is not None else AdaGrad(0.01)
    say("Building classifier graph.")
    Xtr, Ytr, Xte, Yte = (_values(a) for a in (Xtr, Ytr, Xte, Yte))
    Ntr, Din = Xtr.shape
    Dout = Ytr.shape[1]
    s2 = [1.0] * (2 * (len(Dh) + 1))
    if bayesian:
        buildtraining, predict, logjoint, theta = ConstructBayesianMLPClassifier(Din, Dh, Dout, "tanh", s2, infer,
                                                                                 keep=keep, loss=loss)
    else:
        buildtraining, predict, logjoint, theta = ConstructPMLPClassifier(Din, Dh, Dout, "tanh", s2, infer, loss=loss)
    say("Compiling MLP.")
    train = buildtraining(Xtr, Ytr)
    say("Performing inference.")
    rows, logp = np.arange(Ntr, dtype=np.int32), []
    for i in range(epochs):
        logp.extend(train.many(rows, 100).tolist())
        say("Epoch " + str(i) + ". logjoint = " + str(logp[-1]) + ".")
    say("Computing predictions under posterior.")
    draws = int(L) if bayesian else 0
    acc = (train.ctx.accuracy(Xtr, Ytr, draws) / Xtr.shape[0], train.ctx.accuracy(Xte, Yte, draws) / Xte.shape[0])
    say("training accuracy = " + str(acc[0]))
    say("testing accuracy = " + str(acc[1]))
    theta = LearnedTheta(theta)
    theta.train, theta.logp, theta.accuracy = train, logp, acc
    return theta


def GenerateGaussians(N, Ntr):
    """data.py:51-65: two classes of N correlated 2-d Gaussians at (1, 1) and (-1, -1), 1-hot labels,
    permuted with the global RNG; returns (Xtr, Ytr, Xte, Yte), the first Ntr rows for training."""
    cov = np.array([[1.0, -0.75], [-0.75, 1.0]])
    # the draw order of the reference: class 0's rows, class 1's rows, then the permutation
    X = np.concatenate([np.random.multivariate_normal(np.array(m), cov, size=N).astype(np.float32)
                        for m in ((1.0, 1.0), (-1.0, -1.0))])
    Y = np.zeros((2 * N, 2), np.float32)
    Y[:N, 0] = Y[N:, 1] = 1.0
    perm = np.random.permutation(2 * N)
    X, Y = X[perm], Y[perm]
    return X[:Ntr], Y[:Ntr], X[Ntr:], Y[Ntr:]


def _optimizer(name, eta):
    if name == "adagrad":
        return AdaGrad(0.1 if eta is None else eta)
    if name == "sga":
        return GradientAscent(1e-3 if eta is None else eta)
    if name == "adadelta":
        return AdaDelta(eta=1.0 if eta is None else eta)
    return Adam(1e-3 if eta is None else eta)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m vaeb_amd.mlp", description=__doc__.split("\n")[0])
    ap.add_argument("--synthetic", action="store_true", help="GenerateGaussians(1000, 1000) (the only data set here)")
    ap.add_argument("--bayesian", action="store_true", help="weight dropout (ConstructBayesianMLPClassifier)")
    ap.add_argument("--L", type=int, default=20, help="dropout passes averaged per prediction")
    ap.add_argument("--keep", type=float, default=0.5)
    ap.add_argument("--optimizer", choices=("adagrad", "sga", "adadelta", "adam"), default="adagrad")
    ap.add_argument("--eta", type=float, default=None)
    ap.add_argument("--hidden", default="500", help="comma-separated hidden sizes")
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--loss", choices=("bernoulli", "categorical"), default="bernoulli")
    a = ap.parse_args(argv)
    if not a.synthetic:
        ap.error("only --synthetic data is available (the reference's MLPractical loader is not part of it)")
    np.random.seed(SEED)   # mlp.py:424
    Xtr, Ytr, Xte, Yte = GenerateGaussians(1000, 1000)
    LearnMLPracticalClassification(Xtr, Ytr, Xte, Yte, bayesian=int(a.bayesian), epochs=a.epochs,
                                   Dh=[int(h) for h in a.hidden.split(",")], infer=_optimizer(a.optimizer, a.eta),
                                   L=a.L, keep=a.keep, loss=a.loss)


if __name__ == "__main__":
    main()
