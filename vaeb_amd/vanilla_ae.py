"""Drop-in for the reference's vanilla-ae/ae.py drivers (:129-251): LearnFreyFace, LearnMNIST and
main, the squared-error autoencoder baseline behind reconstruction_res/AE_MSE.res.

    python -m vaeb_amd.vanilla_ae [--synthetic] [--out DIR] [--epochs N] [--dz 2,10,20]
                                  [--hidden H] [--ntr N] [--corruption KIND [--noise L0,L1,...]]
                                  [--optimizer adagrad|sga|adadelta|adam] [--eta ETA]

main() seeds the global numpy RNG with 15485863 (:219), then for Dz in 2, 10, 20 trains the Frey
model (hidden 200, 1500 rows, 100 epochs at Dz = 2, otherwise 550) and the MNIST model (hidden 500,
50000 rows, 1000 epochs), each epoch a fresh permutation in batches of 100 with the last partial
batch kept, saves the eight AE_{continuous,discrete}_{Dz}_{orig,recon}_{t}.jpg pairs and appends the
test set's MSE to AE_MSE.res.  All compute runs in libvaeb_hip.so (ae.ConstructVanillaAE); an epoch
is one vaeb_ae_train_many call and the test MSE is reduced on the device (vaeb_ae_sq_error).  The
commented-out matplotlib learning curves of the reference are not written.

--corruption mask|saltpepper|gauss trains every model as a denoising autoencoder (the encoder reads
the corrupted rows, the error is taken on the clean ones); --noise L0,L1,... is a schedule of stages
spread over each model's epochs by ae.noise_schedule (default: one stage at 0.3).  AE_MSE.res stays the
clean test-set MSE.  Without --corruption nothing changes.

--optimizer picks the update rule of every model (infalg.AdaGrad | GradientAscent with momentum 0.9 |
AdaDelta | Adam; default adagrad) and --eta its step size (defaults 0.01 | 1e-3 | 1.0 | 1e-3).  Without
either the run is the reference's AdaGrad(0.01).

Data comes through cli.load_dataset (freyfaces.pkl / mnist.pkl.gz in the working directory, or the
synthetic stand-ins with --synthetic).  MNIST follows data.py:11-21: the training rows are the first
Ntr of train + valid, the test rows the test split.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import numpy.random as rnd

from . import ae
from .cli import get_arg, get_flag, load_dataset
from .image import save_image
from .infalg import AdaDelta, AdaGrad, Adam, GradientAscent

log_file = 'AE_MSE.res'
latent_sizes = [2, 10, 20]                          # ae.py:226
FREY = dict(hidden=200, Ntr=1500)                   # ae.py:129, 138
MNIST = dict(hidden=500, Ntr=50000, epochs=1000)    # ae.py:183, 241


def frey_epochs(Dz):
    return 550 if Dz > 2 else 100                   # ae.py:227


def load_frey(Ntr=1500, synthetic=False):
    """data.LoadFreyFace (data.py:44-47): the first Ntr faces train, the rest test."""
    a, b = load_dataset(True, synthetic)
    X = np.vstack((a, b))
    return X[:Ntr], X[Ntr:]


def load_mnist(Ntr=50000, synthetic=False):
    """data.LoadMNIST (data.py:11-21): the first Ntr of train + valid train, the test split tests."""
    (xtr, _), (xva, _), (xte, _) = load_dataset(False, synthetic, splits=3)
    return np.vstack((xtr, xva))[:Ntr], xte


DEFAULT_NOISE = [0.3]


def corruption_args(kind, noise):
    """The checked (kind, stage list) of --corruption / --noise, or None without --corruption."""
    if kind is None:
        if noise is not None:
            raise ValueError("--noise needs --corruption mask|saltpepper|gauss")
        return None
    if kind not in ae.CORRUPTIONS:
        raise ValueError(f"--corruption {kind!r} not supported (mask | saltpepper | gauss)")
    return kind, list(noise) if noise is not None else list(DEFAULT_NOISE)


OPTIMIZERS = {"adagrad": lambda eta: AdaGrad(0.01 if eta is None else eta),
              "sga": lambda eta: GradientAscent(1e-3 if eta is None else eta, momentum=0.9),
              "adadelta": lambda eta: AdaDelta(eta=1.0 if eta is None else eta),
              "adam": lambda eta: Adam(1e-3 if eta is None else eta)}


def optimizer_args(name, eta):
    """The checked inference algorithm of --optimizer / --eta (None, None: the reference's AdaGrad(0.01))."""
    name = "adagrad" if name is None else name
    if name not in OPTIMIZERS:
        raise ValueError(f"--optimizer {name!r} not supported (adagrad | sga | adadelta | adam)")
    return OPTIMIZERS[name](eta)


def _learn(Xtr, Xte, epochs, Dz, hidden, batch_size=100, corruption=None, inf=None):
    """The shared body of LearnFreyFace / LearnMNIST (ae.py:136-166, 181-211).  corruption: (kind,
    stage list) of a denoising run, the stages spread over the epochs.  inf: the update rule (None:
    AdaGrad(0.01), ae.py:141)."""
    Xtr, Xte = np.asarray(Xtr, np.float32), np.asarray(Xte, np.float32)
    Ntr = Xtr.shape[0]
    if Xte.shape[0] < 8:
        raise ValueError(f"{Xte.shape[0]} test rows left after {Ntr} training rows; the report needs 8 (lower --ntr)")
    levels = ae.noise_schedule(corruption[1], epochs) if corruption else None
    train, reconstruct, encode, decode, theta = ae.ConstructVanillaAE(
        Xtr, Denc=[hidden], Dz=Dz, Ddec=[hidden], inf=inf if inf is not None else AdaGrad(0.01),
        corruption=(corruption[0], levels[0] if levels else 0.0) if corruption else None)
    print('Training the autoencoder.')
    mse = []
    for i in range(epochs):
        if levels:
            train.set_noise(levels[i])
        idx = rnd.permutation(np.arange(Ntr)).astype(np.int32)
        mse.extend(train.ctx.train_many(idx, batch_size).tolist())
        print('Epoch ' + str(i) + '. mse = ' + str(mse[-1]))
    rmsetr, rmsete = ae.rmse(Xtr, reconstruct(Xtr)), ae.rmse(Xte, reconstruct(Xte))
    print('training rmse = ' + str(rmsetr))
    print('testing rmse = ' + str(rmsete))

    def recon(X):
        return reconstruct(X)

    recon.train, recon.mse_curve = train, mse
    return recon, encode, decode, Xtr, Xte


def LearnFreyFace(epochs=100, Dz=20, Ntr=1500, hidden=FREY["hidden"], data=None, synthetic=False, corruption=None,
                  inf=None):
    """ae.py:129-166.  Returns (reconstruct, encode, decode, Xtr, Xte); reconstruct.train is the
    training function (train.mse(X): the device-side MSE), reconstruct.mse_curve the per-step se / M."""
    Xtr, Xte = data if data is not None else load_frey(Ntr, synthetic)
    return _learn(Xtr, Xte, epochs, Dz, hidden, corruption=corruption, inf=inf)


def LearnMNIST(epochs=25, Dz=20, Ntr=50000, hidden=MNIST["hidden"], data=None, synthetic=False, corruption=None,
                  inf=None):
    """ae.py:174-211; returns as LearnFreyFace."""
    Xtr, Xte = data if data is not None else load_mnist(Ntr, synthetic)
    return _learn(Xtr, Xte, epochs, Dz, hidden, corruption=corruption, inf=inf)


def _report(data_type, Dz, reconstruct, Xte, out_dir):
    """ae.py:231-238 / 244-251: eight jpg pairs and one AE_MSE.res row; the MSE on the device."""
    for t in range(8):
        save_image(Xte[t:t + 1], os.path.join(out_dir, 'AE_{0}_{1}_orig_{2}.jpg'.format(data_type, Dz, t)))
        save_image(reconstruct(Xte[t:t + 1]), os.path.join(out_dir, 'AE_{0}_{1}_recon_{2}.jpg'.format(data_type, Dz, t)))
    mseVal = reconstruct.train.mse(Xte)
    with open(os.path.join(out_dir, log_file), 'a') as f:
        f.write('{0},{1},{2}\n'.format(data_type, Dz, mseVal))
    reconstruct.train.ctx.close()
    return mseVal


def main(argv=None, data=None):
    """ae.py:216-251.  data: {"continuous": (Xtr, Xte), "discrete": (Xtr, Xte)} overrides the files
    (tests).  --epochs overrides every model's epoch count, --hidden both hidden widths, --ntr both
    training-row counts, --corruption / --noise make the run a denoising one, --optimizer / --eta pick the
    update rule (all checked before any device work).  Returns {(data_type, Dz): mse}."""
    args = list(sys.argv[1:] if argv is None else argv)
    out_dir = get_arg('out', args, 'reconstruction_res', str)
    epochs = get_arg('epochs', args, None, int)
    dz_list = get_arg('dz', args, latent_sizes, lambda s: [int(v) for v in s.split(',')])
    hidden = get_arg('hidden', args, None, int)
    ntr = get_arg('ntr', args, None, int)
    synthetic = get_flag('synthetic', args)
    corruption = corruption_args(get_arg('corruption', args, None, str),
                                 get_arg('noise', args, None, lambda s: [float(v) for v in s.split(',')]))
    inf = optimizer_args(get_arg('optimizer', args, None, str), get_arg('eta', args, None, float))
    if args:
        print('Have unused args: {0}'.format(args))
    data = data or {}

    rnd.seed(15485863)                               # a large-ish prime (ae.py:219)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, log_file), 'w') as f:
        f.write('data_type,latent_size,MSE\n')
    res = {}
    for Dz in dz_list:
        reconstruct, _, _, _, Xte = LearnFreyFace(
            epochs=epochs if epochs is not None else frey_epochs(Dz), Dz=Dz, Ntr=ntr or FREY["Ntr"],
            hidden=hidden or FREY["hidden"], data=data.get('continuous'), synthetic=synthetic, corruption=corruption,
            inf=inf)
        res[('continuous', Dz)] = _report('continuous', Dz, reconstruct, Xte, out_dir)
        reconstruct, _, _, _, Xte = LearnMNIST(
            epochs=epochs if epochs is not None else MNIST["epochs"], Dz=Dz, Ntr=ntr or MNIST["Ntr"],
            hidden=hidden or MNIST["hidden"], data=data.get('discrete'), synthetic=synthetic, corruption=corruption,
            inf=inf)
        res[('discrete', Dz)] = _report('discrete', Dz, reconstruct, Xte, out_dir)
    return res


if __name__ == '__main__':
    main()
