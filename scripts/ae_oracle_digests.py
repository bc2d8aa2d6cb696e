"""SHA-256 digests of everything the layer-stack engine's NumPy oracles return (host only).

One line per case and dtype (float64, float32) over the value(s), the returned intermediates, the
gradient per block and theta' / acc' of train_step, for every case of the existing tables
(tests/ae_grad_cases.py, tests/vanilla_ae_cases.py, tests/vae_prior_cases.py both forms, the
denoise, stack, IW and IW-train lists of their host tests, one IW denoising step), and one line per
listed wrong gradient.  It is written against the signatures of the feature modules
(tests/*_oracle.py, oracle/ae_oracle.py), so the same file runs on two commits; two outputs made on one
machine with one thread setting, one run after the other, are equal line for line when the arithmetic
of the oracles is unchanged operation by operation.  BLAS kernels differ between hosts: the outputs
are a record (profiles/ae_oracle/), never an assertion.

    python scripts/ae_oracle_digests.py > digests.txt
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import ae_oracle as A                       # noqa: E402
from tests import ae_grad_cases as G                    # noqa: E402
from tests import denoise_oracle as D                   # noqa: E402
from tests import test_ae_grads_host as GH              # noqa: E402
from tests import test_denoise_host as DH               # noqa: E402
from tests import test_vae_stack_host as SH             # noqa: E402
from tests import test_vanilla_ae_host as NH            # noqa: E402
from tests import test_vae_stack_iw_host as WH          # noqa: E402
from tests import test_vae_stack_iwtrain_host as TH     # noqa: E402
from tests import vae_prior_cases as PC                 # noqa: E402
from tests import vae_prior_oracle as PO                # noqa: E402
from tests import vae_stack_iw_oracle as W              # noqa: E402
from tests import vae_stack_iwtrain_oracle as T         # noqa: E402
from tests import vae_stack_oracle as V                 # noqa: E402
from tests import vanilla_ae_cases as NC                # noqa: E402
from tests import vanilla_ae_oracle as N                # noqa: E402

DTYPES = (np.float64, np.float32)
POINT_KEYS = ("loglik", "logjoint", "H", "Z", "G", "Xpr")
VANILLA_KEYS = ("value", "se", "loglik", "logjoint", "H", "Z", "Zpre", "G", "Xpr")
GAUSS_KEYS = ("loglik", "negkl", "elbo", "f", "mu", "lv", "z", "Xpr", "H", "G")
IW_KEYS = ("iw", "rows", "wn", "lw", "f", "mu", "lv", "z", "Xpr", "H", "G")
DENOISE_KEYS = ("data", "negkl", "value", "f", "H", "Z", "G", "Xpr")
PRIOR_KEYS = ("value", "f", "loglik", "latent", "rows", "lw", "lat", "wn", "t", "r", "mu", "lv", "z", "Xpr", "H", "G")


def feed(h, x):
    if isinstance(x, (list, tuple)):
        h.update(b"[%d" % len(x))
        for y in x:
            feed(h, y)
    elif isinstance(x, dict):
        for k in x:
            h.update(k.encode())
            feed(h, x[k])
    else:
        a = np.ascontiguousarray(x)
        h.update(f"{a.dtype.str}{a.shape}".encode())
        h.update(a.tobytes())


def line(label, *parts):
    h = hashlib.sha256()
    for p in parts:
        feed(h, p)
    print(f"{h.hexdigest()}  {label}", flush=True)


def picked(out, keys):
    """The listed results of an oracle call that it returned, then its gradients per block."""
    return [{k: out[k] for k in keys if k in out}, out.get("grads", []), out.get("data_grads", [])]


def cast(arrays, dt):
    return [np.asarray(a).astype(dt) for a in arrays]


def acc0(params, dt):
    return [np.full(p.shape, 1e-4, dt) for p in params]


def step_line(label, keys, result):
    v, new_p, new_a, aux = result
    line(label, np.float64(v), new_p, new_a, *picked(aux, keys))


def tag(dt):
    return np.dtype(dt).name


def grad_cases():
    for (name, latent, scaled), cid in zip(G.CASES, G.CASE_IDS):
        st = G.case(name, latent, scaled)
        for dt in DTYPES:
            p, a, X = cast(st.params, dt), acc0(st.params, dt), st.Xtr.astype(dt)
            if latent == "gauss":
                step_line(f"grads {cid} {tag(dt)}", GAUSS_KEYS, V.train_step(p, a, X, st.idx, st.eps.astype(dt), st.cfg))
            else:
                step_line(f"grads {cid} {tag(dt)}", POINT_KEYS, A.train_step(p, a, X, st.idx, st.cfg))
    for kind, name, latent, scaled in GH.MUTANT_CASES:
        st = G.case(name, latent, scaled)
        g = GH.mutant_grads(st, kind)
        line(f"grads-wrong {kind} {name}-{latent}-{'x30' if scaled else 'theta0'}", [g[n] for n, _ in st.shapes])


def vanilla_cases():
    for (name, latent, otype, scaled), cid in zip(NC.CASES, NC.CASE_IDS):
        st = NC.case(name, latent, otype, scaled)
        for dt in DTYPES:
            p, X = cast(st.params, dt), st.Xtr.astype(dt)
            step_line(f"vanilla {cid} {tag(dt)}", VANILLA_KEYS, N.train_step(p, acc0(p, dt), X, st.idx, st.cfg, latent))
            for kind in N.WRONG:
                if not NH.applies(kind, latent, otype):
                    continue
                out = N.forward_backward(p, X[st.idx], st.cfg, latent, wrong=kind)
                line(f"vanilla-wrong {kind} {cid} {tag(dt)}", out["grads"])


def prior_cases():
    for (name, form), sid in zip(PC.STEPS, PC.STEP_IDS):
        st, c = PC.step(name, form), PC.CASE[name]
        for dt in DTYPES:
            p, X, eps = cast(st.params, dt), st.Xtr.astype(dt), st.eps.astype(dt)
            step_line(f"prior {sid} {tag(dt)}", PRIOR_KEYS,
                      PO.train_step(p, acc0(p, dt), X, st.idx, eps, st.cfg, c.mean1, c.width, form))
            for kind in PO.WRONG:
                if kind == "half_not_half_wn" and form != "iw":
                    continue
                with np.errstate(invalid="ignore", over="ignore"):
                    out = PO.forward_backward(p, X[st.idx], eps, st.cfg, c.mean1, c.width, form, wrong=kind)
                line(f"prior-wrong {kind} {sid} {tag(dt)}", out["grads"])
    # a corrupting two-mode step: the encoder fed other rows than the output scores
    st, c = PC.step("dz17_m5_cont_a2", "iw"), PC.CASE["dz17_m5_cont_a2"]
    for dt in DTYPES:
        p, X = cast(st.params, dt), st.Xtr.astype(dt)
        step_line(f"prior dz17_m5_cont_a2-iw-xenc {tag(dt)}", PRIOR_KEYS,
                  PO.train_step(p, acc0(p, dt), X, st.idx, st.eps.astype(dt), st.cfg, c.mean1, c.width, "iw",
                                Xenc=X[st.idx][::-1].copy()))


def denoise_cases():
    for name in DH.DENOISE_IDS + ["philox"]:
        c = DH.philox_case() if name == "philox" else DH.denoise_case(name)
        for dt in DTYPES:
            X = c.X[c.idx].astype(dt)
            xt = D.corrupt(X, c.kind, c.level, c.draw.astype(dt))
            p, a = cast(c.params, dt), cast(c.acc, dt)
            if c.K >= 2:                                   # the IW denoising step
                step_line(f"denoise {name} {tag(dt)}", IW_KEYS, D.iw_train_step(p, a, xt, X, c.eps.astype(dt), c.cfg))
                continue
            eps = None if c.eps is None else c.eps.astype(dt)
            step_line(f"denoise {name} {tag(dt)}", DENOISE_KEYS, D.train_step(p, a, xt, X, c.cfg, c.latent, eps))
            for kind in D.WRONG:
                out = D.forward_backward(p, xt, X, c.cfg, c.latent, eps, wrong=kind)
                line(f"denoise-wrong {kind} {name} {tag(dt)}", out["grads"])


def stack_cases():
    runs = [(name, SH.step_setup(kw, B, scale)) for name, kw, B, scale in SH.STEP_CASES]
    cfg, X, params, acc, idx = SH.philox_setup()
    runs.append(("philox", (cfg, X, params, acc, idx, V.train_eps(SH.SEED, idx, cfg.Dz, SH.STEP))))
    for name, (cfg, X, params, acc, idx, eps) in runs:
        for dt in DTYPES:
            step_line(f"stack {name} {tag(dt)}", GAUSS_KEYS,
                      V.train_step(cast(params, dt), cast(acc, dt), X.astype(dt), idx, np.asarray(eps, dt), cfg))


def iw_cases():
    for name in WH.IW_IDS:
        cfg, X, params, eps = WH.iw_setup(name)
        for dt in DTYPES:
            out = W.log_weights(cast(params, dt), X.astype(dt), eps.astype(dt), cfg)
            line(f"iw {name} {tag(dt)}", {k: out[k] for k in ("lw", "ll", "lat", "mu", "lv")}, W.iw_from_lw(out["lw"]),
                 [picked(o, GAUSS_KEYS) for o in out["outs"]])


def iwtrain_cases():
    for (name, scaled), cid in zip(TH.ALL_CASES, TH.ALL_IDS):
        st, _ = TH.case(name, scaled)
        for dt in DTYPES:
            p, X, eps = cast(st.params, dt), st.Xtr.astype(dt), st.eps.astype(dt)
            step_line(f"iwtrain {cid} {tag(dt)}", IW_KEYS, T.train_step(p, acc0(p, dt), X, st.idx, eps, st.cfg))
            if not scaled:
                continue
            M = len(st.idx)
            for kind in T.WRONG:
                out = T.forward_backward(p, X[st.idx], eps, st.cfg, wrong=kind)
                line(f"iwtrain-wrong {kind} {cid} {tag(dt)}", out["grads"])
            out = T.forward_backward(p, X[st.idx], eps, st.cfg, Y=X[:M])
            line(f"iwtrain-wrong y_by_position {cid} {tag(dt)}", out["grads"])
            line(f"iwtrain marginal_rows {cid} {tag(dt)}", T.marginal_rows(p, X[st.idx], eps, st.cfg))
    cfg, X, params, acc, idx = TH.philox_setup()
    eps = T.train_eps(TH.SEED, idx, cfg.Dz, TH.STEP, TH.PHILOX_K)
    for dt in DTYPES:
        step_line(f"iwtrain philox {tag(dt)}", IW_KEYS,
                  T.train_step(cast(params, dt), cast(acc, dt), X.astype(dt), idx, eps.astype(dt), cfg))


if __name__ == "__main__":
    for part in (grad_cases, vanilla_cases, prior_cases, denoise_cases, stack_cases, iw_cases, iwtrain_cases):
        part()
