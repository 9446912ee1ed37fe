#!/usr/bin/env python3
"""
Golden vectors of batched OGIVE (ogive_batch).  Runs ONLY in the build container (needs the reference sources): imports the real
reference ``ive.py`` with the shims of make_ogive_golden.py, unchanged, and calls its ``ogive()`` once per problem.

Writes ``ogive_batch.npz`` next to this file: B problems of one small shape, i.i.d. and mixture inputs.  X is not stored: problem
b's input is ``make_input(family[b], T, F, M, S, seed[b])`` (oracle.overiva_oracle.synth_iid / synth_mixture, complex64, run in
complex128), and ``X_sum`` (B,) -- the complex128 sum of every problem's X -- pins it.  Keys:
  ``T``, ``F``, ``M``, ``S`` (sources of the mixtures), ``family`` (B,), ``seed`` (B,), ``X_sum`` (B,), ``n_iter`` (epochs of the
  fixed-count runs), for every ``<update>_<model>``:
    ``W_<update>_<model>`` (B, F, M, 1): w after n_iter epochs with tol = 0, proj_back=False
    ``amp_<update>_<model>`` (B,): relative change of that w under a 1e-12 relative perturbation of X, / 1e-12
    ``floor_<update>_<model>`` (B,): distance of the reference's own complex64 run from its complex128 run (NaN: not finite)
  and the early-stop run (update="demix", model="laplace", ``stop_n_iter`` epochs at most, tol = ``stop_tol``):
    ``stop_epochs`` (B,): epochs the reference ran (the one whose max ||delta|| met the rule included),
    ``W_stop`` (B, F, M, 1), ``amp_stop`` (B,), ``stop_margin`` (B,): smallest |max ||delta|| - tol| / tol over its epochs.
The epoch count is read by counting the reference's per-epoch ``np.max`` (ive.py:243) through the module-global numpy proxy.

Usage:  python tests/golden/make_ogive_batch_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import make_input  # noqa: E402
from make_ogive_golden import import_reference  # noqa: E402

T, F, M, S = 96, 53, 5, 1
FAMILIES = ("iid", "mix", "iid", "mix", "mix")
SEEDS = tuple(7100 + 13 * b for b in range(len(FAMILIES)))
N_ITER = 12
UPDATES = ("demix", "mix", "switching")
MODELS = ("laplace", "gauss")
STOP_TOL, STOP_N_ITER = 5e-2, 600


class _Counting:
    """the module-global numpy of ive.py with a counter on ``max``: called once at ive.py:108 and once per epoch at :243"""

    def __init__(self, inner):
        self.inner = inner
        self.n_max = 0
        self.values = []

    def __getattr__(self, name):
        if name == "max":
            def counted(*a, **k):
                self.n_max += 1
                v = self.inner.max(*a, **k)
                self.values.append(v)
                return v
            return counted
        return getattr(self.inner, name)


def main():
    ive = import_reference()
    counter = _Counting(ive.np)
    ive.np = counter
    Xs = [make_input(fam, T, F, M, S, seed) for fam, seed in zip(FAMILIES, SEEDS)]
    out = {"T": T, "F": F, "M": M, "S": S, "family": np.array(FAMILIES, dtype="U8"), "seed": np.array(SEEDS),
           "X_sum": np.array([X.astype(np.complex128).sum() for X in Xs]), "n_iter": N_ITER, "stop_tol": STOP_TOL,
           "stop_n_iter": STOP_N_ITER}

    def run(X, **kw):
        with np.errstate(all="ignore"):
            return np.array(ive.ogive(X.copy(), proj_back=False, return_filters=True, **kw)[1])

    for update in UPDATES:
        for model in MODELS:
            W, amp, floor = [], [], []
            for b, X64 in enumerate(Xs):
                X = X64.astype(np.complex128)
                kw = dict(n_iter=N_ITER, tol=0.0, update=update, model=model)
                w = run(X, **kw)
                pert = 1.0 + 1e-12 * np.random.default_rng(SEEDS[b] + 2).standard_normal(X.shape)
                wp = run(X * pert, **kw)
                w64 = run(X64, **kw)
                W.append(w)
                amp.append(np.linalg.norm(wp - w) / np.linalg.norm(w) / 1e-12)
                floor.append(np.linalg.norm(w64 - w) / np.linalg.norm(w) if np.all(np.isfinite(w64)) else np.nan)
            key = f"{update}_{model}"
            out[f"W_{key}"] = np.stack(W)
            out[f"amp_{key}"] = np.array(amp)
            out[f"floor_{key}"] = np.array(floor)
            print(key, "amp", np.round(amp, 1), "floor", np.array(floor))
    W, amp, epochs, margin = [], [], [], []
    for b, X64 in enumerate(Xs):
        X = X64.astype(np.complex128)
        counter.n_max, counter.values = 0, []
        w = run(X, n_iter=STOP_N_ITER, tol=STOP_TOL)
        epochs.append(counter.n_max - 1)
        margin.append(np.min(np.abs(np.array(counter.values[1:]) - STOP_TOL)) / STOP_TOL)
        pert = 1.0 + 1e-12 * np.random.default_rng(SEEDS[b] + 3).standard_normal(X.shape)
        wp = run(X * pert, n_iter=STOP_N_ITER, tol=STOP_TOL)
        W.append(w)
        amp.append(np.linalg.norm(wp - w) / np.linalg.norm(w) / 1e-12)
    out["stop_epochs"] = np.array(epochs)
    out["W_stop"] = np.stack(W)
    out["amp_stop"] = np.array(amp)
    out["stop_margin"] = np.array(margin)
    print("early stop: epochs", epochs, "amp", np.round(amp, 1), "margin", margin)
    path = os.path.join(HERE, "ogive_batch.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
