#!/usr/bin/env python3
"""
Golden vectors of the batched path (overiva_batch).  Runs ONLY in the build container (needs the reference sources; see
make_golden.py, whose import shims it reuses unchanged).

Writes ``batch_<name>.npz`` next to this file: B problems of one small shape -- 65 bins (a ragged last batch of 64) x 160
frames -- mixing i.i.d. and mixture inputs.  The expected outputs come from calling the real reference once per problem.
X is not stored (it would be most of the bytes): problem b's input is ``make_input(family[b], T, F, M, K, seed[b])``, i.e.
oracle.overiva_oracle.synth_iid / synth_mixture, and ``X_sum`` (B,) -- the complex128 sum of every problem's X -- pins it.
Keys: ``T``, ``F``, ``M``, ``K``, ``family`` (B,) ("iid" | "mix"), ``seed`` (B,), ``W_<c64|c128>`` (B, F, M, K) after 20 laplace
iterations without projection back, ``Y_c128`` (n, T, F, K) of the first problem where T F K <= Y_MAX_ENTRIES (n = 1), else none
(n = 0), ``amp`` (B,) the reference's conditioning per problem (relative change of its complex128 W under a 1e-12 relative
perturbation of X, / 1e-12).  Each file stays well under 1 MB.

Usage:  python tests/golden/make_batch_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import import_reference, make_input  # noqa: E402

# (name, T, F, M, K, families of the B problems)
CASES = [
    ("a", 160, 65, 4, 2, ("iid", "mix", "iid", "mix")),
    ("b", 160, 65, 8, 4, ("iid", "mix", "iid", "iid", "mix")),
]
N_ITER = 20
Y_MAX_ENTRIES = 25000     # Y of one problem in complex128: at most 400 KB


def main():
    ref_overiva, _ = import_reference()
    for name, T, F, M, K, fams in CASES:
        Xs, out = [], {"T": T, "F": F, "M": M, "K": K, "family": np.array(fams, dtype="U8")}
        seeds = [5000 + 97 * ord(name) + b for b in range(len(fams))]
        res = {k: [] for k in ("W_c64", "W_c128", "Y_c64", "Y_c128")}
        amp = []
        for b, fam in enumerate(fams):
            seed = seeds[b]
            X64 = make_input(fam, T, F, M, K, seed)
            Xs.append(X64)
            for dt_name, X in (("c64", X64), ("c128", X64.astype(np.complex128))):
                Y, W = ref_overiva.overiva(X.copy(), n_src=K, n_iter=N_ITER, proj_back=False, return_filters=True)
                res[f"W_{dt_name}"].append(np.ascontiguousarray(W))
                res[f"Y_{dt_name}"].append(np.ascontiguousarray(Y))
            pert = 1.0 + 1e-12 * np.random.default_rng(seed + 2).standard_normal(X64.shape)
            W = res["W_c128"][-1]
            _, Wp = ref_overiva.overiva(X64.astype(np.complex128) * pert, n_src=K, n_iter=N_ITER, proj_back=False, return_filters=True)
            amp.append(np.linalg.norm(Wp - W) / np.linalg.norm(W) / 1e-12)
        out["seed"] = np.array(seeds)
        out["X_sum"] = np.array([X.astype(np.complex128).sum() for X in Xs])
        out["W_c64"] = np.stack(res["W_c64"])
        out["W_c128"] = np.stack(res["W_c128"])
        nY = 1 if T * F * K <= Y_MAX_ENTRIES else 0
        out["Y_c128"] = np.array(res["Y_c128"][:nY], dtype=np.complex128).reshape((nY, T, F, K))
        out["amp"] = np.array(amp)
        path = os.path.join(HERE, f"batch_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"{path}: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
