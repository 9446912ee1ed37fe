#!/usr/bin/env python3
"""
Golden vectors of the ragged batched path (overiva_batch_ragged).  Runs ONLY in the build container (needs the reference sources;
see make_golden.py, whose import shims it reuses unchanged).

Writes ``ragged.npz`` next to this file: P problems at 65 bins (a ragged last batch of 64) and different frame counts -- one
above 256, i.e. two covariance splits --, in four groups (M / K 4 / 2 and 8 / 4, each with the laplace and the gauss model), every
group a ragged batch of two lengths mixing i.i.d. and mixture inputs.  The expected outputs come from calling the real reference
once per problem.  X is not stored: problem p's input is ``make_input(family[p], T[p], F, M[p], K[p], seed[p])``, i.e.
oracle.overiva_oracle.synth_iid / synth_mixture, and ``X_sum`` (P,) -- the complex128 sum of its X -- pins it.
Keys: ``F``, ``n_iter``; per problem (P,): ``T``, ``M``, ``K``, ``model``, ``group`` (problems of one group form one ragged batch),
``family`` ("iid" | "mix"), ``seed``, ``X_sum``, ``amp`` (the reference's conditioning: relative change of its complex128 W under a
1e-12 relative perturbation of X, / 1e-12); ``W_c64``, ``W_c128`` (P, F, 8, 4): W after n_iter iterations without projection
back, zero-padded past (M, K); ``Y_c128`` (T, F, K) of problem ``Y_index`` only.  The file stays well under 1 MB.

Usage:  python tests/golden/make_ragged_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import import_reference, make_input  # noqa: E402

F = 65
N_ITER = 20
# (M, K, model, [(T, family), ...]): one ragged batch per group
GROUPS = [
    (4, 2, "laplace", [(100, "iid"), (300, "mix")]),
    (4, 2, "gauss", [(147, "mix"), (168, "iid")]),
    (8, 4, "laplace", [(160, "iid"), (257, "mix")]),
    (8, 4, "gauss", [(300, "mix"), (200, "iid")]),
]
Y_INDEX = 0          # Y of the first problem (100 x 65 x 2 complex128: about 200 KB)


def main():
    ref_overiva, _ = import_reference()
    keys = ("T", "M", "K", "model", "group", "family", "seed", "X_sum", "amp")
    out = {k: [] for k in keys}
    W = {"c64": [], "c128": []}
    Y = None
    p = 0
    for g, (M, K, model, probs) in enumerate(GROUPS):
        for T, fam in probs:
            seed = 7000 + 131 * g + T
            X64 = make_input(fam, T, F, M, K, seed)
            for dt_name, X in (("c64", X64), ("c128", X64.astype(np.complex128))):
                Yr, Wr = ref_overiva.overiva(X.copy(), n_src=K, n_iter=N_ITER, proj_back=False, model=model, return_filters=True)
                Wp = np.zeros((F, 8, 4), np.complex128)
                Wp[:, :M, :K] = Wr
                W[dt_name].append(Wp)
                if dt_name == "c128" and p == Y_INDEX:
                    Y = np.ascontiguousarray(Yr, dtype=np.complex128)
            pert = 1.0 + 1e-12 * np.random.default_rng(seed + 2).standard_normal(X64.shape)
            _, Wq = ref_overiva.overiva(X64.astype(np.complex128) * pert, n_src=K, n_iter=N_ITER, proj_back=False, model=model,
                                        return_filters=True)
            W0 = W["c128"][-1][:, :M, :K]
            for k, v in zip(keys, (T, M, K, model, g, fam, seed, X64.astype(np.complex128).sum(),
                                   np.linalg.norm(Wq - W0) / np.linalg.norm(W0) / 1e-12)):
                out[k].append(v)
            p += 1
    res = {"F": F, "n_iter": N_ITER, "Y_index": Y_INDEX}
    for k in keys:
        res[k] = np.array(out[k], dtype="U8" if k in ("model", "family") else None)
    res["W_c64"] = np.stack(W["c64"]).astype(np.complex64)        # (the reference's complex64 run: complex64 W)
    res["W_c128"] = np.stack(W["c128"])
    res["Y_c128"] = Y
    path = os.path.join(HERE, "ragged.npz")
    np.savez_compressed(path, **res)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KiB; amp {np.round(res['amp'], 1)}")


if __name__ == "__main__":
    main()
