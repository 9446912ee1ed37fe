#!/usr/bin/env python3
"""
Golden vectors of the wide path (17..32 channels).  Runs ONLY in the build container (needs the reference sources; see
make_golden.py, whose import shims it reuses unchanged).

Writes ``wide_<name>_<family>.npz`` next to this file -- NOT ``overiva_*.npz``: conftest.golden_files() feeds that pattern to
the tests of the narrow path.  Keys as make_golden.py: the input ``X`` (complex64), ``W_<c64|c128>_<model>_<n_iter>`` (the
reference's own complex64 and complex128 results), ``Y_c128_<model>_20``, ``amp_<model>_<n_iter>`` (the reference's
conditioning: relative change of its complex128 W under a 1e-12 relative perturbation of X, / 1e-12), ``nonfinite``; plus the
projection back and callback payloads (``Ypb_c128_laplace_12``, ``cb0_c128_laplace``, ``cb10_c128_laplace``), a warm start
(``W0``, ``W_w0_c128_laplace_3``), ``W_eig_c128_laplace_3`` and ``Ypca_c128_laplace_5``.  Arrays of T x F x K entries (Y and
the payloads) only where K T F <= 20000, so that every fixture stays below 1 MB.

Usage:  python tests/golden/make_wide_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import import_reference, make_input  # noqa: E402

# (name, T, F, M, K, family)
CASES = [
    ("a", 160, 9, 17, 2, "iid"),
    ("b", 200, 7, 24, 3, "mix"),
    ("c", 256, 6, 32, 2, "iid"),
    ("d", 256, 3, 32, 32, "mix"),
    ("e", 192, 11, 31, 1, "iid"),
]
N_ITERS = (1, 5, 20)


def main():
    ref_overiva, ref_pca = import_reference()
    total = 0
    for name, T, F, M, K, family in CASES:
        seed = 3000 + ord(name)
        X64 = make_input(family, T, F, M, K, seed)
        X128 = X64.astype(np.complex128)
        out = {"X": X64, "T": T, "F": F, "M": M, "K": K}
        nonfinite = []
        pert = 1.0 + 1e-12 * np.random.default_rng(seed + 2).standard_normal(X64.shape)
        for dt_name, X in (("c64", X64), ("c128", X128)):
            for model in ("laplace", "gauss"):
                for n_iter in N_ITERS:
                    Y, W = ref_overiva.overiva(X.copy(), n_src=K, n_iter=n_iter, proj_back=False, model=model,
                                               return_filters=True)
                    key = f"{dt_name}_{model}_{n_iter}"
                    if not (np.all(np.isfinite(W)) and np.all(np.isfinite(Y))):
                        nonfinite.append(key)
                        continue
                    out[f"W_{key}"] = np.ascontiguousarray(W)
                    if dt_name == "c128":
                        _, Wp = ref_overiva.overiva(X * pert, n_src=K, n_iter=n_iter, proj_back=False, model=model,
                                                    return_filters=True)
                        out[f"amp_{model}_{n_iter}"] = np.float64(np.linalg.norm(Wp - W) / np.linalg.norm(W) / 1e-12)
                        if n_iter == 20 and K * T * F <= 20000:       # (kept small: the fixtures stay well under 1 MB)
                            out[f"Y_{key}"] = Y
        if K * T * F <= 20000:
            got = []
            out["Ypb_c128_laplace_12"] = ref_overiva.overiva(X128.copy(), n_src=K, n_iter=12, proj_back=True, model="laplace",
                                                             callback=lambda y: got.append(np.array(y)))
            out["cb0_c128_laplace"], out["cb10_c128_laplace"] = got
        rng = np.random.default_rng(seed + 1)
        W0 = np.eye(M, K)[None] + 0.1 * (rng.standard_normal((F, M, K)) + 1j * rng.standard_normal((F, M, K)))
        out["W0"] = W0
        out["W_w0_c128_laplace_3"] = np.ascontiguousarray(
            ref_overiva.overiva(X128.copy(), n_src=K, n_iter=3, proj_back=False, W0=W0, return_filters=True)[1])
        out["W_eig_c128_laplace_3"] = np.ascontiguousarray(
            ref_overiva.overiva(X128.copy(), n_src=K, n_iter=3, proj_back=False, init_eig=True, return_filters=True)[1])
        if K < M and K * T * F <= 20000:
            out["Ypca_c128_laplace_5"] = ref_pca.auxiva_pca(X128.copy(), n_src=K, n_iter=5, proj_back=True, model="laplace")
        out["nonfinite"] = np.array(nonfinite, dtype="U32")
        path = os.path.join(HERE, f"wide_{name}_{family}.npz")
        np.savez_compressed(path, **out)
        sz = os.path.getsize(path)
        total += sz
        print(f"{path}: {len(out)} arrays, {sz / 1024:.0f} KiB")
    print(f"total {total / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
