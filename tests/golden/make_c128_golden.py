#!/usr/bin/env python3
"""
Golden vectors of the complex128 data path (``overiva_batch(..., data="complex128")``).  Runs ONLY in the build container (needs the
reference checkout), through ``make_golden.import_reference()`` and its two shims.

Inputs are full-precision complex128, NOT representable in complex64, seed 11 (``make_input``):

* ``iid``: ``rng.standard_normal((T, F, M)) + 1j * rng.standard_normal((T, F, M))``
* ``mix``: the statements of ``oracle.synth_mixture`` with S = M and without its final ``astype(complex64)``

A (T, F, M) complex128 array of random mantissas does not compress, and the larger cases alone would pass the size limit of a
committed file several times over, so a fixture holds no X and no whole Y: the tests regenerate X with ``make_input`` (``X_sum``
and ``X_abs`` pin the regenerated array) and compare Y on ``rows``, four frames spread over the room.  Stored per case
(``c128_<T>x<F>x<M>x<K>_<family>.npz``), from the real reference in complex128:

* ``W_<model>_<n>``, n = 1, 5, 20; ``Yrows_<model>_20`` (no projection back), ``Ypbrows_<model>_12`` (with it)
* ``amp_<model>_<n>``, n = 1, 5, 12, 20, as ``make_golden.py`` defines it (the reference's own response to a relative
  perturbation of X, divided by the perturbation's size; for 12 measured on Y), the larger of the figures for a 1e-12 and a
  1e-13 perturbation.  A well-conditioned row responds in proportion and gives the same figure twice (gauss 20 on 257x20x8x4
  iid: 2.69 and 2.69).  A row on which the reference is chaotic moves by a fixed amount whatever the size of the perturbation
  (gauss 20 on 257x20x8x4 mix: 2.9e-10 and 3.6e-10 of W, i.e. 287 and 3580), so one probe at 1e-12 under-reports it; an
  independent float64 implementation (``oracle.overiva_staged``) stands 1.2e-9 from the reference on that row and 1e-13 .. 3e-15
  on its neighbours.
* ``W_rounded_<model>_20``: the reference run on ``X.astype(complex64).astype(complex128)``: what a path that rounds X on upload
  is expected to land near

Usage:  python tests/golden/make_c128_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 11
MODELS = ("laplace", "gauss")
N_ITERS = (1, 5, 20)
PERTURBATIONS = (1e-12, 1e-13)
# (T, F, M, K, families): all eight channel counts, a second covariance split, 16-bin groups and 64-bin parts both exactly full
# and with a one-bin tail, a 7-bin room and a determined case
CASES = [
    (70, 17, 2, 1, ("iid", "mix")),
    (100, 65, 3, 2, ("iid", "mix")),
    (257, 20, 8, 4, ("iid", "mix")),
    (300, 33, 5, 5, ("iid", "mix")),
    (64, 130, 4, 2, ("iid", "mix")),
    (70, 7, 1, 1, ("iid",)),
    (129, 16, 7, 3, ("iid",)),
    (96, 40, 6, 6, ("iid",)),
]


def make_input(family, T, F, M):
    rng = np.random.default_rng(SEED)
    if family == "iid":
        return rng.standard_normal((T, F, M)) + 1j * rng.standard_normal((T, F, M))
    S = M
    act = rng.gamma(0.5, 1.0, (T, 1, S))
    src = act * (rng.standard_normal((T, F, S)) + 1j * rng.standard_normal((T, F, S)))
    A = rng.standard_normal((F, M, S)) + 1j * rng.standard_normal((F, M, S))
    X = np.einsum("fmk,tfk->tfm", A, src)
    return X + 0.1 * (rng.standard_normal((T, F, M)) + 1j * rng.standard_normal((T, F, M)))


def frame_rows(T):
    return np.unique(np.linspace(0, T - 1, 4).astype(int))


def case_path(T, F, M, K, family):
    return os.path.join(HERE, f"c128_{T}x{F}x{M}x{K}_{family}.npz")


def main():
    sys.path.insert(0, HERE)
    from make_golden import import_reference

    ref, _ = import_reference()
    total = 0
    for T, F, M, K, families in CASES:
        for family in families:
            X = make_input(family, T, F, M)
            assert X.dtype == np.complex128 and not np.array_equal(X, X.astype(np.complex64))
            rows = frame_rows(T)
            out = {"T": T, "F": F, "M": M, "K": K, "family": family, "rows": rows, "X_sum": X.sum(), "X_abs": np.abs(X).sum()}
            noise = np.random.default_rng(SEED + 2).standard_normal(X.shape)

            def amp(run, base):
                """the reference's response to a relative perturbation of X over its size, the larger of two sizes"""
                return np.float64(max(np.linalg.norm(run(X * (1.0 + size * noise)) - base) / np.linalg.norm(base) / size
                                      for size in PERTURBATIONS))

            Xr = X.astype(np.complex64).astype(np.complex128)
            for model in MODELS:
                for n in N_ITERS:
                    Y, W = ref.overiva(X.copy(), n_src=K, n_iter=n, proj_back=False, model=model, return_filters=True)
                    assert W.dtype == np.complex128 and Y.dtype == np.complex128
                    out[f"W_{model}_{n}"] = np.ascontiguousarray(W)
                    out[f"amp_{model}_{n}"] = amp(lambda Xp: ref.overiva(Xp, n_src=K, n_iter=n, proj_back=False, model=model,
                                                                         return_filters=True)[1], W)
                    if n == 20:
                        out[f"Yrows_{model}_20"] = np.ascontiguousarray(Y[rows])
                        _, Wq = ref.overiva(Xr.copy(), n_src=K, n_iter=n, proj_back=False, model=model, return_filters=True)
                        out[f"W_rounded_{model}_20"] = np.ascontiguousarray(Wq)
                Ypb = ref.overiva(X.copy(), n_src=K, n_iter=12, proj_back=True, model=model)
                out[f"Ypbrows_{model}_12"] = np.ascontiguousarray(Ypb[rows])
                out[f"amp_{model}_12"] = amp(lambda Xp: ref.overiva(Xp, n_src=K, n_iter=12, proj_back=True, model=model), Ypb)
            path = case_path(T, F, M, K, family)
            np.savez_compressed(path, **out)
            total += os.path.getsize(path)
            print(f"{os.path.basename(path)}: {os.path.getsize(path) / 1024:.0f} KiB; amps",
                  {k[4:]: float(f"{float(v):.3g}") for k, v in out.items() if k.startswith("amp_")})
    print(f"total {total / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
