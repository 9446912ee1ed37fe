"""Inputs shared by tests/test_ilrma_host.py and tests/test_ilrma_gpu.py: the iterated-parity cases and their generators."""
import numpy as np

from oracle import overiva_oracle as orc

import ilrma_oracle as ilo

SEED = 11
# (T, F, M, L) of the iterated comparisons: no case has fewer than 70 frames (a mixture at 33 frames, M = L = 3, overfits)
SHORT_SHAPES = [(70, 17, 2, 2), (100, 65, 3, 3), (70, 17, 4, 2), (257, 20, 8, 2)]
LONG_SHAPES = [(70, 17, 2, 2), (100, 65, 3, 3), (257, 20, 8, 2)]
# the component counts and channel counts the shapes above leave out: LP = 8 and 16 with L below and at LP, LP = 4 exact, M = 6, 7
WIDE_SHAPES = [(70, 17, 6, 5), (100, 33, 7, 8), (130, 17, 3, 9), (64, 16, 2, 16), (128, 64, 2, 16), (70, 17, 4, 4)]
ONE_CHANNEL = (70, 5, 1, 4)          # i.i.d. only: a one-source mixture is the same thing
# (kind, shape, n_iter): 1 and 5 epochs on i.i.d. and mixture input, 20 epochs on i.i.d. input only
ITERATED = ([(kind, shape, n) for kind in ("iid", "mix") for shape in SHORT_SHAPES for n in (1, 5)]
            + [("iid", shape, 20) for shape in LONG_SHAPES]
            + [(kind, shape, n) for kind in ("iid", "mix") for shape in WIDE_SHAPES for n in (1, 5)]
            + [("iid", ONE_CHANNEL, n) for n in (1, 5)])


def case_id(case):
    kind, (T, F, M, L), n = case
    return f"{kind}-{T}x{F}x{M}-L{L}-n{n}"


def make_x(kind, T, F, M, seed=SEED):
    """one room (T, F, M) complex64: i.i.d., or a mixture of M sources"""
    return orc.synth_iid(T, F, M, seed=seed) if kind == "iid" else orc.synth_mixture(T, F, M, M, seed=seed)


def make_nmf(T, F, M, L, seed=SEED, B=1):
    """(T0 (B, M, F, L), V0 (B, M, L, T)) by the documented default recipe"""
    return ilo.default_init(B, T, F, M, L, seed=seed)


def perturbed(X, seed=SEED + 1000):
    """X (1 + 1e-13 g) in complex128, g a seeded standard normal"""
    g = np.random.default_rng(seed).standard_normal(X.shape)
    return X.astype(np.complex128) * (1.0 + 1e-13 * g)


def rel(a, b):
    """relative Frobenius distance"""
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


_ORACLE = {}


def oracle_run(case):
    """the oracle on the case and on its perturbed input, computed once: dict with W, Tn, Vn, R, delta (of W), delta_R"""
    if case not in _ORACLE:
        kind, (T, F, M, L), n = case
        X = make_x(kind, T, F, M)
        T0, V0 = make_nmf(T, F, M, L)
        W, Tn, Vn, R, _ = ilo.ilrma(X, n, T0[0], V0[0])
        W2, _, _, R2, _ = ilo.ilrma(perturbed(X), n, T0[0], V0[0])
        for a in (W, Tn, Vn, R):
            a.setflags(write=False)
        _ORACLE[case] = dict(X=X, T0=T0, V0=V0, W=W, Tn=Tn, Vn=Vn, R=R, delta=rel(W2, W), delta_R=rel(R2, R))
    return _ORACLE[case]
