"""The fixtures of the complex128 data path (tests/golden/c128_*.npz, written by tests/golden/make_c128_golden.py) as the host and
the GPU tests read them: the input is regenerated, not stored."""
import glob
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_c128_golden as mk  # noqa: E402

HEADER = os.path.join(os.path.dirname(HERE), "include", "overiva_hip.h")
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "c128_*.npz")))
AMP_LIMIT = 1e3      # as conftest.AMP_LIMIT


def load_case(path):
    """the fixture, its regenerated input and K"""
    with np.load(path) as d:
        g = {k: d[k] for k in d.files}
    T, F, M, K = (int(g[k]) for k in ("T", "F", "M", "K"))
    X = mk.make_input(str(g["family"]), T, F, M)
    assert X.dtype == np.complex128 and X.shape == (T, F, M)
    assert abs(X.sum() - g["X_sum"]) < 1e-9 * float(g["X_abs"]) and abs(np.abs(X).sum() - g["X_abs"]) < 1e-9 * float(g["X_abs"])
    return g, X, K


def admitted(g, model, n):
    """a row is compared only when the reference itself is well conditioned there (conftest.chaotic's cap)"""
    return float(g[f"amp_{model}_{n}"]) <= AMP_LIMIT
