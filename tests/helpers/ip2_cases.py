"""Inputs shared by tests/test_ip2_host.py and tests/test_ip2_gpu.py: the shapes, the seeds, the generators and the oracle runs."""
import numpy as np

from oracle import overiva_oracle as orc

import ip2_oracle as ipo

SEED = 11
MODELS = ("laplace", "gauss")
# (B, T, F, M, K) of the UPDATE stage alone: every MP (2, 4, 8), odd and even K at both parities, one and two covariance splits
# (T = 70 | 257), bin counts that leave a partly filled wavefront at 16, 4 and 1 bins per wave
UPDATE_SHAPES = [(3, 70, 17, 2, 2), (2, 70, 65, 3, 3), (2, 257, 20, 4, 4), (2, 70, 17, 4, 2), (1, 70, 5, 5, 2), (1, 257, 17, 8, 2),
                 (1, 70, 17, 8, 8), (2, 70, 33, 7, 3), (1, 70, 17, 6, 5), (1, 70, 5, 3, 1)]
UPDATE_BOTH_MODELS = [(2, 257, 20, 4, 4), (2, 70, 33, 7, 3)]
UPDATE_SEEDS = {(2, 70, 65, 3, 3): 12}     # (seed 11 leaves one of its 130 bins with two nearly equal eigenvalues in a pair step)
UPDATE_CASES = ([(shape, "laplace") for shape in UPDATE_SHAPES] + [(shape, "gauss") for shape in UPDATE_BOTH_MODELS])
# (T, F, M, K) of the iterated comparisons
IID_SHAPES = [(70, 17, 2, 2), (100, 65, 3, 3), (70, 17, 4, 2), (257, 20, 8, 2), (130, 9, 4, 4), (257, 9, 7, 3), (70, 5, 3, 1)]
MIX_SHAPES = [(70, 17, 2, 2), (100, 65, 3, 3), (70, 17, 4, 2), (257, 20, 8, 2), (257, 9, 6, 5)]
IID_COUNTS = (1, 5, 20)
MIX_COUNTS = (1, 5)
# (kind, shape, model): compared after every count of its kind
ITERATED = ([("iid", shape, "laplace") for shape in IID_SHAPES] + [("iid", (130, 9, 4, 4), "gauss")]
            + [("mix", shape, "laplace") for shape in MIX_SHAPES] + [("mix", (70, 17, 4, 2), "gauss")])


def counts(case):
    return IID_COUNTS if case[0] == "iid" else MIX_COUNTS


def case_id(case):
    kind, shape, model = case
    return f"{kind}-{'x'.join(map(str, shape))}-{model}"


def update_id(case):
    shape, model = case
    return f"{'x'.join(map(str, shape))}-{model}"


def make_x(kind, T, F, M, K, seed=SEED):
    """one room (T, F, M) complex64: i.i.d., or a mixture of K sources"""
    return orc.synth_iid(T, F, M, seed=seed) if kind == "iid" else orc.synth_mixture(T, F, M, K, seed=seed)


def make_rooms(B, T, F, M, K, seed=SEED):
    """(B, T, F, M) complex64: mixtures of K sources, one seed per room"""
    return np.stack([orc.synth_mixture(T, F, M, K, seed=seed + b) for b in range(B)])


def random_w0(B, F, M, K, seed=SEED, amp=0.1):
    """(B, F, M, K) complex128: the identity start plus a complex normal perturbation of ``amp`` per entry"""
    rng = np.random.default_rng(seed + 500)
    W0 = np.zeros((B, F, M, K), np.complex128)
    W0[:, :, :K, :] = np.eye(K)
    return W0 + amp * (rng.standard_normal(W0.shape) + 1j * rng.standard_normal(W0.shape))


def update_inputs(case):
    """(X (B, T, F, M) complex64 i.i.d. rooms, W0 (B, F, M, K)) of a case of the UPDATE stage alone.  I.i.d. rooms and a start
    near the identity keep every bin's W_hat^H V well conditioned: the stage is held to 1e-12 of the largest entry, which means
    something only where the restatement itself moves far less under a rounding-sized change of its inputs
    (test_ip2_host.py::test_update_cases_are_well_conditioned)"""
    (B, T, F, M, K), _ = case
    seed = UPDATE_SEEDS.get((B, T, F, M, K), SEED)
    X = np.stack([orc.synth_iid(T, F, M, seed=seed + b) for b in range(B)])
    return X, random_w0(B, F, M, K, seed=seed)


def perturbed(X, seed=SEED + 1000):
    """X (1 + 1e-13 g) in complex128, g a seeded standard normal"""
    g = np.random.default_rng(seed).standard_normal(X.shape)
    return X.astype(np.complex128) * (1.0 + 1e-13 * g)


def rel(a, b):
    """relative Frobenius distance"""
    return float(np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel()))


_RUNS = {}


def oracle_run(case):
    """the oracle on an iterated case and on its perturbed input, computed once: {"X": X, n: dict(W, delta)} for n in its counts,
    W the (F, M, K) demixing vectors"""
    if case not in _RUNS:
        kind, (T, F, M, K), model = case
        X = make_x(kind, T, F, M, K)
        ns = counts(case)
        a = ipo.iterate(X, K, max(ns), model, snapshots=ns)
        b = ipo.iterate(perturbed(X), K, max(ns), model, snapshots=ns)
        out = {"X": X}
        for n in ns:
            W = a[n][:, :, :K].copy()
            W.setflags(write=False)
            out[n] = dict(W=W, delta=rel(b[n][:, :, :K], W))
        _RUNS[case] = out
    return _RUNS[case]
