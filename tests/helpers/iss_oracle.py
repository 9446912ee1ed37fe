"""NumPy restatement of the determined AuxIVA by iterative source steering that ``auxiva_iss_batch()`` runs:
float64 / complex128 throughout, one room.

Conventions are the package's: X (T, F, M) complex64 promoted to complex128, W (F, M, M) with columns as demixing vectors
(``y[t,f,k] = sum_m x[t,f,m] conj(W[f,m,k])``), p, r and phi (T, M).  The run can be stopped after any step of any sweep
(``stop``), watched step by step (``observe``), and ``cost`` is the J the iteration minimises.  The inputs of the tests come
from the generators of ``ilrma_cases`` (``make_x``), seed 11, complex64.  The checker, not the thing run: the product never
imports it.
"""
import numpy as np

import ilrma_cases as gen

EPS = 1e-15                 # overiva.py:170
SEED = gen.SEED
# (T, F, M) of the iterated comparisons, i.i.d. and mixture input; and the two that run on i.i.d. input only
ITER_SHAPES = [(70, 17, 2), (65, 5, 3), (130, 9, 8), (257, 20, 8)]
IID_ONLY_SHAPES = [(33, 4, 1), (64, 1, 5)]
ITER_COUNTS = (1, 5, 20)
MODELS = ("laplace", "gauss")
# (kind, shape, model): every one is compared after 1, 5 and 20 iterations
ITERATED = ([(kind, shape, model) for kind in ("iid", "mix") for shape in ITER_SHAPES for model in MODELS]
            + [("iid", shape, model) for shape in IID_ONLY_SHAPES for model in MODELS])
# (kind, (B, T, F, M), model) of the cost tests
COST_CASES = [("mix", (2, 70, 17, 4), "laplace"), ("iid", (1, 130, 9, 8), "laplace"), ("iid", (1, 70, 17, 2), "gauss")]


def case_id(case):
    kind, shape, model = case
    return f"{kind}-{'x'.join(map(str, shape))}-{model}"


def make_x(kind, T, F, M, seed=SEED):
    return gen.make_x(kind, T, F, M, seed=seed)


def demix(X, W):
    return np.einsum("tfm,fmk->tfk", X, np.conj(W))


def powers(Y):
    """p[t,k] = sum_f |y[t,f,k]|^2"""
    return np.sum(Y.real ** 2 + Y.imag ** 2, axis=1)


def activation(p, F, model):
    """(phi (T, M), scale (M)) from the powers, overiva.py:152-173: r = 2 sqrt(p) | p / F, g = mean_t r, r /= g, phi = 1 / max(r, eps);
    column k of W and y[:, :, k] are to be divided by scale[k] = g[k] | sqrt(g[k])"""
    r = 2.0 * np.sqrt(p) if model == "laplace" else p / F
    g = np.mean(r, axis=0)
    r = r / g[None, :]
    r[r < EPS] = EPS
    return 1.0 / r, (g if model == "laplace" else np.sqrt(g))


def step(Y, W, phi, k):
    """rank-1 step k of the sweep, in place on Y (T, F, M) and W (F, M, M); returns v (F, M)"""
    T, F, M = Y.shape
    yk = Y[:, :, k].copy()                                              # the old y_k
    a = yk.real ** 2 + yk.imag ** 2                                     # (T, F)
    d = np.einsum("tm,tf->fm", phi, a)                                  # d_m = sum_t phi[t,m] |y_k|^2
    num = np.einsum("tm,tfm,tf->fm", phi, Y, np.conj(yk))
    pos = d > 0
    v = np.zeros((F, M), np.complex128)
    v[pos] = num[pos] / d[pos]
    dk, pk = d[:, k], pos[:, k]
    v[:, k] = 0.0
    v[pk, k] = 1.0 - (dk[pk] / T) ** -0.5
    Y -= v[None, :, :] * yk[:, :, None]
    W -= np.conj(v)[:, None, :] * W[:, :, k].copy()[:, :, None]
    return v


def cost(X, W, model):
    """J = sum_{t,k} sqrt(p) (laplace) | F log(p / F) (gauss) - 2 T sum_f log|det W_f|, p from X and W"""
    T, F, _ = X.shape
    p = powers(demix(X.astype(np.complex128), W))
    g = np.sum(np.sqrt(p)) if model == "laplace" else np.sum(F * np.log(p / F))
    return float(g - 2.0 * T * np.sum(np.linalg.slogdet(W)[1]))


def projected(X, Y):
    """Y scaled onto channel 0 of X (overiva.py:197-199, no clipping)"""
    num = np.sum(np.conj(X[:, :, :1]) * Y, axis=0)
    den = np.sum(Y.real ** 2 + Y.imag ** 2, axis=0)
    z = np.ones(num.shape, np.complex128)
    z[den > 0] = num[den > 0] / den[den > 0]
    return Y * np.conj(z)[None]


def iss(X, n_iter, model="laplace", W0=None, stop=None, observe=None, snapshots=()):
    """``n_iter`` iterations from W0 (default: the identity).

    One iteration: Y = X conj(W) afresh; the activation from p (of that Y in the first iteration, of the swept Y of the iteration
    before afterwards: the same numbers up to rounding), W's columns and Y scaled; the M steps.  ``stop = (iteration, n_steps)``
    ends the run after ``n_steps`` steps of that iteration's sweep (0: after its activation).  ``observe(iteration, k, Y, W, phi,
    yk_old)`` is called after the activation (k = -1, yk_old None) and after every step k.  Returns the dict of W, Y (the swept
    signals), p (the powers of Y), phi and ``snap`` ({n: W after n iterations} for n in ``snapshots``).
    """
    X = X.astype(np.complex128)
    T, F, M = X.shape
    W = np.tile(np.eye(M, dtype=np.complex128), (F, 1, 1)) if W0 is None else np.array(np.broadcast_to(W0, (F, M, M)), np.complex128)
    Y = demix(X, W)
    p = powers(Y)
    phi, snap = None, {}
    if 0 in snapshots:
        snap[0] = W.copy()
    for it in range(n_iter):
        Y = demix(X, W)
        phi, scale = activation(p, F, model)
        W /= scale[None, None, :]
        Y /= scale[None, None, :]
        if observe is not None:
            observe(it, -1, Y, W, phi, None)
        n_steps = M if stop is None or stop[0] != it else stop[1]
        for k in range(n_steps):
            yk = Y[:, :, k].copy()
            step(Y, W, phi, k)
            if observe is not None:
                observe(it, k, Y, W, phi, yk)
        p = powers(Y)
        if it + 1 in snapshots:
            snap[it + 1] = W.copy()
        if stop is not None and stop[0] == it:
            break
    return dict(W=W, Y=Y, p=p, phi=phi, snap=snap)


def perturbed(X, seed=SEED + 1000):
    return gen.perturbed(X, seed)


rel = gen.rel
_RUNS = {}


def oracle_run(case):
    """the oracle on an iterated case and on its perturbed input, computed once: {n: dict(W, delta)} for n in ITER_COUNTS, with X"""
    if case not in _RUNS:
        kind, (T, F, M), model = case
        X = make_x(kind, T, F, M)
        a = iss(X, max(ITER_COUNTS), model, snapshots=ITER_COUNTS)["snap"]
        b = iss(perturbed(X), max(ITER_COUNTS), model, snapshots=ITER_COUNTS)["snap"]
        out = {"X": X}
        for n in ITER_COUNTS:
            a[n].setflags(write=False)
            out[n] = dict(W=a[n], delta=rel(b[n], a[n]))
        _RUNS[case] = out
    return _RUNS[case]
