"""NumPy restatement of the FIVE that ``five_batch()`` runs: float64 / complex128 throughout, one room.

Conventions are the package's: X (T, F, M) complex64 promoted to complex128, w (F, M) the demixing vector of the one output
(``y[t,f] = sum_m x[t,f,m] conj(w[f,m])``), Cx and V (F, M, M) with ``Cx[f] = mean_t x x^H``.  One iteration is given in two
formulations that differ only by rounding -- ``numpy.linalg.eigh`` on the matrix whitened by Cx, and
``scipy.linalg.eigh(V, Cx)`` -- and their distance, with the restatement's own move under a 1e-13 relative change of X, is the
yardstick the GPU tests hold the device to.  The inputs come from ``iss_oracle.make_x("mix", ...)``, seed 11 + room, complex64.
The checker, not the thing run: the product never imports it.
"""
import numpy as np
import scipy.linalg

import iss_oracle as iso

EPS = 1e-15
SEED = iso.SEED
MODELS = ("laplace", "gauss")
# (B, T, F, M): every channel count, bin counts that end inside a group of four bins (17, 65, 9, 33), one bin, frame counts below,
# at and above 64 and above one frame split of 256, odd M
SHAPES = [(3, 70, 17, 2), (2, 33, 65, 3), (2, 128, 9, 4), (2, 64, 1, 5), (1, 130, 33, 6), (1, 100, 20, 7), (2, 257, 20, 8)]
# every shape with both models, except gauss at one bin: the model degenerates there (the restatement itself moves by 1e-2 under a
# 1e-13 change of X)
CASES = [(shape, model) for shape in SHAPES for model in MODELS if not (model == "gauss" and shape[2] == 1)]
RAGGED_FRAMES, RAGGED_F, RAGGED_M = (70, 33, 128, 65), 17, 4
ITER_COUNTS = (1, 3, 10)
MIN_GAP = 0.005             # (lambda_2 - lambda_1) / lambda_2 on every bin of every compared iterate


def case_id(case):
    shape, model = case
    return "x".join(map(str, shape)) + "-" + model


def rooms(shape, seed=SEED):
    B, T, F, M = shape
    return np.stack([iso.make_x("mix", T, F, M, seed=seed + b) for b in range(B)])


def ragged_rooms(seed=SEED):
    return [iso.make_x("mix", T, RAGGED_F, RAGGED_M, seed=seed + b) for b, T in enumerate(RAGGED_FRAMES)]


def covariance(X):
    """Cx[f] = mean_t x x^H"""
    X = X.astype(np.complex128)
    return np.einsum("tfm,tfn->fmn", X, np.conj(X)) / X.shape[0]


def start(Cx):
    """the principal eigenvector of every bin's Cx (its scale and phase do not matter to what follows)"""
    return np.linalg.eigh(Cx)[1][:, :, -1]


def demix(X, w):
    return np.einsum("tfm,fm->tf", X.astype(np.complex128), np.conj(w))


def weights(X, w, model):
    """1 / max(r / mean r, eps), r = 2 sqrt(p) (laplace) | p / F (gauss), p_t = sum_f |w^H x|^2"""
    y = demix(X, w)
    p = np.sum(y.real ** 2 + y.imag ** 2, axis=1)
    r = 2.0 * np.sqrt(p) if model == "laplace" else p / X.shape[1]
    r = r / np.mean(r)
    r[r < EPS] = EPS
    return 1.0 / r


def weighted_cov(X, phi):
    """V[f] = mean_t phi_t x x^H"""
    X = X.astype(np.complex128)
    return np.einsum("t,tfm,tfn->fmn", phi, X, np.conj(X)) / X.shape[0]


def step_whitened(V, Cx):
    """(w (F, M), lambda (F, M) ascending): Q = E Lambda^-1/2 of Cx = E Lambda E^H, numpy.linalg.eigh of Q^H V Q, w = Q u /
    sqrt(lambda_1)"""
    lc, E = np.linalg.eigh(Cx)
    Q = E / np.sqrt(lc)[:, None, :]
    A = np.conj(np.swapaxes(Q, 1, 2)) @ V @ Q
    A = 0.5 * (A + np.conj(np.swapaxes(A, 1, 2)))
    lam, U = np.linalg.eigh(A)
    w = np.einsum("fmn,fn->fm", Q, U[:, :, 0]) / np.sqrt(lam[:, :1])
    return w, lam


def step_pencil(V, Cx):
    """the same from scipy.linalg.eigh(V, Cx) per bin, w = u / sqrt(u^H V u)"""
    F, M, _ = V.shape
    w, lam = np.empty((F, M), np.complex128), np.empty((F, M))
    for f in range(F):
        lam[f], vecs = scipy.linalg.eigh(V[f], Cx[f])
        u = vecs[:, 0]
        w[f] = u / np.sqrt(np.real(np.conj(u) @ V[f] @ u))
    return w, lam


def gaps(lam):
    """(lambda_2 - lambda_1) / lambda_2 per bin (1 with one channel)"""
    if lam.shape[1] < 2:
        return np.ones(lam.shape[0])
    return (lam[:, 1] - lam[:, 0]) / lam[:, 1]


def five(X, n_iter, model="laplace", w0=None, step=step_whitened, snapshots=()):
    """``n_iter`` iterations from w0 (default: ``start``).  Returns dict(w, min_gap (the smallest relative gap over all bins and
    iterations), snap ({n: w after n iterations} for n in ``snapshots``))"""
    Cx = covariance(X)
    w = start(Cx) if w0 is None else np.array(w0, np.complex128)
    snap, min_gap = {}, np.inf
    for it in range(n_iter):
        V = weighted_cov(X, weights(X, w, model))
        w, lam = step(V, Cx)
        min_gap = min(min_gap, float(gaps(lam).min()))
        if it + 1 in snapshots:
            snap[it + 1] = w.copy()
    return dict(w=w, min_gap=min_gap, snap=snap)


def wdist(w, wref):
    """phase-free distance: every bin of w turned by the phase of wref^H w, then the maximum difference over the maximum
    magnitude; w (..., F, M)"""
    a = np.sum(np.conj(wref) * w, axis=-1, keepdims=True)
    mag = np.abs(a)
    ph = np.where(mag > 0, a / np.where(mag > 0, mag, 1.0), 1.0)
    return float(np.max(np.abs(w * np.conj(ph) - wref)) / np.max(np.abs(wref)))


def dist(a, b):
    """maximum absolute difference over the maximum magnitude"""
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def projected(X, w):
    """the output projected back onto channel 0 of X (T, F): free of the phase of w"""
    y = demix(X, w)
    num = np.sum(np.conj(X[:, :, 0].astype(np.complex128)) * y, axis=0)
    den = np.sum(y.real ** 2 + y.imag ** 2, axis=0)
    z = np.ones(num.shape, np.complex128)
    z[den > 0] = num[den > 0] / den[den > 0]
    return y * np.conj(z)[None]


def perturbed(X, seed=SEED + 1000):
    return iso.perturbed(X, seed)


def one_step(X, w0, model, step=step_whitened):
    """one iteration from w0: (w, lambda)"""
    return step(weighted_cov(X, weights(X, w0, model)), covariance(X))


def yardstick(X, w0, model, counts=ITER_COUNTS):
    """per iteration count n: the restatement's w and projected-back y after n iterations from w0, the smallest gap met, and the
    yardsticks 10 max(distance between the two formulations, move under a 1e-13 relative change of X) of w (phase-free) and of
    y.  dict {n: dict(w, y, tol_w, tol_y)}, "min_gap" """
    n = max(counts)
    a = five(X, n, model, w0, step_whitened, counts)
    b = five(X, n, model, w0, step_pencil, counts)
    Xp = perturbed(X)
    c = five(Xp, n, model, w0, step_whitened, counts)
    out = {"min_gap": min(a["min_gap"], b["min_gap"], c["min_gap"])}
    for k in counts:
        w, y = a["snap"][k], projected(X, a["snap"][k])
        d_w = max(wdist(b["snap"][k], w), wdist(c["snap"][k], w))
        d_y = max(dist(projected(X, b["snap"][k]), y), dist(projected(Xp, c["snap"][k]), y))
        out[k] = dict(w=w, y=y, tol_w=10.0 * d_w, tol_y=10.0 * d_y, d_w=d_w, d_y=d_y)
    return out
