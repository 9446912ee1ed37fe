"""NumPy restatement of the ILRMA that ``ilrma_batch()`` runs: float64 / complex128 throughout, one room.

Conventions are the package's: X (T, F, M) complex64 promoted to complex128, W (F, M, K) with columns as demixing vectors
(``y[t,f,s] = sum_m x[t,f,m] conj(W[f,m,s])``), K = M, Tn (K, F, L), Vn (K, L, T), R = Tn @ Vn and P = |y|^2 both (K, F, T).
The checker, not the thing run: the product never imports it.
"""
import numpy as np

EPS = np.finfo(np.float64).eps


def power(X, W):
    """P[s,f,t] = |y[t,f,s]|^2"""
    Y = np.einsum("tfm,fms->sft", X, np.conj(W))
    return Y.real ** 2 + Y.imag ** 2


def update_t(P, R, Tn, Vn, s):
    """the T update of source s and its R (step 1, first half)"""
    iR = 1.0 / R[s]
    Tn[s] *= np.sqrt(((P[s] * iR ** 2) @ Vn[s].T) / (iR @ Vn[s].T))
    Tn[s][Tn[s] < EPS] = EPS
    R[s] = Tn[s] @ Vn[s]


def update_v(P, R, Tn, Vn, s):
    """the V update of source s (step 1, second half); R[s] still to be rewritten"""
    iR = 1.0 / R[s]
    Vn[s] *= np.sqrt((Tn[s].T @ (P[s] * iR ** 2)) / (Tn[s].T @ iR))
    Vn[s][Vn[s] < EPS] = EPS


def rewrite_r(R, Tn, Vn, s):
    R[s] = Tn[s] @ Vn[s]


def weighted_cov(X, R, s):
    """C_s[f] = (1/T) sum_t x[t,f] x[t,f]^H / R[s,f,t], (F, M, M)"""
    T = X.shape[0]
    return np.einsum("ft,tfc,tfd->fcd", 1.0 / R[s], X, np.conj(X)) / T


def ip1(W, C, s):
    """w_s <- (W^H C_s)^-1 e_s, w_s /= sqrt(w_s^H C_s w_s), in place (overiva.py:181-186 with V = C_s)"""
    F, M, _ = W.shape
    A = np.conj(np.transpose(W, (0, 2, 1))) @ C
    e = np.zeros((F, M, 1), np.complex128)
    e[:, s, 0] = 1.0
    w = np.linalg.solve(A, e)[:, :, 0]
    d = np.einsum("fc,fcd,fd->f", np.conj(w), C, w).real
    W[:, :, s] = w / np.sqrt(d)[:, None]


def normalise(X, W, Tn, R):
    """step 4: P from the new W, lambda_s = sqrt(mean P[s]); W, P, R and Tn scaled in place; returns (P, lambda)"""
    P = power(X, W)
    lam = np.sqrt(np.mean(P, axis=(1, 2)))
    W /= lam[None, None, :]
    P /= lam[:, None, None] ** 2
    R /= lam[:, None, None] ** 2
    Tn /= lam[:, None, None] ** 2
    return P, lam


def cost(P, R, W):
    """Q = sum (P / R + log R) - 2 T sum_f log |det W_f|"""
    T = P.shape[2]
    _, logdet = np.linalg.slogdet(W)
    return float(np.sum(P / R + np.log(R)) - 2.0 * T * np.sum(logdet))


def default_init(B, T, F, M, L, seed=None):
    """the documented default start of ``ilrma_batch``: (T0 (B, M, F, L), V0 (B, M, L, T))"""
    rng = np.random.RandomState(seed)
    T0 = 0.1 + 0.9 * rng.rand(B, M, F, L)
    V0 = 0.1 + 0.9 * rng.rand(B, M, L, T)
    return T0, V0


def start(X, T0, V0, W0=None):
    """(X128, W, Tn, Vn, R, P) of epoch 0"""
    X = np.asarray(X).astype(np.complex128)          # (complex64 data promoted; a complex128 X is taken as it is)
    T, F, M = X.shape
    W = np.tile(np.eye(M, dtype=np.complex128), (F, 1, 1)) if W0 is None else np.array(np.broadcast_to(W0, (F, M, M)), np.complex128)
    Tn = np.array(T0, np.float64)
    Vn = np.array(V0, np.float64)
    R = Tn @ Vn
    return X, W, Tn, Vn, R, power(X, W)


def ilrma(X, n_iter, T0, V0, W0=None, interleaved=False, observe=None):
    """``n_iter`` epochs; returns (W, Tn, Vn, R, P).  ``interleaved``: steps 1-3 per source, as pra writes them, instead of
    stage-wise.  ``observe(step, P, R, W)`` is called after the start (step 0) and after every step 1, 3 and 4; between step 3
    and step 4 it is given the P of the new W."""
    X, W, Tn, Vn, R, P = start(X, T0, V0, W0)
    M = X.shape[2]
    if observe:
        observe(0, P, R, W)
    for _ in range(n_iter):
        if interleaved:
            for s in range(M):
                update_t(P, R, Tn, Vn, s)
                update_v(P, R, Tn, Vn, s)
                rewrite_r(R, Tn, Vn, s)
                ip1(W, weighted_cov(X, R, s), s)
        else:
            for s in range(M):
                update_t(P, R, Tn, Vn, s)
                update_v(P, R, Tn, Vn, s)
                rewrite_r(R, Tn, Vn, s)
            if observe:
                observe(1, P, R, W)
            C = [weighted_cov(X, R, s) for s in range(M)]
            for s in range(M):
                ip1(W, C[s], s)
        if observe:
            observe(3, power(X, W), R, W)
        P, _ = normalise(X, W, Tn, R)
        if observe:
            observe(4, P, R, W)
    return W, Tn, Vn, R, P


def demix(X, W):
    """Y (T, F, K) in complex128, without projection back"""
    return np.einsum("tfm,fms->tfs", np.asarray(X).astype(np.complex128), np.conj(W))
