"""NumPy restatement of OverIVA / AuxIVA with pairwise IP2 updates as ``overiva_ip2_batch()`` runs it: float64 /
complex128 throughout, one room, every bin at once.

Conventions are ``overiva()``'s: X (T, F, M), W_hat (F, M, M) whose first K columns are the demixing vectors (``y_s = w_s^H x``),
the background block [J; -I], Cx the input covariance, V (F, K, M, M) the weighted covariances of an iteration, all formed from
the r of its start.  The checker, not the thing run: the product never imports it.
"""
import numpy as np

EPS = 1e-15                 # overiva.py:170


def herm(A):
    return np.conj(np.swapaxes(A, -1, -2))


def schedule(K, n):
    """the steps of iteration n: tuples (a, b) and (s,)"""
    if K == 1:
        return [(0,)]
    if K == 2:
        return [(0, 1)]
    first = 0 if n % 2 == 0 else 1
    steps = [(0,)] if first else []
    steps += [(s, s + 1) for s in range(first, K - 1, 2)]
    if (K - first) % 2:
        steps.append((K - 1,))
    return steps


def input_covariance(X):
    X = X.astype(np.complex128)
    return np.einsum("tfi,tfj->fij", X, np.conj(X)) / X.shape[0]


def update_j(W_hat, Cx, K):
    """J from the orthogonality constraint, overiva.py:96-98, in place"""
    M = W_hat.shape[1]
    if K < M:
        tmp = herm(W_hat[:, :, :K]) @ Cx
        W_hat[:, :K, K:] = np.linalg.solve(tmp[:, :, :K], tmp[:, :, K:])


def init_w_hat(Cx, K, W0=None):
    """overiva.py:89-123 without the eigenvector start"""
    F, M, _ = Cx.shape
    W_hat = np.zeros((F, M, M), np.complex128)
    if W0 is None:
        W_hat[:, :K, :K] = np.eye(K)
    else:
        W_hat[:, :, :K] = np.broadcast_to(W0, (F, M, K))
    if K < M:
        update_j(W_hat, Cx, K)
        W_hat[:, K:, K:] = -np.eye(M - K)
    return W_hat


def single_step(W_hat, Vs, s):
    """IP1 on source s, overiva.py:181-186, in place"""
    F, M, _ = W_hat.shape
    e = np.zeros((F, M, 1), np.complex128)
    e[:, s, 0] = 1.0
    w = np.linalg.solve(herm(W_hat) @ Vs, e)
    d = np.real(herm(w) @ Vs @ w)
    W_hat[:, :, s] = (w / np.sqrt(d))[:, :, 0]


def _p_u(W_hat, Vs, a, b):
    F, M, _ = W_hat.shape
    E = np.zeros((F, M, 2), np.complex128)
    E[:, a, 0] = 1.0
    E[:, b, 1] = 1.0
    P = np.linalg.solve(herm(W_hat) @ Vs, E)
    U = herm(P) @ Vs @ P
    return P, 0.5 * (U + herm(U))


def rotate(Ua, Ub):
    """(h_a, h_b), each (F, 2): the closed form of the generalised eigenvectors of (U_a, U_b) by one rotation, normalised"""
    L = np.linalg.cholesky(Ub)
    Li = np.linalg.inv(L)
    C = Li @ Ua @ herm(Li)
    p, q, z = C[:, 0, 0].real, C[:, 1, 1].real, C[:, 0, 1]
    az = np.abs(z)
    nz = az > 0
    safe = np.where(nz, az, 1.0)
    phi = np.where(nz, z / safe, 1.0 + 0.0j)
    tau = (q - p) / (2.0 * safe)
    t = np.where(tau == 0, 1.0, np.where(tau > 0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1.0 + tau * tau)))
    t = np.where(nz, t, 0.0)
    c = 1.0 / np.sqrt(1.0 + t * t)
    s = t * c
    v1 = np.stack([c + 0.0j, -s * np.conj(phi)], axis=-1)
    v2 = np.stack([s * phi, c + 0.0j], axis=-1)
    lam1, lam2 = p - t * az, q + t * az
    first = (lam1 >= lam2)[:, None]
    q_hi, q_lo = np.where(first, v1, v2), np.where(first, v2, v1)
    LiH = herm(Li)
    ha = (LiH @ q_hi[:, :, None])
    hb = (LiH @ q_lo[:, :, None])
    ha = ha / np.sqrt(np.real(herm(ha) @ Ua @ ha))
    hb = hb / np.sqrt(np.real(herm(hb) @ Ub @ hb))
    return ha[:, :, 0], hb[:, :, 0]


def rotate_eigh(Ua, Ub):
    """the same from scipy.linalg.eigh(U_a, U_b): equal to ``rotate`` up to a unit phase per vector"""
    import scipy.linalg

    F = Ua.shape[0]
    ha, hb = np.empty((F, 2), np.complex128), np.empty((F, 2), np.complex128)
    for f in range(F):
        lam, vec = scipy.linalg.eigh(Ua[f], Ub[f])           # ascending
        a, b = vec[:, 1], vec[:, 0]
        ha[f] = a / np.sqrt(np.real(np.conj(a) @ Ua[f] @ a))
        hb[f] = b / np.sqrt(np.real(np.conj(b) @ Ub[f] @ b))
    return ha, hb


def pair_step(W_hat, Va, Vb, a, b, rotation=rotate):
    """the pair step (a, b), in place"""
    Pa, Ua = _p_u(W_hat, Va, a, b)
    Pb, Ub = _p_u(W_hat, Vb, a, b)
    ha, hb = rotation(Ua, Ub)
    W_hat[:, :, a] = (Pa @ ha[:, :, None])[:, :, 0]
    W_hat[:, :, b] = (Pb @ hb[:, :, None])[:, :, 0]


def update(W_hat, V, Cx, K, n, rotation=rotate, observe=None):
    """the schedule of iteration n on a copy of W_hat with V (F, K, M, M) fixed, J after every step; ``observe(step, phase,
    W_hat)`` is called after every step's vectors are set (phase "step") and after its J update (phase "j")"""
    W_hat = np.array(W_hat, np.complex128)
    for step in schedule(K, n):
        if len(step) == 1:
            single_step(W_hat, V[:, step[0]], step[0])
        else:
            pair_step(W_hat, V[:, step[0]], V[:, step[1]], step[0], step[1], rotation)
        if observe is not None:
            observe(step, "step", W_hat)
        update_j(W_hat, Cx, K)
        if observe is not None:
            observe(step, "j", W_hat)
    return W_hat


def update_ip1(W_hat, V, Cx, K, sources=None):
    """IP1 on the given sources in order (default all), J after every one: the reference's update"""
    W_hat = np.array(W_hat, np.complex128)
    for s in range(K) if sources is None else sources:
        single_step(W_hat, V[:, s], s)
        update_j(W_hat, Cx, K)
    return W_hat


def weights(X, W_hat, K, model, normalise=True):
    """overiva.py:140-173: (r_inv (T, K), scale (K)) -- W's columns are to be divided by scale"""
    T, F, M = X.shape
    Y = np.einsum("tfm,fmk->tfk", X, np.conj(W_hat[:, :, :K]))
    p = np.sum(Y.real ** 2 + Y.imag ** 2, axis=1)
    r = 2.0 * np.sqrt(p) if model == "laplace" else p / F
    scale = np.ones(K)
    if normalise:
        g = np.mean(r, axis=0)
        r = r / g[None, :]
        scale = g if model == "laplace" else np.sqrt(g)
    r = np.where(r < EPS, EPS, r)
    return 1.0 / r, scale


def weighted_cov(X, r_inv):
    """V (F, K, M, M), overiva.py:179 for every source"""
    return np.einsum("tfi,tk,tfj->fkij", X, r_inv, np.conj(X)) / X.shape[0]


def iterate(X, K, n_iter, model="laplace", W0=None, first=0, W_hat=None, normalise=True, ip1=False, snapshots=(), costs=None):
    """iterations first .. first + n_iter - 1 from W0 (or from a W_hat of an earlier call).  Returns W_hat, or with ``snapshots``
    {n: W_hat after iteration index n - 1}.  ``ip1``: the reference's IP1 sweep instead of the schedule.  ``costs``: a list that
    receives the cost before every iteration and after the last."""
    X = X.astype(np.complex128)
    Cx = input_covariance(X)
    W_hat = init_w_hat(Cx, K, W0) if W_hat is None else np.array(W_hat, np.complex128)
    snap = {}
    if first in snapshots:
        snap[first] = W_hat.copy()
    for n in range(first, first + n_iter):
        if costs is not None:
            costs.append(cost(X, W_hat, K, model))
        r_inv, scale = weights(X, W_hat, K, model, normalise)
        W_hat[:, :, :K] /= scale[None, None, :]
        V = weighted_cov(X, r_inv)
        W_hat = update_ip1(W_hat, V, Cx, K) if ip1 else update(W_hat, V, Cx, K, n)
        if n + 1 in snapshots:
            snap[n + 1] = W_hat.copy()
    if costs is not None:
        costs.append(cost(X, W_hat, K, model))
    return snap if snapshots else W_hat


def surrogate(W_hat, V, K):
    """sum_s w_s^H V_s w_s - 2 log|det W_hat| per bin, (F,)"""
    W = W_hat[:, :, :K]
    quad = np.real(np.einsum("fis,fsij,fjs->f", np.conj(W), V, W))
    return quad - 2.0 * np.linalg.slogdet(W_hat)[1]


def cost(X, W_hat, K, model):
    """sum_{t,s} sqrt(p) (laplace) | F log(p / F) (gauss) - 2 T sum_f log|det W_hat_f|: what the iteration minimises when the scale
    normalisation is left out (for K < M up to the background's constant term)"""
    T, F, _ = X.shape
    Y = np.einsum("tfm,fmk->tfk", X.astype(np.complex128), np.conj(W_hat[:, :, :K]))
    p = np.sum(Y.real ** 2 + Y.imag ** 2, axis=1)
    g = np.sum(np.sqrt(p)) if model == "laplace" else np.sum(F * np.log(p / F))
    return float(g - 2.0 * T * np.sum(np.linalg.slogdet(W_hat)[1]))


def pair_properties(W_hat, Va, Vb, a, b, others=None):
    """the largest deviation from the defining properties of a pair step on (a, b): unit quadratic forms, the two cross terms and
    the orthogonality of the other columns of W_hat (all of them, or ``others``) to V_a w_a and V_b w_b.  The last holds for the
    columns as they are when the step ends: before its J update and before any later step moves them"""
    M = W_hat.shape[1]
    wa, wb = W_hat[:, :, a], W_hat[:, :, b]
    ga = np.einsum("fij,fj->fi", Va, wa)          # V_a w_a
    gb = np.einsum("fij,fj->fi", Vb, wb)
    worst = max(np.max(np.abs(np.einsum("fi,fi->f", np.conj(wa), ga) - 1.0)), np.max(np.abs(np.einsum("fi,fi->f", np.conj(wb), gb) - 1.0)))
    worst = max(worst, np.max(np.abs(np.einsum("fi,fi->f", np.conj(wb), ga))), np.max(np.abs(np.einsum("fi,fi->f", np.conj(wa), gb))))
    for j in range(M) if others is None else others:
        if j not in (a, b):
            wj = W_hat[:, :, j]
            worst = max(worst, np.max(np.abs(np.einsum("fi,fi->f", np.conj(wj), ga))), np.max(np.abs(np.einsum("fi,fi->f", np.conj(wj), gb))))
    return float(worst)


def single_properties(W_hat, Vs, s, others=None):
    """the same for an IP1 step: w_s^H V_s w_s = 1 and w_j^H V_s w_s = 0 for the other columns"""
    g = np.einsum("fij,fj->fi", Vs, W_hat[:, :, s])
    worst = 0.0
    for j in range(W_hat.shape[1]) if others is None else [s] + [o for o in others if o != s]:
        v = np.einsum("fi,fi->f", np.conj(W_hat[:, :, j]), g)
        worst = max(worst, np.max(np.abs(v - (1.0 if j == s else 0.0))))
    return float(worst)


def j_orthogonality(W_hat, Cx, K):
    """max |W^H Cx [J; -I]|, relative to max |W^H Cx|"""
    M = W_hat.shape[1]
    if K == M:
        return 0.0
    t = herm(W_hat[:, :, :K]) @ Cx
    return float(np.max(np.abs(t @ W_hat[:, :, K:])) / np.max(np.abs(t)))
