"""NumPy restatement of the BSS Eval "sources" criteria (Vincent, Gribonval, Fevotte 2006; time-invariant filter of Lf taps), written
from DESIGN.md 3.10 and the published description of the criteria.  Two forms:

``bss_eval_td``    the time-domain form: zero-extend by Lf - 1, correlations by FFT of length 2^ceil(log2(n + Lf - 1)), Toeplitz
                   blocks, ``np.linalg.solve``, filter the references, subtract to get s_target, e_spat, e_interf and e_artif, form
                   the energy ratios
``bss_eval_gram``  the Gram formulas of DESIGN.md 3.10 with direct sums: no FFT, no filtered signal

Both return ``sdr, sir, sar`` as (N, N) matrices indexed [estimate, reference].  float64 throughout.
"""
import numpy as np


def _db(num, den):
    with np.errstate(divide="ignore"):
        return np.inf if den == 0 else 10.0 * np.log10(num / den)


def toeplitz_gram(r, N, Lf):
    """G[(i,p),(j,q)] = r[i][j][p - q] from r (N, N, 2 Lf - 1) holding lags -(Lf-1) .. Lf-1"""
    lag = np.arange(Lf)[:, None] - np.arange(Lf)[None, :] + (Lf - 1)
    G = np.empty((N * Lf, N * Lf))
    for i in range(N):
        for j in range(N):
            G[i * Lf:(i + 1) * Lf, j * Lf:(j + 1) * Lf] = r[i, j][lag]
    return G


# ---- direct sums -------------------------------------------------------------------------------------------------------------
def lag_sums_direct(ref, est, Lf):
    """r (N, N, 2 Lf - 1): r[i,j][Lf-1+tau] = sum_u s_i[u] s_j[u+tau];  D (N, N, Lf): D[k,i,p] = sum_u s_i[u] e_k[u+p];  E (N,)"""
    N, n = ref.shape
    r = np.zeros((N, N, 2 * Lf - 1))
    D = np.zeros((N, N, Lf))
    for tau in range(min(Lf, n)):
        for i in range(N):
            for j in range(N):
                v = np.dot(ref[i, :n - tau], ref[j, tau:])
                r[i, j, Lf - 1 + tau] = v
                r[j, i, Lf - 1 - tau] = v
            for k in range(N):
                D[k, i, tau] = np.dot(ref[i, :n - tau], est[k, tau:])
    return r, D, np.sum(est * est, axis=1)


def gram_direct(ref, est, Lf):
    """G (N Lf, N Lf), D (N, N Lf), E (N,) with direct sums"""
    N = ref.shape[0]
    r, D, E = lag_sums_direct(ref, est, Lf)
    return toeplitz_gram(r, N, Lf), D.reshape(N, N * Lf), E


def criteria_from_gram(G, D, E, N, Lf):
    """the five quadratic forms and three ratios of DESIGN.md 3.10 for all (k, j)"""
    C = np.linalg.solve(G, D.T).T                                   # (N, N Lf)
    sdr, sir, sar = np.empty((N, N)), np.empty((N, N)), np.empty((N, N))
    for k in range(N):
        tot = C[k] @ G @ C[k]
        art = E[k] - 2.0 * D[k] @ C[k] + tot
        for j in range(N):
            sl = slice(j * Lf, (j + 1) * Lf)
            Gjj = G[sl, sl]
            c = np.linalg.solve(Gjj, D[k, sl])
            a = c @ Gjj @ c
            res = E[k] - 2.0 * D[k, sl] @ c + a
            d = C[k].copy()
            d[sl] -= c
            interf = d @ G @ d
            sdr[k, j] = _db(a, res)
            sir[k, j] = np.inf if N == 1 else _db(a, interf)
            sar[k, j] = _db(tot, art)
    return sdr, sir, sar


def bss_eval_gram(ref, est, Lf):
    ref, est = np.asarray(ref, dtype=np.float64), np.asarray(est, dtype=np.float64)
    G, D, E = gram_direct(ref, est, Lf)
    return criteria_from_gram(G, D, E, ref.shape[0], Lf)


# ---- time domain ---------------------------------------------------------------------------------------------------------------
def _project(refs, est_k, Lf):
    """least-squares projection of est_k on the span of the references delayed by 0..Lf-1: the filtered sum, n + Lf - 1 samples"""
    M, n = refs.shape
    nfft = 1 << int(np.ceil(np.log2(n + Lf - 1)))
    sf = np.fft.rfft(np.hstack([refs, np.zeros((M, Lf - 1))]), nfft, axis=1)
    ef = np.fft.rfft(np.hstack([est_k, np.zeros(Lf - 1)]), nfft)
    r = np.empty((M, M, 2 * Lf - 1))
    for i in range(M):
        for j in range(M):
            ss = np.fft.irfft(np.conj(sf[i]) * sf[j], nfft)         # ss[tau] = sum_u s_i[u] s_j[u + tau], circular
            r[i, j] = np.hstack([ss[nfft - Lf + 1:], ss[:Lf]]) if Lf > 1 else ss[:1]
    G = toeplitz_gram(r, M, Lf)
    D = np.empty(M * Lf)
    for i in range(M):
        D[i * Lf:(i + 1) * Lf] = np.fft.irfft(np.conj(sf[i]) * ef, nfft)[:Lf]
    C = np.linalg.solve(G, D).reshape(M, Lf)
    out = np.zeros(n + Lf - 1)
    for i in range(M):
        out += np.convolve(refs[i], C[i])[:n + Lf - 1]
    return out


def bss_eval_td(ref, est, Lf):
    ref, est = np.asarray(ref, dtype=np.float64), np.asarray(est, dtype=np.float64)
    N, n = ref.shape
    sdr, sir, sar = np.empty((N, N)), np.empty((N, N)), np.empty((N, N))
    for k in range(N):
        p_all = _project(ref, est[k], Lf)
        e_artif = np.hstack([est[k], np.zeros(Lf - 1)]) - p_all
        for j in range(N):
            s_true = np.hstack([ref[j], np.zeros(Lf - 1)])
            p_j = _project(ref[j:j + 1], est[k], Lf)
            e_spat = p_j - s_true
            e_interf = p_all - p_j
            s_filt = s_true + e_spat
            sdr[k, j] = _db(np.sum(s_filt ** 2), np.sum((e_interf + e_artif) ** 2))
            sir[k, j] = np.inf if N == 1 else _db(np.sum(s_filt ** 2), np.sum(e_interf ** 2))
            sar[k, j] = _db(np.sum((s_filt + e_interf) ** 2), np.sum(e_artif ** 2))
    return sdr, sir, sar


def best_permutation(sir):
    """the rule of bss_eval_batch, restated: maximise mean_j sir[perm[j], j], ties to the first in itertools order"""
    import itertools

    N = sir.shape[0]
    best, best_mean = None, -np.inf
    for perm in itertools.permutations(range(N)):
        m = np.mean([sir[perm[j], j] for j in range(N)])
        if best is None or m > best_mean:
            best, best_mean = perm, m
    return np.array(best)
