"""NumPy restatement of the shoebox image-source simulation of DESIGN.md 3.11, written from that statement (not from the device
code): the yardstick of tests/test_room_gpu.py.  One room per call, float64, vectorised over the images so that order 17 is usable.

    images(N)                          the triples in the order of the contract
    rir(...) -> (S, M, L), margin      impulse responses and the tie margin min | |phi| - 1/2 |
    premix(signals, rir)               full linear convolutions (np.convolve)
    mix_down(premix, ...)              mix (n_out, M), ref (K + 1, n_out, M)
"""
import numpy as np

FDL = 81
H = 40
WIN = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(FDL) / 80)


def image_count(N):
    return (2 * N + 1) * (2 * N * N + 2 * N + 3) // 3


def images(N):
    """(n_img, 3) int: |nx| + |ny| + |nz| <= N; nx ascending from -N, then ny ascending, then nz ascending"""
    out = [(nx, ny, nz) for nx in range(-N, N + 1) for ny in range(-N, N + 1) for nz in range(-N, N + 1)
           if abs(nx) + abs(ny) + abs(nz) <= N]
    return np.array(out, dtype=int).reshape(-1, 3)


def absorption6(absorption):
    a = np.asarray(absorption, dtype=float)
    return np.full(6, float(a)) if a.ndim == 0 else a.reshape(6)


def image_terms(room_dim, source, mic, absorption, fs, c, N):
    """per image of one (source, microphone) pair, in order: k (int), phi, g"""
    L = np.asarray(room_dim, dtype=float)
    s = np.asarray(source, dtype=float)
    m = np.asarray(mic, dtype=float)
    beta = np.sqrt(1.0 - absorption6(absorption))
    n = images(N)
    odd = n % 2 != 0
    pos = np.where(odd, (n + 1) * L - s, n * L + s)
    a = np.abs(n)
    more, less = (a + 1) // 2, a // 2                              # ceil(|n| / 2), floor(|n| / 2)
    at_zero = np.where(n < 0, more, less)                          # n > 0: ceil at the far wall, floor at the wall at 0
    at_far = np.where(n < 0, less, more)                           # n < 0: ceil at the wall at 0, floor at the far wall
    gain = np.ones(len(n))
    for axis in range(3):
        gain = gain * beta[2 * axis] ** at_zero[:, axis] * beta[2 * axis + 1] ** at_far[:, axis]
    d = np.sqrt(np.sum((pos - m) ** 2, axis=1))
    g = gain / (4 * np.pi * d)
    tau = fs * d / c
    k = np.floor(tau + 0.5)
    phi = tau - k
    return k.astype(int), phi, g


def rir(room_dim, sources, mics, absorption=0.35, fs=16000, c=343.0, max_order=17, rir_length=None):
    """-> rir (S, M, L) and the tie margin of the case.  The taps of the images are added in the order of the images."""
    sources, mics = np.atleast_2d(sources), np.atleast_2d(mics)
    S, M = len(sources), len(mics)
    terms = [[image_terms(room_dim, sources[s], mics[m], absorption, fs, c, max_order) for m in range(M)] for s in range(S)]
    kmax = max(int(t[0].max()) for row in terms for t in row)
    margin = min(float(np.min(np.abs(np.abs(t[1]) - 0.5))) for row in terms for t in row)
    L = kmax + FDL if rir_length is None else int(rir_length)
    if L > 65536:
        raise ValueError("impulse responses of more than 65536 samples")
    j = np.arange(FDL)
    out = np.zeros((S, M, L))
    for s in range(S):
        for m in range(M):
            k, phi, g = terms[s][m]
            taps = g[:, None] * WIN[None, :] * np.sinc(j[None, :] - H - phi[:, None])       # (n_img, 81)
            idx = k[:, None] + j[None, :]
            keep = idx < L
            # np.add.at adds unbuffered, element by element in the order of the (row-major) index array: image after image
            np.add.at(out[s, m], idx[keep], taps[keep])
    return out, margin


def premix(signals, h):
    """signals (S, n), h (S, M, L) -> (S, M, n + L - 1)"""
    S, M, L = h.shape
    return np.stack([np.stack([np.convolve(signals[s], h[s, m]) for m in range(M)]) for s in range(S)])


def mix_down(prem, n_targets, sinr, snr, ref_mic=0, sources_var=None, noise=None):
    """-> mix (n_out, M), ref (K + 1, n_out, M)"""
    S, M, n_out = prem.shape
    K = int(n_targets)
    var = np.ones(K) if sources_var is None else np.asarray(sources_var, dtype=float)
    if S == K and np.isfinite(sinr):
        raise ValueError("no interferer: sinr must be inf")
    p = prem / np.std(prem[:, ref_mic, :], axis=1)[:, None, None]
    p[:K] = p[:K] * np.sqrt(var)[:, None, None]
    sigma_n = np.sqrt(10 ** (-snr / 10) * np.sum(var))
    if S > K:
        sigma_i = np.sqrt(max(0.0, 10 ** (-sinr / 10) * np.sum(var) - sigma_n ** 2) / (S - K))
        background = sigma_i * np.sum(p[K:], axis=0)
    else:
        background = np.zeros((M, n_out))
    if noise is not None:
        background = background + sigma_n * np.asarray(noise, dtype=float).T
    mix = np.sum(p[:K], axis=0) + background
    ref = np.concatenate([p[:K].swapaxes(1, 2), background.T[None]], axis=0)
    return mix.T.copy(), ref
