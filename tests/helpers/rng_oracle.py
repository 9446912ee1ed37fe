"""NumPy restatement of the seeded normal stream of DESIGN.md 3.13, written from that statement.

Philox-4x64-10 on the counter (j, purpose, 0, 0) under the key (k0, k1): ten rounds of

    c = [hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)],  then  k0 += W0, k1 += W1  (mod 2^64)

with the 64 x 64 -> 128-bit products formed from 32-bit halves.  A word w gives u = ((w >> 12) + 0.5) 2^-52; words 0, 1 give
r cos(2 pi u1), r sin(2 pi u1) with r = sqrt(-2 ln u0); words 2, 3 the next two.  Element n of a stream is value n mod 4 of block
n div 4.  tests/test_rng_host.py pins the raw words to numpy.random.Philox."""
import numpy as np

M0, M1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157
W0, W1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B
ALL_ONES = (1 << 64) - 1
# (key, purpose, block) of the raw-word tests: block 0 (numpy's counter wraps to get there, for purpose 0 through all four words),
# a key word with all bits set, j next to 2^32 and the last block 2^64 - 1
RAW_CASES = [((0, 0), 0, 0), ((123, 0), 0, 0), ((123, 0), 1, 0), ((123, 1), 0, 5), ((ALL_ONES, 0), 3, 0), ((7, ALL_ONES), 1, 1),
             ((2 ** 63 + 11, 42), 0, 2 ** 32 - 1), ((2 ** 63 + 11, 42), 0, 2 ** 32), ((99, 0), 2 ** 40, 2 ** 32 + 1),
             ((5, 6), 1, ALL_ONES)]
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def mulhilo(a, b):
    """(hi, lo) of the 128-bit product of the constant a and the uint64 array b"""
    a = np.uint64(a)
    a0, a1 = a & _LOW, a >> _S32
    b0, b1 = b & _LOW, b >> _S32
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1            # each below 2^64
    mid = (p00 >> _S32) + (p01 & _LOW) + (p10 & _LOW)                   # below 3 * 2^32
    hi = p11 + (p01 >> _S32) + (p10 >> _S32) + (mid >> _S32)
    lo = (mid << _S32) | (p00 & _LOW)
    return hi, lo


def raw_blocks(key, purpose, first_block, n_blocks):
    """(n_blocks, 4) uint64: the words of blocks first_block .. first_block + n_blocks - 1 (the block index wraps mod 2^64)"""
    with np.errstate(over="ignore"):
        j = np.uint64(first_block) + np.arange(n_blocks, dtype=np.uint64)
        c = [j, np.full(n_blocks, purpose, dtype=np.uint64), np.zeros(n_blocks, np.uint64), np.zeros(n_blocks, np.uint64)]
        k0, k1 = np.uint64(key[0]), np.uint64(key[1])
        for _ in range(10):
            hi0, lo0 = mulhilo(M0, c[0])
            hi1, lo1 = mulhilo(M1, c[2])
            c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
            k0, k1 = k0 + np.uint64(W0), k1 + np.uint64(W1)
    return np.stack(c, axis=1)


def unit_open(w):
    return ((w >> np.uint64(12)).astype(np.float64) + 0.5) * 2.0 ** -52


def standard_normal(n, key, purpose=0):
    """the first n values of the stream"""
    w = raw_blocks(key, purpose, 0, (n + 3) // 4)
    z = np.empty((w.shape[0], 4))
    for a in (0, 2):
        r = np.sqrt(-2.0 * np.log(unit_open(w[:, a])))
        theta = 2.0 * np.pi * unit_open(w[:, a + 1])
        z[:, a], z[:, a + 1] = r * np.cos(theta), r * np.sin(theta)
    return z.reshape(-1)[:n]


def statistics(z, other_room, other_purpose):
    """{name: (value, bound)} of n draws of one stream, every bound at five standard deviations of the statistic under the
    normal law (the Kolmogorov-Smirnov distance at 1.95 / sqrt(n), its 0.1 % point); other_room, other_purpose: n draws each of
    the stream of another key and of another purpose under the same key"""
    import torch

    n = len(z)
    corr = lambda a, b: float(np.mean(a * b))      # noqa: E731
    var = float(np.var(z))
    c = z - np.mean(z)
    cdf = 0.5 * (1.0 + torch.erf(torch.from_numpy(np.sort(z) / np.sqrt(2.0))).numpy())
    steps = np.arange(n + 1) / n
    ks = float(max(np.max(steps[1:] - cdf), np.max(cdf - steps[:-1])))
    five = 5.0 / np.sqrt(n)
    return {"mean": (abs(float(np.mean(z))), five), "variance": (abs(var - 1.0), 5.0 * np.sqrt(2.0 / n)),
            "lag 1": (abs(corr(z[:-1], z[1:])), five), "lag 2": (abs(corr(z[:-2], z[2:])), five),
            "cross-room": (abs(corr(z, other_room)), five), "cross-purpose": (abs(corr(z, other_purpose)), five),
            "kurtosis": (abs(float(np.mean(c ** 4)) / var ** 2 - 3.0), 5.0 * np.sqrt(96.0 / n)), "ks": (ks, 1.95 / np.sqrt(n))}


def numpy_philox_block(key, purpose, j):
    """the same block from numpy.random.Philox, which increments its 256-bit counter before it generates"""
    c = ((j + (purpose << 64)) - 1) % (1 << 256)
    counter = np.array([(c >> (64 * i)) & ((1 << 64) - 1) for i in range(4)], dtype=np.uint64)
    return np.random.Philox(key=np.array(key, dtype=np.uint64), counter=counter).random_raw(4)
