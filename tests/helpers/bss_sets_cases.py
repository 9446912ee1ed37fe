"""Inputs shared by tests/test_bss_eval_sets_host.py and tests/test_bss_eval_sets_gpu.py: several sets of estimates against one set
of references.

The references are ``bss_eval_cases.make_refs``.  Set e of a room is the recipe of ``bss_eval_cases.make_room`` -- a 5-tap random
mixing of the references (diagonal tap 0 boosted by 2, every other tap 0.3 N(0,1)) plus 0.05 N(0,1) noise -- drawn from its own
seed, so the sets differ while the references are shared.
"""
import numpy as np

import bss_eval_cases as cases

# (kind, B, N, n, Lf) of test "sets equal single calls"
CASES = [("white", 2, 2, 700, 33),
         ("ar", 1, 3, 2049, 70),          # a second segment of one sample; N Lf = 210 across four 64-blocks
         ("white", 1, 8, 900, 9),         # 8 right-hand sides and 72 vectors
         ("white", 1, 2, 1500, 257),      # the second 256-lag workgroup with one live lag
         ("ar", 1, 4, 640, 128),          # whole blocks
         ("white", 1, 1, 300, 8)]         # SIR +inf
SEED = 41


def make_set(ref, seed):
    """one (N, n) set of estimates of the (N, n) references"""
    N, n = ref.shape
    rng = np.random.default_rng(seed + 5000)
    taps = 0.3 * rng.standard_normal((N, N, 5))
    taps[np.arange(N), np.arange(N), 0] += 2.0
    est = np.zeros((N, n))
    for k in range(N):
        for i in range(N):
            est[k] += np.convolve(ref[i], taps[k, i])[:n]
    est += 0.05 * rng.standard_normal((N, n))
    return est


def make_sets(ref, E, seed):
    """(E, N, n): set e is seeded seed + 17 e"""
    return np.stack([make_set(ref, seed + 17 * e) for e in range(E)])


def make_rooms(kind, N, lens, E, seed=SEED):
    """(refs: B arrays (N, n_b), sets: B arrays (E, N, n_b)); room b is seeded seed + 100 b"""
    refs = [cases.make_refs(kind, N, n, seed + 100 * b) for b, n in enumerate(lens)]
    return refs, [make_sets(r, E, seed + 100 * b + 1) for b, r in enumerate(refs)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
