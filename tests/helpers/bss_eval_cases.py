"""Inputs shared by tests/test_bss_eval_host.py and tests/test_bss_eval_gpu.py: the cases, their generators and the yardstick.

References are seeded white noise ("white"), or the same through the AR(1) filter 1 / (1 - 0.9 z^-1) ("ar").  Estimates are a 5-tap
random mixing of the references (diagonal tap 0 boosted by 2, every other tap 0.3 N(0,1)) plus 0.05 N(0,1) noise.

The yardstick of a room is the restatement's own spread on it, in dB, max over the entries of the SDR, SIR and SAR matrices: the
larger of ``delta`` (how far a 1e-13 relative perturbation of all inputs moves the time-domain form) and the distance between
the restatement's two forms.
"""
import numpy as np

import bss_eval_oracle as bso

SEED = 23
# (kind, B, N, n, Lf)
CASES = [("white", 3, 1, 300, 8), ("white", 2, 2, 700, 33), ("ar", 2, 3, 1500, 70), ("ar", 1, 5, 1200, 20), ("ar", 1, 2, 4000, 512),
         # N = 4, 6, 7, 8 (8: 72 vectors in the quadratic forms, 8 right-hand sides per substitution); n of exactly one segment of
         # 2048, of one sample more and of whole 128-sample tiles; Lf = 64 (a small system is one block), 257 (a single lag in the
         # second 256), N Lf = 512 and 192 (whole blocks)
         ("ar", 1, 4, 2048, 16), ("white", 2, 6, 2049, 11), ("ar", 1, 7, 1000, 10), ("ar", 1, 8, 900, 9), ("white", 1, 8, 1100, 64),
         ("white", 1, 2, 1500, 257), ("ar", 1, 3, 700, 64), ("ar", 1, 4, 640, 128), ("white", 1, 1, 128, 64)]
ADMIT_DB = 1e-6          # a case is admitted only if 10 x yardstick <= this
FACTOR = 10.0


def case_id(case):
    kind, B, N, n, Lf = case
    return f"{kind}-B{B}-N{N}-n{n}-Lf{Lf}"


def make_refs(kind, N, n, seed):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((N, n))
    if kind == "ar":
        for u in range(1, n):
            s[:, u] += 0.9 * s[:, u - 1]
    return s


def make_room(kind, N, n, seed):
    """(ref, est), each (N, n) float64"""
    ref = make_refs(kind, N, n, seed)
    rng = np.random.default_rng(seed + 5000)
    taps = 0.3 * rng.standard_normal((N, N, 5))
    taps[np.arange(N), np.arange(N), 0] += 2.0
    est = np.zeros((N, n))
    for k in range(N):
        for i in range(N):
            est[k] += np.convolve(ref[i], taps[k, i])[:n]
    est += 0.05 * rng.standard_normal((N, n))
    return ref, est


def make_case(case):
    """(ref (B, N, n), est (B, N, n)); room b is seeded SEED + 100 b"""
    kind, B, N, n, Lf = case
    rooms = [make_room(kind, N, n, SEED + 100 * b) for b in range(B)]
    return np.stack([r for r, _ in rooms]), np.stack([e for _, e in rooms])


def perturbed(a, seed):
    return a * (1.0 + 1e-13 * np.random.default_rng(seed).standard_normal(a.shape))


def db_distance(A, B):
    """max over the three matrices and their entries of |a - b| in dB; entries that are +inf in both count as equal"""
    worst = 0.0
    for a, b in zip(A, B):
        a, b = np.asarray(a), np.asarray(b)
        both_inf = np.isinf(a) & np.isinf(b) & (np.sign(a) == np.sign(b))
        d = np.where(both_inf, 0.0, np.abs(np.where(both_inf, 0.0, a) - np.where(both_inf, 0.0, b)))
        worst = max(worst, float(np.max(d)))
    return worst


_ORACLE = {}


def oracle_run(case):
    """per room of the case, computed once: the time-domain form's (sdr, sir, sar), the Gram form's G, D, E, delta, the distance
    between the forms and the yardstick"""
    if case not in _ORACLE:
        kind, B, N, n, Lf = case
        ref, est = make_case(case)
        rooms = []
        for b in range(B):
            td = bso.bss_eval_td(ref[b], est[b], Lf)
            G, D, E = bso.gram_direct(ref[b], est[b], Lf)
            gram = bso.criteria_from_gram(G, D, E, N, Lf)
            td2 = bso.bss_eval_td(perturbed(ref[b], SEED + 1000 + b), perturbed(est[b], SEED + 2000 + b), Lf)
            delta, forms = db_distance(td2, td), db_distance(gram, td)
            for a in td + (G, D, E):
                a.setflags(write=False)
            rooms.append(dict(td=td, gram=gram, G=G, D=D, E=E, delta=delta, forms=forms, yardstick=max(delta, forms)))
        ref.setflags(write=False)
        est.setflags(write=False)
        _ORACLE[case] = dict(ref=ref, est=est, rooms=rooms)
    return _ORACLE[case]
