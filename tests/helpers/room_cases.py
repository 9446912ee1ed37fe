"""The cases of the room simulation tests: seeded geometries, every position drawn from L * U(0.15, 0.85) per axis.  A case is
admissible only if its tie margin min | |phi| - 1/2 | is >= MIN_MARGIN (asserted in tests/test_room_host.py, on the CPU): at a tie
host and device may legitimately round k differently.  The oracle of a case runs once per process and is shared."""
import functools

import numpy as np

import room_oracle as ro

MIN_MARGIN = 1e-6
SMALL = (3.0, 4.0, 2.6)
MID = (5.0, 4.0, 2.7)
BIG = (10.0, 7.5, 3.0)

# name, room_dim, S, M, max_order, fs, absorption, rir_length, seed
CASES = (
    ("order0_1x1", SMALL, 1, 1, 0, 8000, 0.35, None, 1),                 # one image
    ("order1_3x2", SMALL, 3, 2, 1, 8000, 0.35, None, 2),                 # 7 images
    ("order3_2x5", MID, 2, 5, 3, 8000, 0.35, None, 3),                   # 63 images: one short of 64
    ("order4_3x2", SMALL, 3, 2, 4, 8000, 0.2, None, 4),                  # 129 images: two chunks of 64 plus one
    ("order6_2x5", MID, 2, 5, 6, 8000, 0.35, None, 5),                   # 377 images: more than one table of 256
    ("order3_16k", BIG, 3, 2, 3, 16000, 0.35, None, 6),
    ("six_walls", MID, 1, 1, 4, 8000, (0.1, 0.25, 0.4, 0.55, 0.7, 0.85), None, 7),
    ("hard_walls", SMALL, 1, 1, 1, 8000, 0.0, None, 8),
    ("cut_300", MID, 3, 2, 4, 8000, 0.35, 300, 9),                       # a fixed length that cuts windows off
    ("near_5cm", SMALL, 1, 1, 1, 8000, 0.35, None, 10),                  # a source 5 cm from the microphone: k < H
)


def case_id(case):
    return case[0]


def geometry(room_dim, S, M, seed):
    rng = np.random.default_rng(seed)
    L = np.asarray(room_dim, dtype=float)
    return L * rng.uniform(0.15, 0.85, (S, 3)), L * rng.uniform(0.15, 0.85, (M, 3))


def make_case(case):
    """-> dict(room_dim (3,), sources (S, 3), mics (M, 3), absorption6 (6,), fs, max_order, rir_length)"""
    name, room_dim, S, M, order, fs, absorption, rir_length, seed = case
    sources, mics = geometry(room_dim, S, M, seed)
    if name.startswith("near"):
        sources = mics[:1] + np.array([0.03, 0.04, 0.0])
    return dict(room_dim=np.asarray(room_dim, dtype=float), sources=sources, mics=mics, absorption=ro.absorption6(absorption), fs=fs,
                max_order=order, rir_length=rir_length)


@functools.lru_cache(maxsize=None)
def oracle_run(case):
    """-> (rir (S, M, L), tie margin) of the case, read-only"""
    g = make_case(case)
    h, margin = ro.rir(g["room_dim"], g["sources"], g["mics"], g["absorption"], g["fs"], 343.0, g["max_order"], g["rir_length"])
    h.setflags(write=False)
    return h, margin


# ---- a batch of three rooms that differ in size, geometry, absorption and signal length (S = 3, M = 2, order 3, fs 8000) ----
TRIO = (
    dict(room_dim=SMALL, absorption=(0.3,) * 6, seed=21, n=700),
    dict(room_dim=MID, absorption=(0.1, 0.2, 0.3, 0.4, 0.5, 0.6), seed=22, n=1),
    dict(room_dim=(4.0, 6.0, 3.1), absorption=(0.5,) * 6, seed=23, n=3001),
)
TRIO_S, TRIO_M, TRIO_ORDER, TRIO_FS = 3, 2, 3, 8000


@functools.lru_cache(maxsize=None)
def trio():
    """-> the three rooms as dicts(room_dim, sources, mics, absorption, signals (S, n), noise_seed) with the oracle's rir and
    premix, read-only"""
    out = []
    for spec in TRIO:
        sources, mics = geometry(spec["room_dim"], TRIO_S, TRIO_M, spec["seed"])
        rng = np.random.default_rng(spec["seed"] + 100)
        signals = rng.standard_normal((TRIO_S, spec["n"]))
        h, margin = ro.rir(spec["room_dim"], sources, mics, spec["absorption"], TRIO_FS, 343.0, TRIO_ORDER)
        prem = ro.premix(signals, h)
        for a in (h, prem, signals):
            a.setflags(write=False)
        out.append(dict(room_dim=np.asarray(spec["room_dim"], dtype=float), sources=sources, mics=mics,
                        absorption=np.asarray(spec["absorption"], dtype=float), signals=signals, rir=h, premix=prem, margin=margin,
                        seed=spec["seed"]))
    return tuple(out)


def trio_args(rooms):
    """the keyword arguments of rir_batch / simulate_batch for some rooms of the trio"""
    return dict(room_dim=np.stack([r["room_dim"] for r in rooms]), sources=np.stack([r["sources"] for r in rooms]),
                mics=np.stack([r["mics"] for r in rooms]), absorption=np.stack([r["absorption"] for r in rooms]), fs=TRIO_FS,
                max_order=TRIO_ORDER)
