"""Inputs of the decay tests (tests/test_decay_host.py, tests/test_decay_gpu.py): the decaying-noise family of
tests/helpers/decay_oracle.py at the lengths where the kernel changes its path, and the small rooms of the room-handle and search
tests."""
import numpy as np

import decay_oracle as do

FS = 8000
TILE = 1024                       # the kernel's tile (overiva_amd.acoustics.TILE; the host test holds the two together)
RTS = (0.05, 0.12, 0.3)
SHORT = (1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
LONG = (4097, 9000)               # long enough for windows of >= 32 samples at every rt


def curve_inputs():
    """every (length, rt) of SHORT in one list -- the middle rt with the lengths reversed, so that multi-tile responses lie at even
    and at odd offsets of the packed batch (16-byte loads and the 8-byte path) -- and one response with 300 trailing zeros"""
    out = []
    for i, rt in enumerate(RTS):
        out += [do.family(L, rt, FS) for L in (SHORT[::-1] if i == 1 else SHORT)]
    tail = do.family(1500, 0.05, FS)
    tail[-300:] = 0.0
    return out + [tail]


def long_inputs():
    return [do.family(L, rt, FS) for L in LONG for rt in RTS]


def offsets(items):
    return np.concatenate([[0], np.cumsum([len(h) for h in items])[:-1]])


# 2 rooms of 2 sources x 3 microphones: RoomBatch.measure_rt60 and set_absorption
HANDLE_ROOMS = dict(
    room_dim=np.array([[5.0, 4.0, 3.0], [6.2, 4.6, 2.7]]),
    sources=np.array([[[1.0, 1.1, 1.2], [3.5, 2.0, 1.5]], [[1.3, 1.1, 1.2], [4.5, 3.0, 1.4]]]),
    mics=np.array([[[2.0, 3.0, 1.25], [2.2, 3.1, 1.3], [2.4, 2.9, 1.2]], [[2.0, 3.0, 1.25], [2.2, 3.1, 1.3], [2.5, 3.3, 1.1]]]),
    fs=FS, max_order=6, rir_length=1500)

# 3 rooms of different sizes, 2 x 2 pairs: absorption_for_rt60.  At order 8 every response is cut long before -25 dB (the horizon
# of room 0 is 38 ms), so the measured time follows the truncation as much as the walls: between absorptions 0.12 and 0.4 it GROWS
# with the absorption in all three rooms (measured with room_oracle + decay_oracle: 0.113 -> 0.133, 0.168 -> 0.183, 0.086 -> 0.114 s),
# and it falls again above 0.6.  The search only needs the target between the two end values; the bracket is chosen for that.
SEARCH_ROOMS = dict(
    room_dim=np.array([[5.0, 4.0, 3.0], [6.0, 5.0, 2.5], [4.0, 3.5, 2.8]]),
    sources=np.array([[[1.0, 1.1, 1.2], [3.5, 2.0, 1.5]], [[1.3, 1.1, 1.2], [4.5, 3.0, 1.4]], [[1.0, 1.1, 1.2], [3.0, 2.0, 1.5]]]),
    mics=np.array([[[2.0, 3.0, 1.25], [2.2, 3.1, 1.3]], [[2.0, 3.0, 1.25], [2.2, 3.1, 1.3]], [[2.0, 2.9, 1.25], [2.2, 2.7, 1.3]]]),
    fs=FS, max_order=8, rir_length=2000)
SEARCH_ABSORPTION = 0.3
SEARCH_BRACKET = (0.12, 0.4)


def room_median(h, **kw):
    """the restatement's value of one room (S, M, L): the median of rt60_fit over its pairs, and whether every pair is finite"""
    fit = np.array([do.measure(h[s, m], FS, **kw)["rt60_fit"] for s in range(h.shape[0]) for m in range(h.shape[1])])
    return float(np.median(fit)), bool(np.all(np.isfinite(fit)))
