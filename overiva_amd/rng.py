"""``standard_normal_batch()``: seeded standard normals drawn on the device (``oiva_rng_*``, csrc/kernels_rng.hip), the generator
behind ``simulate_batch(seed=...)`` and ``sweep_batch(seed=...)``.

The stream is counter-based, a pure function of (key, purpose, index): Philox-4x64-10 under the key
``(k0, k1)`` on the counter ``(j, purpose, 0, 0)`` gives block j, four 64-bit words -- the words
``numpy.random.Philox(key=[k0, k1], counter=(j, purpose, 0, 0) - 1).random_raw(4)`` returns.  A word w becomes
``u = ((w >> 12) + 0.5) * 2**-52`` in (0, 1); words 0, 1 give ``r cos(2 pi u1)`` and ``r sin(2 pi u1)`` with
``r = sqrt(-2 ln u0)``, words 2, 3 the next two values.  Element n of a stream is value ``n % 4`` of block ``n // 4``: a stream is a
prefix of every longer draw with its key and purpose, and a room's draws do not depend on the batch, its place in it or the
grouping.  The normals are not ``numpy.random``'s (its transform is another one); only the raw words are numpy's, bit for bit.

``purpose`` is 0 for sensor noise and 1 for the filler row of the sweep; other values are the caller's.
"""
import ctypes as C

import numpy as np

from . import _lib
from .overiva import get_device

NOISE, FILLER = 0, 1
MAX_STREAMS = 65535
MAX_COUNT = 1 << 40
MAX_RAW_BLOCKS = 1 << 20
_U64 = 1 << 64


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _word(name, v):
    if not _is_int(v) or not 0 <= int(v) < _U64:
        raise ValueError(f"{name} must be an integer in 0..2**64 - 1, got {v!r}")
    return int(v)


def check_seed(seed, B):
    """-> the keys of B streams, two uint64 arrays (B,): an int s names the streams (s, 0), (s, 1), ..., (s, B - 1) -- a stream
    then depends on its index; a sequence of B ints names (seed[b], 0), one seed per stream, independent of the batch"""
    if _is_int(seed):
        return np.full(B, _word("seed", seed), dtype=np.uint64), np.arange(B, dtype=np.uint64)
    if isinstance(seed, (bool, np.bool_, float, np.floating, str, bytes)) or seed is None:
        raise ValueError(f"seed must be an integer in 0..2**64 - 1 or a sequence of {B} such integers, got {seed!r}")
    if isinstance(seed, np.ndarray):
        if seed.ndim != 1 or seed.dtype.kind not in "iu":
            raise ValueError(f"seed must be a 1-D sequence of integers, got shape {seed.shape} and dtype {seed.dtype}")
        items = seed.tolist()
    else:
        try:
            items = list(seed)
        except TypeError:
            raise ValueError(f"seed must be an integer or a sequence of {B} integers, got {seed!r}") from None
    if len(items) != B:
        raise ValueError(f"seed holds {len(items)} values for {B} streams: one per stream")
    keys = [_word(f"seed[{b}]", v) for b, v in enumerate(items)]
    return np.array(keys, dtype=np.uint64), np.zeros(B, dtype=np.uint64)


def _check_sizes(sizes):
    if isinstance(sizes, (str, bytes)) or np.ndim(sizes) != 1:
        raise ValueError(f"sizes must be a 1-D sequence of stream lengths, got {sizes!r}")
    sizes = list(sizes)
    if not 1 <= len(sizes) <= MAX_STREAMS:
        raise ValueError(f"sizes must name 1..{MAX_STREAMS} streams, got {len(sizes)}")
    for i, n in enumerate(sizes):
        if not _is_int(n) or not 1 <= n <= MAX_COUNT:
            raise ValueError(f"sizes[{i}] must be an integer in 1..2**40, got {n!r}")
    if sum(int(n) for n in sizes) > MAX_COUNT:
        raise ValueError("sizes name more than 2**40 values")
    return [int(n) for n in sizes]


class DeviceNormal(_lib.Handle):
    """the staged form: one handle (``oiva_rng``) = streams of fixed lengths packed one after the other on the device.
    ``fill(key0, key1, purpose)`` draws every stream under its own key; ``get()`` reads them, ``ptr`` is where they lie."""

    _destroy = "oiva_rng_destroy"

    def __init__(self, sizes, device=None, stream=None):
        self.sizes = _check_sizes(sizes)
        self.lib = _lib.load()
        self.device = get_device() if device is None else int(device)
        h = C.c_void_p()
        counts = (C.c_longlong * len(self.sizes))(*self.sizes)
        _lib.check(self.lib.oiva_rng_create(C.byref(h), self.device, len(self.sizes), counts, C.c_void_p(stream) if stream else None))
        self.h = h

    def fill(self, key0, key1, purpose=NOISE):
        """stream i under the key ``(key0[i], key1[i])``"""
        purpose = _word("purpose", purpose)
        k0, k1 = (np.ascontiguousarray([_word("key", v) for v in k], dtype=np.uint64) for k in (key0, key1))
        if k0.shape != (len(self.sizes),) or k1.shape != k0.shape:
            raise ValueError(f"key0 and key1 must hold {len(self.sizes)} words each")
        _lib.check(self.lib.oiva_rng_fill(self.h, _lib.ptr(k0), _lib.ptr(k1), purpose))
        return self

    def fill_ms(self):
        """device ms of the kernel of the last ``fill``"""
        ms = C.c_float()
        _lib.check(self.lib.oiva_rng_fill_ms(self.h, C.byref(ms)))
        return ms.value

    def get(self):
        """the list of float64 arrays, one per stream"""
        flat = np.empty(sum(self.sizes))
        _lib.check(self.lib.oiva_rng_get(self.h, _lib.ptr(flat)))
        off = np.concatenate([[0], np.cumsum(self.sizes)])
        return [flat[off[i]:off[i + 1]] for i in range(len(self.sizes))]

    @property
    def ptr(self):
        """device address of the packed values, valid until the next ``fill`` or ``close``"""
        dev = C.c_void_p()
        _lib.check(self.lib.oiva_rng_ptr(self.h, C.byref(dev)))
        return dev.value


def standard_normal_batch(sizes, seed, purpose=NOISE):
    """
    Seeded standard normals, drawn on the device: one float64 array of ``sizes[i]`` values per stream.

    Parameters
    ----------
    sizes: a sequence of stream lengths, each >= 1
    seed: an int s in 0..2**64 - 1 -- stream i has the key (s, i), so it depends on its index -- or a sequence of one such int
        per stream -- stream i has the key (seed[i], 0) and does not depend on the other streams
    purpose: 0 (sensor noise), 1 (the filler row) or any other integer in 0..2**64 - 1: another purpose, another stream

    Returns
    -------
    the list of arrays.  A stream of n values is the first n of every longer draw with the same key and purpose.
    """
    sizes = _check_sizes(sizes)
    k0, k1 = check_seed(seed, len(sizes))
    purpose = _word("purpose", purpose)
    with DeviceNormal(sizes) as gen:
        return gen.fill(k0, k1, purpose).get()


def raw_blocks(key, purpose, first_block, n_blocks, device=None):
    """test hook: the raw words (n_blocks, 4) uint64 of blocks ``first_block ..`` of the stream under ``key = (k0, k1)``"""
    k0, k1 = (_word("key", v) for v in key)
    purpose, first_block = _word("purpose", purpose), _word("first_block", first_block)
    if not _is_int(n_blocks) or not 1 <= n_blocks <= MAX_RAW_BLOCKS:
        raise ValueError(f"n_blocks must be an integer in 1..{MAX_RAW_BLOCKS}, got {n_blocks!r}")
    words = np.empty((int(n_blocks), 4), dtype=np.uint64)
    lib = _lib.load()
    _lib.check(lib.oiva_rng_raw(get_device() if device is None else int(device), k0, k1, purpose, first_block, int(n_blocks),
                                _lib.ptr(words)))
    return words
