"""``measure_rt60_batch()``, ``edc_batch()`` and ``absorption_for_rt60()``: the decay curve and the reverberation time of many impulse
responses on the device (``oiva_decay_*``, csrc/kernels_decay.hip), and the search for the wall absorption that gives a wanted one
-- how an ``rt60_list`` entry of the reference's sweep (``"0.3": {"max_order": 17, "absorption": 0.35}``) is made without
pyroomacoustics.

The contract is the algorithm as DESIGN.md 3.14 states it, in float64.  For one response ``h[0..L-1]``:

* ``E[n] = sum_{k >= n} h[k]^2`` (Schroeder integral), summed in an order that is a function of ``(n, L)`` alone: a response has the
  same bits alone, in any batch and at any place in it;
* ``theta_a = E[0] * 10 ** (-start_db / 10)``, ``theta_b = E[0] * 10 ** (-(start_db + decay_db) / 10)``; ``i_a``, ``i_b`` = the
  smallest n with ``E[n] <= theta_a``, ``theta_b`` (-1: none; both -1 for an all-zero response).  Energies are compared, never decibels;
* ``rt60_cross = (60 / decay_db) * (i_b - i_a) / fs`` -- the crossing-time convention of pyroomacoustics' ``measure_rt60``, whose
  source is not part of the reference: as for the room simulation, parity with it is **not pinned**;
* ``rt60_fit = -60 / (m * fs)``, m the least-squares slope in dB per sample of ``D[n] = 10 log10(E[n] / E[0])`` over
  ``[i_a, i_b)``; NaN when the window has fewer than 2 samples.  The device returns ``sum D`` and ``sum n D`` over the window;
  ``sum n`` and ``sum n^2`` follow from the two indices (``window_sums``).

Both estimates are NaN when ``i_b == -1`` (the response ends before ``-(start_db + decay_db)`` dB) or ``E[0] == 0``.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from . import batch as _batch
from .overiva import get_device

TILE = 1024                    # samples per tile of the kernel's walk (kDecayTile)
MAX_LENGTH = 1 << 24           # samples of one response
MAX_RESPONSES = 1 << 22        # responses of one handle


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _number(name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
        raise ValueError(f"{name} must be a finite number, got {v!r}")
    return float(v)


def _check_params(fs, decay_db, start_db):
    fs, decay_db, start_db = _number("fs", fs), _number("decay_db", decay_db), _number("start_db", start_db)
    if fs <= 0:
        raise ValueError(f"fs must be > 0, got {fs}")
    if decay_db <= 0:
        raise ValueError(f"decay_db must be > 0, got {decay_db}")
    if start_db < 0:
        raise ValueError(f"start_db must be >= 0, got {start_db}")
    return fs, decay_db, start_db


def _check_rirs(rirs):
    """-> (list of float64 C-contiguous (n_b, L_b) arrays, the leading shape of each, whether ``rirs`` was a sequence)"""
    ragged = isinstance(rirs, (list, tuple))
    items = [np.asarray(a) for a in rirs] if ragged else [np.asarray(rirs)]
    if not items:
        raise ValueError("rirs is empty")
    out, shapes = [], []
    for b, a in enumerate(items):
        name = f"rirs[{b}]" if ragged else "rirs"
        if a.dtype.kind not in "fiu":
            raise ValueError(f"{name} must be real, got dtype {a.dtype}")
        if a.ndim < 1 or a.size == 0:
            raise ValueError(f"{name} is empty (shape {a.shape}): responses are (..., L) with L >= 1")
        if a.shape[-1] > MAX_LENGTH:
            raise ValueError(f"{name}: responses of {a.shape[-1]} samples (at most 2**24)")
        a = np.ascontiguousarray(a, dtype=np.float64)
        if not np.all(np.isfinite(a)):
            raise ValueError(f"{name} holds non-finite samples")
        shapes.append(a.shape[:-1])
        out.append(a.reshape(-1, a.shape[-1]))
    if sum(a.shape[0] for a in out) > MAX_RESPONSES:
        raise ValueError(f"rirs holds more than {MAX_RESPONSES} responses")
    return out, shapes, ragged


def _refuse_sharding(what):
    from . import sharded

    if sharded.active_group() is not None:
        raise ValueError(f"{what} does not run under enable_bin_sharding(): disable bin sharding for batched calls")


def window_sums(i_a, i_b):
    """(N, sum n, sum n^2) over n in [i_a, i_b), exact Python integers, from the two indices alone"""
    i_a, i_b = int(i_a), int(i_b)
    square_pyramid = lambda k: k * (k + 1) * (2 * k + 1) // 6      # noqa: E731  (sum of n^2 over 0..k)
    return i_b - i_a, (i_b - i_a) * (i_a + i_b - 1) // 2, square_pyramid(i_b - 1) - square_pyramid(i_a - 1)


def estimates(fs, decay_db, e0, i_a, i_b, sum_d, sum_nd):
    """(rt60_cross, rt60_fit) from what the device returns.  The slope is ``(sum nD - nbar sum D) / Sxx`` with
    ``nbar = sum n / N = (i_a + i_b - 1) / 2`` and ``Sxx = sum n^2 - (sum n)^2 / N = N (N^2 - 1) / 12`` of ``window_sums``."""
    e0, sum_d, sum_nd = (np.asarray(v, dtype=np.float64) for v in (e0, sum_d, sum_nd))
    i_a, i_b = np.asarray(i_a, dtype=np.int64), np.asarray(i_b, dtype=np.int64)
    N = (i_b - i_a).astype(np.float64)
    good = (i_b >= 0) & (i_a >= 0) & (e0 > 0)
    cross = np.where(good, (60.0 / decay_db) * N / fs, np.nan)
    fit_ok = good & (N >= 2)
    Nf = np.where(fit_ok, N, 2.0)
    nbar = (i_a + i_b - 1) / 2.0
    with np.errstate(divide="ignore", invalid="ignore"):
        m = (sum_nd - nbar * sum_d) / (Nf * (Nf * Nf - 1.0) / 12.0)
        fit = np.where(fit_ok, -60.0 / (m * fs), np.nan)
    return cross, fit


def truncation_horizon(room_dim, max_order, c=343.0):
    """
    The time before which an image-source response of order ``max_order`` is complete: ``(max_order - 2) / (c sqrt(sum_i 1 / L_i^2))``
    seconds, 0 for orders below 2.  Every image the order leaves out arrives later than this, so a crossing beyond it rests on a
    truncated tail.  Host only; ``room_dim`` is (3,) or (batch, 3), the result a float or (batch,).  Nothing is flagged or refused
    on it: it is for the caller to judge.
    """
    dim = np.asarray(room_dim, dtype=np.float64)
    if dim.ndim not in (1, 2) or dim.shape[-1] != 3 or not np.all(np.isfinite(dim)) or np.any(dim <= 0):
        raise ValueError(f"room_dim must be (3,) or (batch, 3) finite sides > 0, got {room_dim!r}")
    if not _is_int(max_order) or max_order < 0:
        raise ValueError(f"max_order must be an integer >= 0, got {max_order!r}")
    c = _number("c", c)
    if c <= 0:
        raise ValueError(f"c must be > 0, got {c}")
    t = max(0, int(max_order) - 2) / (c * np.sqrt(np.sum(1.0 / dim ** 2, axis=-1)))
    return float(t) if dim.ndim == 1 else t


class DecayBatch(_lib.Handle):
    """the staged form: one handle (``oiva_decay``) = responses of fixed lengths packed one after the other.  ``set`` copies packed
    samples in, ``set_dev`` borrows a device address, ``set_room`` borrows a ``RoomBatch``'s responses where they lie; ``run``
    measures; ``get`` / ``get_curves`` read the results."""

    _destroy = "oiva_decay_destroy"

    def __init__(self, lengths, device=None, stream=None):
        lengths = list(lengths)
        if not 1 <= len(lengths) <= MAX_RESPONSES:
            raise ValueError(f"lengths must name 1..{MAX_RESPONSES} responses, got {len(lengths)}")
        for i, n in enumerate(lengths):
            if not _is_int(n) or not 1 <= n <= MAX_LENGTH:
                raise ValueError(f"lengths[{i}] must be an integer in 1..2**24, got {n!r}")
        self.lengths = [int(n) for n in lengths]
        self.total = sum(self.lengths)
        self.lib = _lib.load()
        self.device = get_device() if device is None else int(device)
        self.params = None
        h = C.c_void_p()
        table = (C.c_int * len(self.lengths))(*self.lengths)
        _lib.check(self.lib.oiva_decay_create(C.byref(h), self.device, len(self.lengths), table, C.c_void_p(stream) if stream else None))
        self.h = h

    def info(self):
        """what ``last_batch_info()`` reports after a run on this handle"""
        out = {"algorithm": "decay", "precision": "float64", "batched": len(self.lengths), "sharded": False}
        if len(set(self.lengths)) > 1:
            out.update(ragged=True, lengths=list(self.lengths))
        else:
            out["n_samples"] = self.lengths[0]
        if self.params:
            out.update(self.params)
        return out

    def set(self, packed):
        packed = np.ascontiguousarray(packed, dtype=np.float64).ravel()
        if packed.size != self.total:
            raise ValueError(f"packed holds {packed.size} samples, the handle's responses {self.total}")
        _lib.check(self.lib.oiva_decay_set_host(self.h, _lib.ptr(packed)))
        return self

    def set_dev(self, dev_ptr):
        """the packed responses at a device address: borrowed, must stay valid until ``run``"""
        _lib.check(self.lib.oiva_decay_set_dev(self.h, C.c_void_p(int(dev_ptr))))
        return self

    def set_room(self, room):
        """the impulse responses of a ``RoomBatch`` (after ``compute_rir``) where they lie; nothing is copied"""
        _lib.check(self.lib.oiva_decay_set_room(self.h, room.h))
        return self

    def run(self, fs, start_db=5.0, decay_db=20.0, keep_curve=False):
        _lib.check(self.lib.oiva_decay_run(self.h, float(fs), float(start_db), float(decay_db), int(bool(keep_curve))))
        self.params = {"fs": float(fs), "start_db": float(start_db), "decay_db": float(decay_db), "curves": bool(keep_curve)}
        return self

    def get(self):
        """{"e0", "i_a", "i_b", "sum_d", "sum_nd"}: one value per response"""
        n = len(self.lengths)
        e0, sd, snd = np.empty(n), np.empty(n), np.empty(n)
        ia, ib = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        _lib.check(self.lib.oiva_decay_get(self.h, _lib.ptr(e0), _lib.ptr(ia), _lib.ptr(ib), _lib.ptr(sd), _lib.ptr(snd)))
        return {"e0": e0, "i_a": ia, "i_b": ib, "sum_d": sd, "sum_nd": snd}

    def get_curves(self):
        """the list of curves, one float64 array per response (``run(..., keep_curve=True)``)"""
        flat = np.empty(self.total)
        _lib.check(self.lib.oiva_decay_get_curve(self.h, _lib.ptr(flat)))
        off = np.concatenate([[0], np.cumsum(self.lengths)])
        return [flat[off[i]:off[i + 1]] for i in range(len(self.lengths))]

    def ms(self):
        """device ms of the kernel of the last ``run``"""
        ms = C.c_float()
        _lib.check(self.lib.oiva_decay_ms(self.h, C.byref(ms)))
        return ms.value

    def rt60(self):
        """(rt60_cross, rt60_fit, i_a, i_b) of the last run, one value per response"""
        r = self.get()
        cross, fit = estimates(self.params["fs"], self.params["decay_db"], r["e0"], r["i_a"], r["i_b"], r["sum_d"], r["sum_nd"])
        return cross, fit, r["i_a"], r["i_b"]


def _run(items, fs, start_db, decay_db, keep_curve):
    lengths = [a.shape[1] for a in items for _ in range(a.shape[0])]
    packed = items[0].ravel() if len(items) == 1 else np.concatenate([a.ravel() for a in items])
    with DecayBatch(lengths) as d:
        d.set(packed).run(fs, start_db, decay_db, keep_curve)
        _batch._info = d.info()
        return d.rt60(), (d.get_curves() if keep_curve else None)


def _split(flat, items, shapes, ragged):
    """one value (or curve) per response -> shaped like the leading axes of every input"""
    out, at = [], 0
    for a, shape in zip(items, shapes):
        part = flat[at:at + a.shape[0]]
        at += a.shape[0]
        out.append(np.asarray(part).reshape(shape + np.shape(part)[1:]) if not isinstance(part, list)
                   else np.stack(part).reshape(shape + (a.shape[1],)))
    return out if ragged else out[0]


def measure_rt60_batch(rirs, fs, decay_db=20.0, start_db=5.0, return_curves=False, return_indices=False):
    """
    Reverberation time of many impulse responses at once, measured on the device (the algorithm of DESIGN.md 3.14; parity with
    pyroomacoustics' ``measure_rt60`` is not pinned).

    Parameters
    ----------
    rirs: real, finite: an array (..., L), or a sequence of arrays (..., L_b) whose lengths may differ; 1 <= L <= 2**24
    fs: sampling rate, > 0
    decay_db, start_db: the line is fitted between ``-start_db`` and ``-(start_db + decay_db)`` dB of the decay curve and
        extrapolated to 60 dB; ``decay_db > 0``, ``start_db >= 0``
    return_curves: also return the decay curves ``E[n]``, shaped like ``rirs``
    return_indices: also return ``(i_a, i_b)``, the first samples at or below the two thresholds (-1: none)

    Returns
    -------
    ``rt60_cross, rt60_fit`` in seconds, shaped like the leading axes of ``rirs`` (lists of such arrays for a sequence), then the
    curves and the index pair when asked for.  Both estimates are NaN for a response that ends before ``-(start_db + decay_db)`` dB
    and for an all-zero one; ``rt60_fit`` also when fewer than 2 samples lie between the thresholds.
    """
    items, shapes, ragged = _check_rirs(rirs)
    fs, decay_db, start_db = _check_params(fs, decay_db, start_db)
    _refuse_sharding("measure_rt60_batch")
    (cross, fit, ia, ib), curves = _run(items, fs, start_db, decay_db, bool(return_curves))
    out = [_split(cross, items, shapes, ragged), _split(fit, items, shapes, ragged)]
    if return_curves:
        out.append(_split(curves, items, shapes, ragged))
    if return_indices:
        out.append((_split(ia, items, shapes, ragged), _split(ib, items, shapes, ragged)))
    return tuple(out)


def edc_batch(rirs):
    """the decay curves ``E[n] = sum_{k >= n} h[k]^2`` alone, shaped like ``rirs`` (``measure_rt60_batch`` tells the forms)"""
    items, shapes, ragged = _check_rirs(rirs)
    _refuse_sharding("edc_batch")
    _, curves = _run(items, 1.0, 5.0, 20.0, True)
    return _split(curves, items, shapes, ragged)


def _room_median(values):
    """nanmedian over a room's pairs; NaN when every pair is NaN"""
    v = np.asarray(values).ravel()
    v = v[~np.isnan(v)]
    return float(np.median(v)) if v.size else math.nan


def absorption_for_rt60(room_dim, sources, mics, rt60, max_order, fs=16000, c=343.0, rir_length=None, estimator="fit", decay_db=20.0,
                        start_db=5.0, rtol=0.01, max_steps=24, bracket=(0.01, 0.99)):
    """
    The uniform wall absorption that gives every room a wanted reverberation time, by bisection on the device: how an
    ``rt60_list`` entry ``{"max_order": ..., "absorption": ...}`` is made.

    ONE ``RoomBatch`` serves the whole search.  A step sets every room's current absorption, recomputes the impulse responses,
    measures them where they lie and brings back only the (n_sources, n_mics) estimates; a room's measured value is the
    ``nanmedian`` over its pairs (all NaN: the room has failed).  Step 1 evaluates the bracket's lower end, step 2 its upper end; a
    room whose target lies outside its two end values stops there, not converged, with the nearer end.  Then plain bisection on
    the midpoint, until ``|measured - target| <= rtol * target`` (per room) or ``max_steps`` steps.  A room's sequence of absorptions
    depends on its own measurements alone: its result does not depend on the batch.

    Parameters
    ----------
    room_dim, sources, mics, fs, c, max_order, rir_length: as ``rir_batch()``
    rt60: the target in seconds, > 0: a scalar or (batch,)
    estimator: "fit" (``rt60_fit``) or "cross" (``rt60_cross``); decay_db, start_db: as ``measure_rt60_batch()``
    rtol: > 0; max_steps: an integer >= 2; bracket: ``(low, high)`` with ``0 < low < high < 1``

    Returns
    -------
    ``absorption (batch,)``, the measured ``rt60 (batch,)`` at it, ``converged (batch,)`` bool and ``steps (batch,)``, the
    evaluations each room used.  ``truncation_horizon(room_dim, max_order, c)`` tells how far the responses can be trusted.
    """
    from . import room as _room

    room_dim, sources, mics, _, fs, c, max_order, rir_length = _room._check_geometry(room_dim, sources, mics, fs, max_order, 0.5, c,
                                                                                     rir_length)
    B = room_dim.shape[0]
    target = _room._real_array("rt60", rt60)
    if target.ndim == 0:
        target = np.full(B, float(target))
    if target.shape != (B,):
        raise ValueError(f"rt60 must be a scalar or (batch,) = ({B},), got shape {target.shape}")
    if np.any(target <= 0):
        raise ValueError("rt60 must be > 0")
    if estimator not in ("fit", "cross"):
        raise ValueError(f"estimator must be 'fit' or 'cross', got {estimator!r}")
    _, decay_db, start_db = _check_params(fs, decay_db, start_db)
    rtol = _number("rtol", rtol)
    if rtol <= 0:
        raise ValueError(f"rtol must be > 0, got {rtol}")
    if not _is_int(max_steps) or max_steps < 2:
        raise ValueError(f"max_steps must be an integer >= 2, got {max_steps!r}")
    try:
        low, high = (_number("bracket", v) for v in bracket)
    except TypeError:
        raise ValueError(f"bracket must be (low, high), got {bracket!r}") from None
    if not 0 < low < high < 1:
        raise ValueError(f"bracket must be (low, high) with 0 < low < high < 1, got {bracket!r}")
    _refuse_sharding("absorption_for_rt60")

    current = np.full(B, low)
    with _room.RoomBatch(room_dim, sources, mics, fs=fs, max_order=max_order, absorption=current, c=c, rir_length=rir_length) as rb:
        def measure():
            if rb.rir_lengths is not None:
                rb.set_absorption(current)
            rb.compute_rir()
            cross, fit = rb.measure_rt60(decay_db, start_db)
            return np.array([_room_median(v) for v in (fit if estimator == "fit" else cross)])

        def close(r):
            return np.abs(r - target) <= rtol * target       # (NaN: False)

        r_low = measure()
        current[:] = high
        r_high = measure()
        steps = np.full(B, 2)
        absorption, measured = np.full(B, low), r_low.copy()
        converged = close(r_low)
        hit_high = ~converged & close(r_high)
        absorption[hit_high], measured[hit_high] = high, r_high[hit_high]
        converged |= hit_high
        between = (np.minimum(r_low, r_high) <= target) & (target <= np.maximum(r_low, r_high))       # (NaN at an end: False)
        active = ~converged & between
        outside = ~converged & ~between
        nearer_high = outside & (np.abs(r_high - target) < np.abs(r_low - target))
        absorption[nearer_high], measured[nearer_high] = high, r_high[nearer_high]
        a_lo, a_hi, above_lo = np.full(B, low), np.full(B, high), r_low > target
        for _ in range(2, int(max_steps)):
            if not active.any():
                break
            mid = 0.5 * (a_lo + a_hi)
            current[:] = np.where(active, mid, absorption)
            r = measure()
            steps[active] += 1
            absorption[active], measured[active] = mid[active], r[active]
            done = active & close(r)
            failed = active & np.isnan(r)
            converged |= done
            same_side = (r > target) == above_lo
            a_lo = np.where(active & same_side, mid, a_lo)
            a_hi = np.where(active & ~same_side, mid, a_hi)
            active &= ~done & ~failed
        info = rb.info()
    _batch._info = dict(info, algorithm="decay", search="absorption_for_rt60", steps=int(steps.max()))
    return absorption, measured, converged, steps
