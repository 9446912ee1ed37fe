"""``rir_batch()`` and ``simulate_batch()``: shoebox rooms by the image-source method for B rooms per set of launches, in float64 on
the device (``oiva_room_*``, csrc/kernels_room.hip): impulse responses, premix (every source convolved with its response at every
microphone) and the mix-down of the reference's Monte-Carlo sweep.

The reference simulates every room with ``pra.ShoeBox(...)``, ``room.compute_rir()`` and ``room.simulate(return_premix=True)``
(``overiva_sim.py:140-163``), then scales and mixes (``:166-198``).  pyroomacoustics is a third-party package whose source is not
part of the reference, so **the contract is the algorithm as DESIGN.md 3.11 states it**, checked against a NumPy restatement
written from that statement (tests/helpers/room_oracle.py); parity with ``pra.ShoeBox`` -- bit or numeric, of any version -- is
not pinned.

Per (room, source, microphone): the images ``(nx, ny, nz)`` with ``|nx| + |ny| + |nz| <= max_order`` in the order nx, ny, nz
ascending, each adding 81 taps of a Hann-windowed sinc at its delay, so an impulse response carries a fixed lag of 40 samples.
Every sample has one owner that adds the taps in that order: a room's bits do not depend on B, on its place in the batch or on
the other rooms.  ``noise`` is the caller's, or, with ``seed``, drawn on the device from the seeded stream of DESIGN.md 3.13
(``overiva_amd/rng.py``): room b's ``(n_out_b, n_mics)`` noise is its purpose-0 stream, read row by row.
"""
import ctypes as C

import numpy as np

from . import _lib, sharded
from . import batch as _batch
from . import rng as _rng
from .overiva import get_device

MAX_ORDER = 32
MAX_SOURCES = 16
MAX_MICS = 32
MAX_RIR = 65536
FDL = 81
STAGES = ("k_max", "rir", "convolve", "mix")


def image_count(max_order):
    """images with ``|nx| + |ny| + |nz| <= max_order``"""
    N = int(max_order)
    return (2 * N + 1) * (2 * N * N + 2 * N + 3) // 3


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _real_array(name, a):
    a = np.asarray(a)
    if a.dtype.kind not in "fiu":
        raise ValueError(f"{name} must be real, got dtype {a.dtype}")
    a = np.require(a, dtype=np.float64, requirements="C")          # (keeps a scalar 0-d)
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{name} holds non-finite values")
    return a


def _check_geometry(room_dim, sources, mics, fs, max_order, absorption, c, rir_length):
    room_dim = _real_array("room_dim", room_dim)
    sources = _real_array("sources", sources)
    mics = _real_array("mics", mics)
    if room_dim.ndim != 2 or room_dim.shape[1] != 3 or room_dim.shape[0] < 1:
        raise ValueError(f"room_dim must have shape (batch, 3), got {room_dim.shape}")
    B = room_dim.shape[0]
    if sources.ndim != 3 or sources.shape[2] != 3:
        raise ValueError(f"sources must have shape (batch, n_sources, 3), got {sources.shape}")
    if mics.ndim != 3 or mics.shape[2] != 3:
        raise ValueError(f"mics must have shape (batch, n_mics, 3), got {mics.shape}")
    if sources.shape[0] != B or mics.shape[0] != B:
        raise ValueError(f"room_dim holds {B} rooms, sources {sources.shape[0]}, mics {mics.shape[0]}: the batch must agree")
    S, M = sources.shape[1], mics.shape[1]
    if not 1 <= S <= MAX_SOURCES:
        raise ValueError(f"simulate_batch runs on 1..{MAX_SOURCES} sources, got {S}")
    if not 1 <= M <= MAX_MICS:
        raise ValueError(f"simulate_batch runs on 1..{MAX_MICS} microphones, got {M}")
    if np.any(room_dim <= 0):
        raise ValueError("room_dim must be > 0")
    for name, pos in (("source", sources), ("microphone", mics)):
        inside = (pos > 0) & (pos < room_dim[:, None, :])
        if not np.all(inside):
            b, i = np.argwhere(~inside.all(axis=2))[0]
            raise ValueError(f"room {b}: {name} {i} at {pos[b, i].tolist()} is on or outside a wall of the box {room_dim[b].tolist()}")
    same = np.all(sources[:, :, None, :] == mics[:, None, :, :], axis=3)
    if np.any(same):
        b, s, m = np.argwhere(same)[0]
        raise ValueError(f"room {b}: source {s} is at zero distance from microphone {m}")
    for name, v in (("fs", fs), ("c", c)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v <= 0:
            raise ValueError(f"{name} must be a finite number > 0, got {v!r}")
    if not _is_int(max_order) or not 0 <= max_order <= MAX_ORDER:
        raise ValueError(f"max_order must be an integer in 0..{MAX_ORDER}, got {max_order!r}")
    a = _check_absorption(absorption, B)
    if rir_length is not None and (not _is_int(rir_length) or rir_length < 1):
        raise ValueError(f"rir_length must be None or an integer >= 1, got {rir_length!r}")
    if rir_length is not None and rir_length > MAX_RIR:
        raise ValueError(f"rir_length must be at most {MAX_RIR}, got {rir_length}")
    return room_dim, sources, mics, a, float(fs), float(c), int(max_order), rir_length and int(rir_length)


def _check_absorption(absorption, B):
    """a scalar, (batch,) or (batch, 6) -> float64 C-contiguous (batch, 6)"""
    a = _real_array("absorption", absorption)
    if a.ndim == 0:
        a = np.full((B, 6), float(a))
    elif a.shape == (B,):
        a = np.repeat(a[:, None], 6, axis=1)
    elif a.shape != (B, 6):
        raise ValueError(f"absorption must be a scalar, (batch,) or (batch, 6), got shape {a.shape}")
    if np.any(a < 0) or np.any(a >= 1):
        raise ValueError("absorption must be in [0, 1)")
    return np.ascontiguousarray(a)


def _check_signals(signals, B, S):
    """-> (list of B float64 C-contiguous (S, n_b) arrays, ragged)"""
    ragged = isinstance(signals, (list, tuple))
    if ragged:
        rooms = [np.asarray(a) for a in signals]
        for b, a in enumerate(rooms):
            if a.ndim != 2:
                raise ValueError(f"signals[{b}] has shape {a.shape}: every room must be (n_sources, n_samples)")
    else:
        arr = np.asarray(signals)
        if arr.ndim != 3:
            raise ValueError("signals must have shape (batch, n_sources, n_samples), or be a sequence of (n_sources, n_samples_b) "
                             f"arrays; got shape {arr.shape}")
        rooms = list(arr)
    if len(rooms) != B:
        raise ValueError(f"signals holds {len(rooms)} rooms, room_dim {B}: the batch must agree")
    out = []
    for b, a in enumerate(rooms):
        if a.dtype.kind not in "fiu":
            raise ValueError(f"signals must be real (float32, float64 or integer), got dtype {a.dtype} in room {b}")
        if a.shape[0] != S:
            raise ValueError(f"signals: room {b} has {a.shape[0]} sources, sources has {S}: the source count must agree")
        if a.shape[1] < 1:
            raise ValueError(f"signals: room {b} has no samples")
        a = np.ascontiguousarray(a, dtype=np.float64)
        if not np.all(np.isfinite(a)):
            raise ValueError(f"signals: room {b} holds non-finite samples")
        out.append(a)
    return out, ragged


def _check_mix(B, S, M, ragged, n_targets, sinr, snr, ref_mic, sources_var, noise):
    """-> (K, sinr, snr, ref_mic, sources_var (K,), noise: None or a list of B float64 (n_b', M) arrays)"""
    if not _is_int(n_targets) or not 1 <= n_targets <= S:
        raise ValueError(f"n_targets must be an integer in 1..{S}, got {n_targets!r}")
    K = int(n_targets)
    for name, v in (("sinr", sinr), ("snr", snr)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or np.isnan(v):
            raise ValueError(f"{name} must be a number (dB), got {v!r}")
    if K == S and np.isfinite(sinr):
        raise ValueError(f"n_targets == n_sources == {S} leaves no interferer to reach sinr = {sinr}: pass sinr=np.inf")
    if not _is_int(ref_mic) or not 0 <= ref_mic < M:
        raise ValueError(f"ref_mic must be in 0..{M - 1}, got {ref_mic!r}")
    var = np.ones(K) if sources_var is None else _real_array("sources_var", sources_var)
    if var.shape != (K,) or np.any(var < 0):
        raise ValueError(f"sources_var must hold n_targets = {K} values >= 0")
    if noise is not None:
        if isinstance(noise, (list, tuple)) != ragged:
            raise ValueError("noise must be an array for array signals and a sequence for a sequence of signals")
        rooms = [np.asarray(a) for a in noise] if ragged else np.asarray(noise)
        if not ragged and rooms.ndim != 3:
            raise ValueError(f"noise must have shape (batch, n_out, n_mics), got {rooms.shape}")
        if len(rooms) != B:
            raise ValueError(f"noise holds {len(rooms)} rooms, room_dim {B}: the batch must agree")
        noise = []
        for b, a in enumerate(rooms):
            if a.ndim != 2 or a.shape[1] != M:
                raise ValueError(f"noise: room {b} has shape {a.shape}: every room must be (n_out, n_mics = {M})")
            noise.append(_real_array("noise", a))
    return K, float(sinr), float(snr), int(ref_mic), np.ascontiguousarray(var, dtype=np.float64), noise


def _refuse_sharding(what):
    if sharded.active_group() is not None:
        raise ValueError(f"{what} does not run under enable_bin_sharding(): disable bin sharding for batched calls")


class RoomBatch(_lib.Handle):
    """one handle = B shoebox rooms of S sources and M microphones on one GPU (``oiva_room``).

    Stages: ``compute_rir`` (k_max, then the impulse responses), ``set_signals``, then per room group ``convolve`` and ``mix``;
    ``get_rir`` / ``get_premix`` / ``get_mix`` read what the stages left.  ``simulate`` walks the groups (the premix of all rooms
    may not fit the device at once; ``max_group`` asks for groups of at most that many rooms)."""

    _destroy = "oiva_room_destroy"

    def __init__(self, room_dim, sources, mics, fs=16000, max_order=17, absorption=0.35, c=343.0, rir_length=None, device=None,
                 stream=None):
        room_dim, sources, mics, a6, fs, c, max_order, rir_length = _check_geometry(room_dim, sources, mics, fs, max_order, absorption,
                                                                                    c, rir_length)
        self.lib = _lib.load()
        self.B, self.S, self.M = room_dim.shape[0], sources.shape[1], mics.shape[1]
        self.fs, self.c, self.max_order, self.fixed_length = fs, c, max_order, rir_length
        self.images = image_count(max_order)
        self.device = get_device() if device is None else int(device)
        self.rir_lengths, self.lengths, self.group, self.K = None, None, None, None
        self.noise_source = None                 # of the last mix: "host", "device" or None (no noise)
        h = C.c_void_p()
        _lib.check(self.lib.oiva_room_create(C.byref(h), self.device, self.B, self.S, self.M, fs, c, max_order, _lib.ptr(room_dim),
                                             _lib.ptr(sources), _lib.ptr(mics), _lib.ptr(a6), rir_length or 0,
                                             C.c_void_p(stream) if stream else None))
        self.h = h

    def info(self):
        """what ``last_batch_info()`` reports after a run on this handle"""
        out = {"algorithm": "simulate", "precision": "float64", "batched": self.B, "sharded": False, "n_sources": self.S,
               "n_mics": self.M, "max_order": self.max_order, "images": self.images,
               "rir_lengths": None if self.rir_lengths is None else list(self.rir_lengths), "rooms_per_group": self.group,
               "noise": self.noise_source}
        if self.lengths is not None:
            if len(set(self.lengths)) > 1:
                out.update(ragged=True, lengths=list(self.lengths))
            else:
                out["n_samples"] = self.lengths[0]
        return out

    def compute_rir(self):
        """k_max of every room, then every impulse response; -> the lengths L_b"""
        _lib.check(self.lib.oiva_room_compute_rir(self.h))
        L = (C.c_int * self.B)()
        n = C.c_int()
        _lib.check(self.lib.oiva_room_rir_lengths(self.h, L, C.byref(n)))
        self.rir_lengths = [int(v) for v in L]
        assert n.value == self.images
        return self.rir_lengths

    def get_rir(self):
        """the list of B arrays (S, M, L_b)"""
        sizes = [self.S * self.M * L for L in self.rir_lengths]
        flat = np.empty(sum(sizes))
        _lib.check(self.lib.oiva_room_get_rir(self.h, _lib.ptr(flat)))
        off = np.concatenate([[0], np.cumsum(sizes)])
        return [flat[off[b]:off[b + 1]].reshape(self.S, self.M, L) for b, L in enumerate(self.rir_lengths)]

    def set_absorption(self, absorption):
        """new wall absorptions -- a scalar, (B,) or (B, 6), as the constructor takes them: the impulse responses become stale and
        ``compute_rir`` may run again on this handle (k_max, the lengths and the device buffers stay: they do not depend on the
        absorption).  Any convolved or mixed group is dropped; ``convolve`` raises until ``compute_rir`` has run"""
        a6 = _check_absorption(absorption, self.B)
        _lib.check(self.lib.oiva_decay_room_set_absorption(self.h, _lib.ptr(a6)))

    def measure_rt60(self, decay_db=20.0, start_db=5.0):
        """``(rt60_cross, rt60_fit)`` of every impulse response, measured where it lies (``measure_rt60_batch()``, DESIGN.md
        3.14): two lists of B arrays (S, M).  Only the estimates' ingredients leave the device"""
        from . import acoustics

        fs, decay_db, start_db = acoustics._check_params(self.fs, decay_db, start_db)
        if self.rir_lengths is None:
            raise RuntimeError("compute_rir has not run")
        pairs = self.S * self.M
        with acoustics.DecayBatch([L for L in self.rir_lengths for _ in range(pairs)], device=self.device) as d:
            cross, fit, _, _ = d.set_room(self).run(fs, start_db, decay_db).rt60()
            _batch._info = dict(d.info(), n_rooms=self.B, n_sources=self.S, n_mics=self.M)
        shape = (self.B, self.S, self.M)
        return list(cross.reshape(shape)), list(fit.reshape(shape))

    def set_signals(self, signals, max_group=0):
        """signals: B arrays (S, n_b); sizes the room groups"""
        if len(signals) != self.B or any(np.ndim(a) != 2 or np.shape(a)[0] != self.S for a in signals):
            raise ValueError(f"signals must be {self.B} arrays of shapes ({self.S}, n_b)")
        self.lengths = [int(np.shape(a)[1]) for a in signals]
        packed = np.concatenate([np.ascontiguousarray(a, dtype=np.float64).ravel() for a in signals])
        ns = (C.c_int * self.B)(*self.lengths)
        _lib.check(self.lib.oiva_room_set_signals(self.h, ns, _lib.ptr(packed), int(max_group)))
        g = C.c_int()
        _lib.check(self.lib.oiva_room_groups(self.h, C.byref(g)))
        self.group = g.value
        self.out_lengths = [n + L - 1 for n, L in zip(self.lengths, self.rir_lengths)]
        return self.group

    def group_rooms(self, g0):
        return range(g0, min(self.B, g0 + self.group))

    def convolve(self, g0=0):
        """the premix of the group that starts at room g0"""
        _lib.check(self.lib.oiva_room_convolve(self.h, int(g0)))

    def get_premix(self, g0=0):
        """the group's premix: a list of (S, M, n_out_b) arrays"""
        sizes = [self.S * self.M * self.out_lengths[b] for b in self.group_rooms(g0)]
        flat = np.empty(sum(sizes))
        _lib.check(self.lib.oiva_room_get_premix(self.h, int(g0), _lib.ptr(flat)))
        off = np.concatenate([[0], np.cumsum(sizes)])
        return [flat[off[i]:off[i + 1]].reshape(self.S, self.M, self.out_lengths[b]) for i, b in enumerate(self.group_rooms(g0))]

    def mix(self, g0=0, n_targets=1, sinr=10.0, snr=60.0, ref_mic=0, sources_var=None, noise=None, seed_keys=None):
        """the mix-down of the group that starts at room g0 (convolved); noise: None or the group's (n_out_b, M) arrays;
        seed_keys: None or (key0, key1), one key per room of the group: the noise is drawn on the device, room by room from the
        purpose-0 stream of its key (``overiva_amd/rng.py``), and nothing is copied from the host"""
        rooms = self.group_rooms(g0)
        if seed_keys is not None and noise is not None:
            raise ValueError("noise and seed_keys exclude each other: the noise is the caller's or the device's")
        packed = None
        if noise is not None:
            if len(noise) != len(rooms) or any(np.shape(a) != (self.out_lengths[b], self.M) for a, b in zip(noise, rooms)):
                want = [(self.out_lengths[b], self.M) for b in rooms]
                raise ValueError(f"noise must be {len(rooms)} arrays of shapes {want}, got {[np.shape(a) for a in noise]}")
            packed = np.concatenate([np.ascontiguousarray(a, dtype=np.float64).ravel() for a in noise])
        var = None if sources_var is None else np.ascontiguousarray(sources_var, dtype=np.float64)
        if var is not None and var.shape != (int(n_targets),):
            raise ValueError(f"sources_var must hold n_targets = {n_targets} values")
        if seed_keys is not None:
            k0, k1 = (np.ascontiguousarray(k, dtype=np.uint64) for k in seed_keys)
            if k0.shape != (len(rooms),) or k1.shape != (len(rooms),):
                raise ValueError(f"seed_keys must be two sequences of {len(rooms)} words, one key per room of the group")
            _lib.check(self.lib.oiva_rng_room_mix(self.h, int(g0), int(n_targets), float(sinr), float(snr), int(ref_mic),
                                                  None if var is None else _lib.ptr(var), _lib.ptr(k0), _lib.ptr(k1)))
        else:
            _lib.check(self.lib.oiva_room_mix(self.h, int(g0), int(n_targets), float(sinr), float(snr), int(ref_mic),
                                              None if var is None else _lib.ptr(var), None if packed is None else _lib.ptr(packed)))
        self.K = int(n_targets)
        self.noise_source = "device" if seed_keys is not None else None if noise is None else "host"

    def get_mix(self, g0=0):
        """the group's mix, a list of (n_out_b, M) arrays, and ref, a list of (K + 1, n_out_b, M) arrays"""
        rooms = self.group_rooms(g0)
        sizes = [self.M * self.out_lengths[b] for b in rooms]
        mix, ref = np.empty(sum(sizes)), np.empty((self.K + 1) * sum(sizes))
        _lib.check(self.lib.oiva_room_get_mix(self.h, int(g0), _lib.ptr(mix), _lib.ptr(ref)))
        off = np.concatenate([[0], np.cumsum(sizes)])
        mixes = [mix[off[i]:off[i + 1]].reshape(self.out_lengths[b], self.M) for i, b in enumerate(rooms)]
        refs = [ref[(self.K + 1) * off[i]:(self.K + 1) * off[i + 1]].reshape(self.K + 1, self.out_lengths[b], self.M)
                for i, b in enumerate(rooms)]
        return mixes, refs

    def simulate(self, mix_args=None, noise=None, seed_keys=None):
        """every group through ``convolve`` (and ``mix`` with ``mix_args``): the premix of every room, or (mix, ref) of every room;
        noise and seed_keys ((key0, key1), one key per room of the batch) as ``mix`` takes them for a group"""
        premix, mixes, refs = [], [], []
        for g0 in range(0, self.B, self.group):
            self.convolve(g0)
            if mix_args is None:
                premix += self.get_premix(g0)
                continue
            rooms = self.group_rooms(g0)
            self.mix(g0, noise=None if noise is None else [noise[b] for b in rooms],
                     seed_keys=None if seed_keys is None else tuple(k[rooms.start:rooms.stop] for k in seed_keys), **mix_args)
            m, r = self.get_mix(g0)
            mixes += m
            refs += r
        return premix if mix_args is None else (mixes, refs)

    def time_stages(self, n, n_targets=1, sinr=10.0, snr=60.0, ref_mic=0):
        """n full runs with events around every stage: {stage: ms per run}"""
        ms = (C.c_float * len(STAGES))()
        _lib.check(self.lib.oiva_room_time_stages(self.h, int(n), int(n_targets), float(sinr), float(snr), int(ref_mic), ms))
        return dict(zip(STAGES, list(ms)))


def rir_batch(room_dim, sources, mics, fs=16000, max_order=17, absorption=0.35, c=343.0, rir_length=None):
    """
    Image-source impulse responses of B shoebox rooms at once (the algorithm of DESIGN.md 3.11; parity with pyroomacoustics is
    not pinned).

    Parameters
    ----------
    room_dim: (batch, 3) box sizes in metres; sources: (batch, n_sources, 3), 1..16 sources; mics: (batch, n_mics, 3), 1..32
        microphones; every position strictly inside its box, no source on a microphone
    fs, c: sampling rate and speed of sound, one value for the batch
    max_order: int, 0..32: the images ``|nx| + |ny| + |nz| <= max_order``
    absorption: energy absorption in [0, 1): a scalar, (batch,), or (batch, 6) for the walls x=0, x=Lx, y=0, y=Ly, z=0, z=Lz
    rir_length: None (room b gets ``k_max,b + 81`` samples) or one length for every room, at most 65536 (later taps are dropped)

    Returns
    -------
    the list of B float64 arrays (n_sources, n_mics, L_b), or one (batch, n_sources, n_mics, rir_length) array for an integer
    ``rir_length``.  Every response carries a fixed lag of 40 samples.
    """
    geometry = _check_geometry(room_dim, sources, mics, fs, max_order, absorption, c, rir_length)
    _refuse_sharding("rir_batch")
    with RoomBatch(*geometry[:3], fs=geometry[4], max_order=geometry[6], absorption=geometry[3], c=geometry[5],
                   rir_length=geometry[7]) as rb:
        rb.compute_rir()
        _batch._info = rb.info()
        rirs = rb.get_rir()
    return np.stack(rirs) if rir_length is not None else rirs


def simulate_batch(signals, room_dim, sources, mics, fs=16000, max_order=17, absorption=0.35, c=343.0, rir_length=None,
                   n_targets=None, sinr=10.0, snr=60.0, ref_mic=0, sources_var=None, noise=None, seed=None, max_group=0):
    """
    Simulate B shoebox rooms at once: impulse responses as ``rir_batch()``, every source convolved with its response at every
    microphone and, with ``n_targets``, the scaling and mix-down of the reference's sweep (``overiva_sim.py:166-198``).  The
    algorithm is DESIGN.md 3.11; parity with pyroomacoustics is not pinned.

    Parameters
    ----------
    signals: (batch, n_sources, n_samples) real, or a sequence of B arrays (n_sources, n_samples_b) whose lengths may differ
    room_dim, sources, mics, fs, max_order, absorption, c, rir_length: as ``rir_batch()``
    n_targets: None for the premix, or K in 1..n_sources: the first K sources are targets, the others interferers
    sinr, snr: dB; every source is first given unit variance at ``ref_mic``, target s then the variance ``sources_var[s]``
        (default ones); ``sigma_n^2 = 10^(-snr/10) sum(var)`` and the interferers share
        ``max(0, 10^(-sinr/10) sum(var) - sigma_n^2)`` equally.  ``n_targets == n_sources`` needs ``sinr=np.inf``
    noise: None (no noise is added) or unit-variance noise of the caller's, (batch, n_out, n_mics) or a sequence of
        (n_out_b, n_mics) arrays with ``n_out_b = n_samples_b + L_b - 1`` (``rir_batch()`` or ``rir_length`` tell L_b beforehand)
    seed: None, or the seed of unit-variance noise drawn on the device (``standard_normal_batch()``; needs
        ``n_targets`` and ``noise=None``): room b's noise is the row-major (n_out_b, n_mics) array of its purpose-0 stream.  An
        int s in 0..2**64 - 1 gives room b the key (s, b): its noise then **depends on the room's index in the batch**.  A
        sequence of B such ints gives room b the key (seed[b], 0) -- one seed per run, as the reference's argument lists carry
        them -- and a room's noise does not depend on the batch.  Nothing but the seeds crosses the bus for the noise
    max_group: 0, or the most rooms that go through the stages together, as ``RoomBatch.set_signals``; a room's bits do not
        depend on it

    Returns
    -------
    premix: (batch, n_sources, n_mics, n_out) when ``signals`` is an array and the rooms come out equally long, else the list
    of B arrays (n_sources, n_mics, n_out_b) -- the full linear convolutions.  With ``n_targets``: ``mix`` (n_out, n_mics) and
    ``ref`` (n_targets + 1, n_out, n_mics) per room -- the target images and the background -- stacked or listed likewise.
    """
    geometry = _check_geometry(room_dim, sources, mics, fs, max_order, absorption, c, rir_length)
    B, S, M = geometry[0].shape[0], geometry[1].shape[1], geometry[2].shape[1]
    sig, ragged = _check_signals(signals, B, S)
    mix_args = seed_keys = None
    if n_targets is not None:
        K, sinr, snr, ref_mic, var, noise = _check_mix(B, S, M, ragged, n_targets, sinr, snr, ref_mic, sources_var, noise)
        mix_args = dict(n_targets=K, sinr=sinr, snr=snr, ref_mic=ref_mic, sources_var=var)
    if seed is not None:
        if n_targets is None:
            raise ValueError("seed names the noise of the mix-down: it needs n_targets")
        if noise is not None:
            raise ValueError("seed and noise exclude each other: the noise is the caller's (noise) or drawn on the device (seed)")
        seed_keys = _rng.check_seed(seed, B)
    if not _is_int(max_group) or max_group < 0:
        raise ValueError(f"max_group must be an integer >= 0, got {max_group!r}")
    _refuse_sharding("simulate_batch")
    with RoomBatch(*geometry[:3], fs=geometry[4], max_order=geometry[6], absorption=geometry[3], c=geometry[5],
                   rir_length=geometry[7]) as rb:
        rb.compute_rir()
        rb.set_signals(sig, max_group)
        if mix_args is not None and noise is not None:
            for b, a in enumerate(noise):
                if a.shape[0] != rb.out_lengths[b]:
                    raise ValueError(f"noise: room {b} has {a.shape[0]} samples, its output has {rb.out_lengths[b]} "
                                     f"(n_samples + rir_length - 1 = {rb.lengths[b]} + {rb.rir_lengths[b]} - 1)")
        out = rb.simulate(mix_args, noise, seed_keys)
        _batch._info = rb.info()
    stack = not ragged and len(set(rb.out_lengths)) == 1
    if mix_args is None:
        return np.stack(out) if stack else out
    return (np.stack(out[0]), np.stack(out[1])) if stack else out
