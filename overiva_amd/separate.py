"""``separate_batch()``: audio in, audio out for B rooms, everything between the audio upload and the audio download on the device.

The reference's Monte-Carlo sweep (``overiva_sim.py:206-207, 298-315``) takes one simulated room after the other through
audio -> STFT -> separation -> iSTFT.  The batched solvers (``batch.py``) start and end at STFT tensors on the host; this module
puts the transform next to them: ``BatchSTFT`` (``oiva_bstft``, csrc/kernels_bstft.hip) transforms all rooms in one set of
launches and writes X on the device in the layout the matching plan borrows -- (B, T, F, M) for rooms of one length, packed
(sum T_b, F, M) for rooms of different lengths -- and ``BatchPlan.demix_device`` leaves Y there for the synthesis.

Framing convention and arithmetic are ``stft.py``'s, room by room: ``hop`` new samples per frame behind ``frame - hop`` old ones,
zero state at the start of every room, ``n_frames = n_samples // hop``, ``n_frames * hop`` output samples; float32 on the device.
"""
import ctypes as C

import numpy as np

from . import _lib, sharded
from . import batch as _batch
from . import ip2 as _ip2
from . import iss as _iss
from . import ive as _ive
from . import pca_batch as _pca_batch
from . import stft as _stft
from .batch import DeviceBatch
from .five import run_five          # (the package's attribute `five` is the function)
from .overiva import get_device

MAX_CHANNELS = _batch.MAX_CHANNELS
PHASES = ("upload", "framing", "fft_r2c", "transpose_in", "transpose_out", "fft_c2r", "overlap_add", "download")


def _windows(frame, hop, win_a, win_s):
    """the reference drivers' choice (overiva_oneshot.py:157-158): Hann and its least-squares synthesis window when frames overlap"""
    if win_a is None and hop < frame:
        win_a = _stft.hann(frame)
    if win_s is None and win_a is not None:
        win_s = _stft.compute_synthesis_window(win_a, hop)
    out = []
    for name, w in (("win_a", win_a), ("win_s", win_s)):
        if w is not None:
            w = np.ascontiguousarray(w, dtype=np.float32)
            if w.shape != (frame,):
                raise ValueError(f"{name} has shape {w.shape}: window length must equal the frame length {frame}")
        out.append(w)
    return out


def _check_stft_args(n_samples, M, frame, hop):
    for name, v in (("frame", frame), ("hop", hop), ("M", M)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    if frame < 2 or frame % 2:
        raise ValueError(f"frame must be even and >= 2, got {frame}")
    if not 1 <= hop <= frame:
        raise ValueError(f"hop must be in 1..frame = {frame}, got {hop}")
    if not 1 <= M <= MAX_CHANNELS:
        raise ValueError(f"the batched path runs on 1..{MAX_CHANNELS} channels, got {M}")
    if not n_samples:
        raise ValueError("at least one room is needed")
    for b, n in enumerate(n_samples):
        if n < hop:
            raise ValueError(f"room {b} has {n} samples: every room must be at least one hop ({hop}) long")
        if n * M >= 2 ** 31 or (n // hop) * M * (frame + 2) >= 2 ** 31:
            raise ValueError(f"room {b} is too large")


class BatchSTFT(_lib.Handle):
    """one handle = B rooms of ``n_samples[b]`` x M samples, one (frame, hop, windows) configuration, on one GPU (``oiva_bstft``).

    ``n_samples``: an int together with ``B`` (rooms of one length: X comes in the dense (B, T, F, M) layout of ``BatchPlan``), or
    a list of B ints (X packed (sum T_b, F, M), the layout of ``RaggedBatchPlan``)."""

    _destroy = "oiva_bstft_destroy"

    def __init__(self, n_samples, M, frame, hop=None, win_a=None, win_s=None, device=None, B=None, stream=None):
        self.dense = isinstance(n_samples, (int, np.integer)) and not isinstance(n_samples, bool)
        if self.dense:
            if B is None or isinstance(B, bool) or not isinstance(B, (int, np.integer)) or B < 1:
                raise ValueError("an int n_samples needs B >= 1, the number of rooms")
            lens = [int(n_samples)] * int(B)
        else:
            if B is not None and B != len(n_samples):
                raise ValueError(f"B = {B} but n_samples lists {len(n_samples)} rooms")
            lens = [int(n) for n in n_samples]
        hop = frame // 2 if hop is None else hop
        _check_stft_args(lens, M, frame, hop)
        wa, ws = _windows(frame, hop, win_a, win_s)
        self.lib = _lib.load()
        self.n_samples, self.B, self.M, self.frame, self.hop = lens, len(lens), int(M), int(frame), int(hop)
        self.device = get_device() if device is None else int(device)
        h = C.c_void_p()
        ns = (C.c_int * self.B)(*lens)
        _lib.check(self.lib.oiva_bstft_create(C.byref(h), self.device, self.B, ns, self.M, self.frame, self.hop,
                                              None if wa is None else _lib.ptr(wa), None if ws is None else _lib.ptr(ws),
                                              C.c_void_p(stream) if stream else None))
        self.h = h
        fr, f = (C.c_int * self.B)(), C.c_int()
        _lib.check(self.lib.oiva_bstft_shape(self.h, fr, C.byref(f)))
        self.frames, self.n_freq = list(fr), f.value
        self.sample_offsets = np.concatenate([[0], np.cumsum(lens)]).astype(int)
        self.out_offsets = np.concatenate([[0], np.cumsum(self.frames)]).astype(int) * self.hop

    def _pack(self, x):
        if isinstance(x, (list, tuple)):
            if len(x) != self.B or any(np.shape(a) != (n, self.M) for a, n in zip(x, self.n_samples)):
                raise ValueError(f"x must be {self.B} arrays of shapes (n_b, {self.M}), n_b = {self.n_samples}")
            return np.concatenate([np.asarray(a, dtype=np.float32) for a in x], axis=0)
        x = np.asarray(x)
        if not self.dense or x.shape != (self.B, self.n_samples[0], self.M):
            raise ValueError(f"x has shape {x.shape}: expected {(self.B, self.n_samples[0], self.M) if self.dense else 'a list of rooms'}")
        return np.ascontiguousarray(x, dtype=np.float32).reshape(-1, self.M)

    def analysis_device(self, x):
        """x: (B, n_samples, M) real or the list of B (n_b, M) arrays -> the ``DeviceBatch`` X, valid until the next
        ``analysis_device`` on this handle or its ``close()``"""
        if not self.h:
            raise RuntimeError("the handle is closed")
        xp = self._pack(x)
        dev = C.c_void_p()
        _lib.check(self.lib.oiva_bstft_analysis(self.h, _lib.ptr(xp), C.byref(dev)))
        return DeviceBatch(dev.value, self.frames, self.n_freq, self.M, self.dense, owner=self)

    def synthesis_device(self, Y_dev, K=None):
        """Y_dev: a ``DeviceBatch`` (``BatchPlan.demix_device``) or the address of a (sum T_b, F, K) complex64 device array ->
        host audio (B, T * hop, K) float32, or the list of B (T_b * hop, K) arrays"""
        if not self.h:
            raise RuntimeError("the handle is closed")
        if isinstance(Y_dev, DeviceBatch):
            if Y_dev.frames != self.frames or Y_dev.n_freq != self.n_freq:
                raise ValueError(f"Y holds frames {Y_dev.frames} x {Y_dev.n_freq} bins, the handle {self.frames} x {self.n_freq}")
            K = Y_dev.n_chan if K is None else K
            if K != Y_dev.n_chan:
                raise ValueError(f"K = {K} but Y holds {Y_dev.n_chan} channels")
            ptr = Y_dev.ptr
        else:
            ptr = int(Y_dev)
        if K is None or not 1 <= K <= self.M:
            raise ValueError(f"K must be in 1..{self.M}")
        y = np.empty((int(self.out_offsets[-1]), int(K)), np.float32)
        _lib.check(self.lib.oiva_bstft_synthesis_dev(self.h, C.c_void_p(ptr), int(K), _lib.ptr(y)))
        if self.dense:
            return y.reshape(self.B, self.frames[0] * self.hop, int(K))
        return [y[self.out_offsets[b]:self.out_offsets[b + 1]] for b in range(self.B)]

    def phase_ms(self):
        """device time of every phase of the last analysis and the last synthesis, ms, by events on the handle's stream"""
        ms = (C.c_float * len(PHASES))()
        _lib.check(self.lib.oiva_bstft_phase_ms(self.h, ms))
        return dict(zip(PHASES, list(ms)))


def _check_separate_args(x, frame, hop, n_src, n_iter, algorithm, model, win_a, win_s, W0, algo_kwargs):
    ragged = isinstance(x, (list, tuple))
    if ragged:
        rooms = [np.asarray(a) for a in x]
        if not rooms:
            raise ValueError("x is empty: separate_batch needs at least one room")
        for b, a in enumerate(rooms):
            if a.ndim != 2:
                raise ValueError(f"x[{b}] has shape {a.shape}: every room must be (n_samples, n_chan)")
        if len({a.dtype for a in rooms}) != 1:
            raise ValueError(f"the rooms have mixed dtypes {sorted({str(a.dtype) for a in rooms})}: give them one real dtype")
        M = rooms[0].shape[1]
        for b, a in enumerate(rooms):
            if a.shape[1] != M:
                raise ValueError(f"x[{b}] has {a.shape[1]} channels, x[0] has {M}: the channel count must agree")
        dtype, lens = rooms[0].dtype, [a.shape[0] for a in rooms]
    else:
        rooms = np.asarray(x)
        if rooms.ndim != 3:
            raise ValueError("x must have shape (batch, n_samples, n_chan), or be a sequence of (n_samples_b, n_chan) arrays")
        if rooms.shape[0] < 1:
            raise ValueError("x holds no room")
        dtype, M, lens = rooms.dtype, rooms.shape[2], [rooms.shape[1]] * rooms.shape[0]
    if dtype.kind not in "fiu":
        raise ValueError(f"x must be real, got dtype {dtype}")
    if algorithm not in ("overiva", "ogive", "auxiva_pca", "auxiva_iss", "five", "overiva_ip2"):
        raise ValueError(f"algorithm must be 'overiva', 'ogive', 'auxiva_pca', 'auxiva_iss', 'five' or 'overiva_ip2', got {algorithm!r}")
    if algorithm == "ogive" and ragged:
        raise ValueError("OGIVE does not run on a ragged batch: give algorithm='ogive' rooms of one length as a (B, n_samples, M) array")
    if algorithm != "ogive" and algo_kwargs:
        raise ValueError(f"unknown arguments for algorithm={algorithm!r}: {sorted(algo_kwargs)}")
    if set(algo_kwargs) - {"step_size", "tol", "update"}:
        raise ValueError(f"unknown arguments for algorithm='ogive': {sorted(set(algo_kwargs) - {'step_size', 'tol', 'update'})}")
    if algo_kwargs.get("update", "demix") not in _ive.UPDATE_IDS:
        raise ValueError(f"update must be one of {sorted(_ive.UPDATE_IDS)}, got {algo_kwargs['update']!r}")
    if isinstance(frame, bool) or not isinstance(frame, (int, np.integer)):
        raise ValueError(f"frame must be an integer, got {frame!r}")
    hop = frame // 2 if hop is None else hop
    _check_stft_args(lens, M, frame, hop)
    wa, ws = _windows(frame, hop, win_a, win_s)
    B, F = len(lens), frame // 2 + 1
    if algorithm == "ogive":
        if n_src not in (None, 1):
            raise ValueError("OGIVE extracts one source: n_src must be 1 (or None)")
        K = 1
    elif algorithm == "five":
        if n_src is not None and (isinstance(n_src, bool) or not isinstance(n_src, (int, np.integer)) or n_src != 1):
            raise ValueError(f"FIVE extracts one source: n_src must be None or 1, got {n_src!r}")
        K = 1
    elif algorithm == "auxiva_iss":
        if n_src is not None and (isinstance(n_src, bool) or not isinstance(n_src, (int, np.integer)) or n_src != M):
            raise ValueError(f"ISS is determined: n_src must be None or the channel count {M}, got {n_src!r}")
        K = M
        for b, n in enumerate(lens):
            if (n // hop) * M > _iss.MAX_SLAB:
                raise ValueError(f"algorithm='auxiva_iss' needs n_frames * n_chan <= {_iss.MAX_SLAB} in every room: room {b} has "
                                 f"{n // hop} x {M}")
    else:
        K = M if n_src is None else n_src
        if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= K <= M:
            raise ValueError(f"n_src must be in 1..{M}")
    if model not in ("laplace", "gauss"):
        raise ValueError(f"model must be 'laplace' or 'gauss', got {model!r}")
    if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)) or n_iter < 0:
        raise ValueError("n_iter must be an integer >= 0")
    _batch._check_w0(W0, B, F, K if algorithm == "auxiva_pca" else M, K)      # (auxiva_pca: the start of the reduced solve)
    if sharded.active_group() is not None:
        raise ValueError("separate_batch does not run under enable_bin_sharding(): disable bin sharding for batched calls")
    return rooms, ragged, lens, int(M), int(hop), int(K), wa, ws, np.float64 if dtype == np.float64 else np.float32


def separate_batch(x, frame, hop=None, n_src=None, n_iter=20, algorithm="overiva", model="laplace", win_a=None, win_s=None,
                   init_eig=False, W0=None, proj_back=True, return_filters=False, **algo_kwargs):
    """
    Audio in, audio out for B rooms: STFT, ``overiva_batch`` / ``overiva_batch_ragged`` / ``ogive_batch`` / ``auxiva_pca_batch`` /
    ``auxiva_iss_batch`` / ``five_batch`` / ``overiva_ip2_batch`` and inverse STFT with X and Y never leaving the device (the chain of reference overiva_sim.py:206-207, 298-315 for many rooms per call).

    Parameters
    ----------
    x: ndarray (batch, n_samples, n_chan) real, or a sequence of B arrays (n_samples_b, n_chan) of one channel count and dtype
        microphone signals, 1..8 channels; a sequence may hold rooms of different lengths
    frame, hop: int
        STFT frame length (even) and shift (default frame // 2); n_frames = n_samples // hop as ``stft.analysis``
    n_src, n_iter, model, init_eig, W0, proj_back, return_filters:
        as ``overiva_batch()`` (``n_src=None``: determined AuxIVA)
    algorithm: "overiva", "overiva_ip2" (the same with pairwise IP2 updates, as ``overiva_ip2_batch()``), "auxiva_iss" (determined AuxIVA by rank-1 ISS updates, as ``auxiva_iss_batch()``: ``n_src`` None or
        n_chan), "five" (one source by FIVE, as ``five_batch()``: ``n_src`` None or 1; rooms of any lengths), "ogive" (one
        source, rooms of one length; ``step_size``, ``tol``, ``update`` as ``ogive_batch()``) or
        "auxiva_pca" (PCA to ``n_src`` channels, then determined AuxIVA, as ``auxiva_pca_batch()``: ``W0`` starts the reduced
        solve, (n_freq, n_src, n_src); ``proj_back`` is ignored, the result is always projected back; W is the composed filters)
    win_a, win_s: analysis / synthesis windows; default ``stft.hann(frame)`` and its ``stft.compute_synthesis_window`` when
        hop < frame, rectangular otherwise

    Returns
    -------
    y (batch, n_frames * hop, n_src), or the list of B arrays (n_frames_b * hop, n_src) for a sequence; float32, or float64 for
    float64 input.  With ``return_filters`` also W (batch, n_freq, n_chan, n_src) complex128.  A room whose W ends non-finite
    raises ``numpy.linalg.LinAlgError`` naming every such room.
    """
    rooms, ragged, lens, M, hop, K, wa, ws, out_dtype = _check_separate_args(x, frame, hop, n_src, n_iter, algorithm, model, win_a,
                                                                             win_s, W0, algo_kwargs)
    B, F = len(lens), frame // 2 + 1
    with BatchSTFT(lens if ragged else lens[0], M, frame, hop, win_a=wa, win_s=ws, B=None if ragged else B) as st:
        Xd = st.analysis_device(list(rooms) if ragged else rooms)
        plan = _batch.RaggedBatchPlan(st.frames, F, M, K, model) if ragged else _batch.BatchPlan(B, st.frames[0], F, M, K, model)
        with plan:
            plan.set_x_device(Xd.ptr, keepalive=Xd)
            plan.covariance()
            info = dict(plan.info(), audio=True)
            if algorithm == "ogive":
                epochs, converged = _batch._run_ogive(plan, n_iter, W0, init_eig, model, **algo_kwargs)
                info.update(algorithm="ogive", epochs=[int(e) for e in epochs], converged=[bool(c) for c in converged])
            elif algorithm == "auxiva_pca" and K < M:
                _pca_batch.reduce_and_solve(plan, n_iter, W0, init_eig, model)
            elif algorithm == "auxiva_iss":
                _iss.run_iss(plan, n_iter, W0, init_eig)
                info.update(algorithm="auxiva_iss")
            elif algorithm == "five":
                run_five(plan, n_iter, W0, init_eig)
                info.update(algorithm="five")
            elif algorithm == "overiva_ip2":
                _ip2.run_ip2(plan, n_iter, W0, init_eig)
                info.update(algorithm="overiva_ip2")
            else:
                if W0 is None and init_eig:
                    plan.set_w_eig()
                else:
                    plan.set_w(W0)
                plan.iterate(n_iter)
            if algorithm == "auxiva_pca":           # always projected back onto channel 0 of the input (auxiva_pca.py:89-90)
                proj_back = True
                info.update(algorithm="auxiva_pca", reduced=K)
            y = st.synthesis_device(plan.demix_device(proj_back))
            _batch._info = info
            if algorithm == "overiva":
                _batch._overiva_module._last_info = dict(info)
            W = plan.get_w(np.complex128)           # (raises LinAlgError naming the non-finite rooms)
    if out_dtype != np.float32:
        y = [a.astype(out_dtype) for a in y] if ragged else y.astype(out_dtype)
    return (y, W) if return_filters else y
