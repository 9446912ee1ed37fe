"""``sweep_batch()``: one step of the reference's Monte-Carlo sweep (``overiva_sim.py:one_loop``) for B rooms per call, from the
geometry to the SDR curves, with every hand-over on the device.

``simulate_batch()``, ``separate_batch()`` and ``bss_eval_batch()`` each put one stage of that step on the device; chained, the
mix, the references, the separated audio and the estimates still go through the host between them.  Here the float64 mix of the
room simulation is cast and transformed where it lies (``oiva_bstft_analysis_dev``), one X serves every entry of ``algorithms``,
the synthesis of a solver's Y stays on the device (``oiva_bstft_synthesis_keep``) and a gather kernel writes the references and
the ordered, trimmed estimates straight into the buffers of a ``BssEval`` handle (``oiva_sweep_*``, csrc/kernels_sweep.hip).  The
solvers, the STFT kernels and the BSS Eval kernels are the ones the three public calls use, on the same bits, and every new step
is exact (the cast the host would do, a gather, float32 -> float64) or decides only an ordering (the channels' standard
deviations): the criteria are those of the chain of the three calls, bit for bit.

**What still crosses the bus**: the source signals and the geometry in, ``noise`` in (the caller's), the filler in, the criteria
out -- and a few words per launch.  With ``seed`` the noise and the filler that the caller does not give are drawn on the device
from the seeded stream of DESIGN.md 3.13 (``overiva_amd/rng.py``, csrc/kernels_rng.hip), straight into the buffers the mix-down
and the gather read: then signals, geometry and seeds go in and the criteria come out.

Alignment: this project's STFT has no delay, ``y[i]`` lines up with ``x[i]`` and the last ``frame - hop`` samples lack their
later overlaps, so the reference's ``y[framesize // 2 : m + framesize // 2]`` is ``y[0 : m_b]`` here, with
``m_b = T_b * hop - (frame - hop)`` and ``T_b = n_out_b // hop``.
"""
import ctypes as C
import time

import numpy as np

from . import _lib
from . import batch as _batch
from . import metrics as _metrics
from . import pca_batch as _pca_batch
from . import rng as _rng
from . import room as _room
from . import separate as _separate
from .batch import DeviceBatch
from .overiva import get_device

MAX_MICS = _batch.MAX_CHANNELS
MAX_TARGETS = _metrics.MAX_SOURCES - 1
ALGOS = ("auxiva", "overiva", "auxiva_pca", "ogive", "auxiva_ip2", "overiva_ip2")
OVERDET_ALGOS = ("overiva", "ogive", "auxiva_pca", "overiva_ip2")
_DEFAULT_N_ITER = {"auxiva": 20, "overiva": 20, "auxiva_pca": 20, "ogive": 4000, "auxiva_ip2": 20, "overiva_ip2": 20}
_DETERMINED = ("auxiva", "auxiva_ip2")       # run on all the channels, whatever n_targets
_IP2 = ("auxiva_ip2", "overiva_ip2")         # the pairwise update (ip2.py) with the keys and the cadence of "auxiva" / "overiva"
_SOLVER_KEYS = {"n_iter", "proj_back", "model", "init_eig", "W0"}
_OGIVE_KEYS = {"step_size", "tol", "update"}


def checkpoints(algo, n_iter, monitor_convergence=False):
    """the iteration counts at which ``sweep_batch`` evaluates an entry.  Without monitoring: ``[0, n_iter]``, the entry at 0
    being the shared evaluation of the unprocessed microphones (``overiva_sim.py:240-243, 289-290``).  With monitoring the
    callback cadence of the solver and then its final state (``:272-284, 323-332``): epochs 0, 10, 20, ... below ``n_iter`` for
    "auxiva" and "overiva" (and their IP2 forms "auxiva_ip2" and "overiva_ip2"); 0, 100, 200, ... for "ogive" -- the list when no group of rooms stops early: the cadence ends once every
    room's stopping rule has fired.  "auxiva_pca" is evaluated at its ends only, ``[0, n_iter]`` with the shared initial
    evaluation at 0, monitored or not: its iterations run on the reduced channels and composing the filters consumes the PCA
    basis, so there is no state to look at in between."""
    if algo not in ALGOS:
        raise ValueError(f"algo must be one of {ALGOS}, got {algo!r}")
    n_iter = int(n_iter)
    if not monitor_convergence or algo == "auxiva_pca":
        return [0, n_iter]
    return list(range(0, n_iter, 100 if algo == "ogive" else 10)) + [n_iter]


def _check_algorithms(algorithms, n_targets, lens, M, frame, hop, win_a, win_s, overdet_algos):
    """-> the list of entries that run: dicts(name, algo, n_src, n_iter, proj_back, model, init_eig, W0, ogive, reorder)"""
    if algorithms is None:
        algorithms = {"overiva": {"algo": "overiva", "kwargs": {"n_iter": 20}}}
    if not isinstance(algorithms, dict) or not algorithms:
        raise ValueError("algorithms must be a non-empty dict {name: {'algo': ..., 'kwargs': {...}}}")
    if isinstance(overdet_algos, str) or not all(isinstance(a, str) for a in overdet_algos):
        raise ValueError("overdet_algos must be a sequence of algorithm names")
    dense = len(set(lens)) == 1
    # what the checkers of separate_batch look at is the shape of the audio, never its samples
    audio = np.broadcast_to(np.float32(0), (len(lens), lens[0], M)) if dense else [np.broadcast_to(np.float32(0), (n, M)) for n in lens]
    entries = []
    for name, params in algorithms.items():
        if not isinstance(params, dict) or "algo" not in params:
            raise ValueError(f"algorithms[{name!r}] must be a dict with the keys 'algo' and 'kwargs'")
        algo, kwargs = params["algo"], dict(params.get("kwargs") or {})
        if algo == "ilrma":
            raise ValueError(f"algorithms[{name!r}]: ILRMA ('ilrma') does not run in sweep_batch: ilrma_batch has no device-X entry "
                             "and no ragged form")
        if algo not in ALGOS:
            raise ValueError(f"algorithms[{name!r}]: algo must be one of {ALGOS}, got {algo!r}")
        allowed = _SOLVER_KEYS | (_OGIVE_KEYS if algo == "ogive" else set())
        if set(kwargs) - allowed:
            raise ValueError(f"algorithms[{name!r}]: unknown arguments for algo={algo!r}: {sorted(set(kwargs) - allowed)}")
        if (algo == "auxiva_pca" and n_targets == 1) or (algo == "ogive" and n_targets != 1):      # overiva_sim.py:250-255
            continue
        n_iter = kwargs.get("n_iter", _DEFAULT_N_ITER[algo])
        n_src = None if algo in _DETERMINED or algo == "ogive" else n_targets
        if algo == "ogive" and not dense:
            raise ValueError(f"algorithms[{name!r}]: OGIVE needs rooms of one output length")
        solver = "overiva_ip2" if algo in _IP2 else "overiva" if algo == "auxiva" else algo
        try:
            _separate._check_separate_args(audio, frame, hop, n_src, n_iter, solver, kwargs.get("model", "laplace"), win_a, win_s,
                                           kwargs.get("W0"), {k: kwargs[k] for k in _OGIVE_KEYS if k in kwargs})
        except ValueError as e:
            raise ValueError(f"algorithms[{name!r}]: {e}") from None
        entries.append(dict(name=name, algo=algo, n_src=M if algo in _DETERMINED else 1 if algo == "ogive" else n_targets,
                            n_iter=int(n_iter), proj_back=bool(kwargs.get("proj_back", True)) or algo == "auxiva_pca",
                            model=kwargs.get("model", "laplace"), init_eig=bool(kwargs.get("init_eig", False)), W0=kwargs.get("W0"),
                            ogive={k: kwargs[k] for k in _OGIVE_KEYS if k in kwargs}, reorder=algo not in overdet_algos))
    return entries


def _eval_lengths(out_lengths, frame, hop):
    """m_b of every room; a room without one complete frame is refused"""
    m = []
    for b, n in enumerate(out_lengths):
        mb = n // hop * hop - (frame - hop)
        if mb < 1:
            raise ValueError(f"room {b} is too short for one complete frame: {n} output samples, frame {frame}, hop {hop}")
        m.append(int(mb))
    return m


def _check_filler(filler, B):
    if filler is None:
        return None
    rows = [np.asarray(a) for a in filler] if isinstance(filler, (list, tuple)) else np.asarray(filler)
    if not isinstance(rows, list):
        if rows.ndim != 2:
            raise ValueError(f"filler must have shape (batch, >= m_b) or be a sequence of 1-D arrays, got shape {rows.shape}")
        rows = list(rows)
    if len(rows) != B:
        raise ValueError(f"filler holds {len(rows)} rooms, room_dim {B}: the batch must agree")
    out = []
    for b, a in enumerate(rows):
        if a.ndim != 1 or a.dtype.kind not in "fiu":
            raise ValueError(f"filler: room {b} must be a real 1-D array, got shape {a.shape} and dtype {a.dtype}")
        a = np.ascontiguousarray(a, dtype=np.float64)
        if not np.all(np.isfinite(a)):
            raise ValueError(f"filler: room {b} holds non-finite samples")
        out.append(a)
    return out


class SweepBatch(_lib.Handle):
    """the staged form of ``sweep_batch``: a ``RoomBatch`` and, for the room group at hand, a ``BatchSTFT``, the sweep handle
    (``oiva_sweep``), a ``BssEval`` the device gather writes into and a ``BssEvalSets`` that evaluates what was gathered: the
    group's references are prepared once, every later evaluation runs the estimate half alone.

    ``set_signals`` (the impulse responses, then the signals; ``max_group`` as ``RoomBatch.set_signals``), ``set_filler``, then per
    group g0: ``open_group``, ``convolve``, ``mix``, ``take_mix`` (-> the ``DeviceBatch`` X every solver borrows) and
    ``evaluate(Y, reorder)`` for every state to be measured -- or ``gather(Y, reorder, e)`` for several states and one
    ``evaluate_sets(n)`` for all of them.  ``get_order`` / ``get_eval_signals`` read what the last ``evaluate`` or ``gather``
    left."""

    _destroy = "oiva_sweep_destroy"
    room = stft = ev = sets = g0 = filler_gen = None
    rooms = ()

    def __init__(self, room_dim, sources, mics, frame, hop=None, n_targets=1, fs=16000, max_order=17, absorption=0.35, c=343.0,
                 rir_length=None, ref_mic=0, filter_length=512, win_a=None, win_s=None, device=None):
        M = np.shape(mics)[1] if np.ndim(mics) == 3 else 0
        if not 1 <= M <= MAX_MICS:
            raise ValueError(f"sweep_batch runs on 1..{MAX_MICS} microphones, got {M}")
        if not _room._is_int(n_targets) or not 1 <= n_targets <= min(M, MAX_TARGETS):
            raise ValueError(f"n_targets must be an integer in 1..min(n_mics, {MAX_TARGETS}) = {min(M, MAX_TARGETS)}, got {n_targets!r}")
        if not _room._is_int(ref_mic) or not 0 <= ref_mic < M:
            raise ValueError(f"ref_mic must be in 0..{M - 1}, got {ref_mic!r}")
        if not _room._is_int(filter_length) or not 1 <= filter_length <= _metrics.MAX_FILTER:
            raise ValueError(f"filter_length must be an integer in 1..{_metrics.MAX_FILTER}, got {filter_length!r}")
        if not _room._is_int(frame):
            raise ValueError(f"frame must be an integer, got {frame!r}")
        hop = frame // 2 if hop is None else hop
        _separate._check_stft_args([max(int(hop), 1) if _room._is_int(hop) else 1], M, frame, hop)
        self.win_a, self.win_s = _separate._windows(frame, hop, win_a, win_s)
        self.device = get_device() if device is None else int(device)
        self.room = _room.RoomBatch(room_dim, sources, mics, fs=fs, max_order=max_order, absorption=absorption, c=c,
                                    rir_length=rir_length, device=self.device)
        self.lib = self.room.lib
        self.B, self.S, self.M, self.K = self.room.B, self.room.S, int(M), int(n_targets)
        self.frame, self.hop, self.ref_mic, self.Lf = int(frame), int(hop), int(ref_mic), int(filter_length)
        self.out_lengths = self.eval_lengths = self.group = self.filler = self.filler_keys = None
        self.g0, self.stft, self.ev, self.sets, self.rooms, self.last_C = None, None, None, None, (), 0
        self.reference_preparations = self.sets_evaluated = self.groups_without_sets = 0

    def set_signals(self, signals, max_group=0):
        """signals: B arrays (S, n_b); computes the impulse responses on first use; -> rooms per group"""
        if self.room.rir_lengths is None:
            self.room.compute_rir()
        self.close_group()
        self.group = self.room.set_signals(signals, max_group)
        self.out_lengths = list(self.room.out_lengths)
        self.eval_lengths = _eval_lengths(self.out_lengths, self.frame, self.hop)
        return self.group

    def set_filler(self, filler=None, seed=None):
        """filler: B 1-D arrays of at least m_b samples each, or None: room b gets the first m_b draws of
        ``numpy.random.default_rng(0).standard_normal`` -- every room from a generator of its own, so that a room's row does not
        depend on the batch it is in.  seed (an int, or one int per room, as ``sweep_batch`` takes it) instead of a filler: room
        b's row is the first m_b values of its purpose-1 stream, drawn on the device when its group is opened"""
        if seed is not None:
            if filler is not None:
                raise ValueError("filler and seed exclude each other: the row is the caller's or drawn on the device")
            self.filler_keys, self.filler = _rng.check_seed(seed, self.B), None
            if self.h:
                self._draw_filler()
            return
        self.filler_keys = None
        self._close_filler_gen()
        if filler is None:
            filler = [np.random.default_rng(0).standard_normal(m) for m in self.eval_lengths]
        if len(filler) != self.B:
            raise ValueError(f"filler must hold {self.B} rooms")
        for b, (a, m) in enumerate(zip(filler, self.eval_lengths)):
            if np.ndim(a) != 1 or len(a) < m:
                raise ValueError(f"filler: room {b} has {np.shape(a)} samples, {m} are evaluated (m_b = T_b * hop - (frame - hop))")
        self.filler = [np.ascontiguousarray(a[:m], dtype=np.float64) for a, m in zip(filler, self.eval_lengths)]
        if self.h:
            self._upload_filler()

    def _upload_filler(self):
        packed = np.concatenate([self.filler[b] for b in self.rooms])
        _lib.check(self.lib.oiva_sweep_set_filler(self.h, _lib.ptr(packed)))

    def _draw_filler(self):
        """the open group's filler rows on the device: packed (sum m_b), the ``filler_dev`` of every ``evaluate``"""
        self._close_filler_gen()
        self.filler_gen = _rng.DeviceNormal([self.eval_lengths[b] for b in self.rooms], device=self.device)
        self.filler_gen.fill(*(k[self.rooms.start:self.rooms.stop] for k in self.filler_keys), purpose=_rng.FILLER)

    def _close_filler_gen(self):
        if self.filler_gen is not None:
            self.filler_gen.close()
        self.filler_gen = None

    def open_group(self, g0=0, max_sets=1):
        """the handles of the group that starts at room g0 (those of the group before are closed); max_sets: the most states
        that are gathered before one ``evaluate_sets``.  When the ``BssEvalSets`` handle cannot be made for lack of memory the
        group evaluates every state with a full ``BssEval.run()`` instead (``groups_without_sets`` counts such groups)"""
        if self.group is None:
            raise RuntimeError("signals not set")
        if self.filler is None and self.filler_keys is None:
            self.set_filler()
        self.close_group()
        self.rooms = self.room.group_rooms(g0)
        lens = [self.out_lengths[b] for b in self.rooms]
        self.dense = len(set(lens)) == 1
        self.stft = _separate.BatchSTFT(lens[0] if self.dense else lens, self.M, self.frame, self.hop, win_a=self.win_a,
                                        win_s=self.win_s, device=self.device, B=len(lens) if self.dense else None)
        h = C.c_void_p()
        ns = (C.c_int * len(lens))(*lens)
        _lib.check(self.lib.oiva_sweep_create(C.byref(h), self.device, len(lens), ns, self.M, self.K, self.frame, self.hop, self.ref_mic,
                                              self.Lf, None))
        self.h = h
        self.ev = _metrics.BssEval([self.eval_lengths[b] for b in self.rooms], self.K + 1, self.Lf, device=self.device)
        try:
            self.sets = _metrics.BssEvalSets([self.eval_lengths[b] for b in self.rooms], self.K + 1, self.Lf, max_sets=max(1, int(max_sets)),
                                             device=self.device)
        except _lib.HipError as err:
            if not _metrics._is_out_of_memory(err):
                raise
            self.sets = None
            self.groups_without_sets += 1
        self.max_sets, self.references_taken, self.pending = max(1, int(max_sets)), False, []
        self.g0, self.last_C = int(g0), 0
        if self.filler_keys is not None:
            self._draw_filler()
        else:
            self._upload_filler()

    def close_group(self):
        _lib.Handle.close(self)
        if self.sets is not None:
            prep, done = self.sets.counts()
            self.reference_preparations += prep
            self.sets_evaluated += done
        for part in (self.stft, self.ev, self.sets, self.filler_gen):
            if part is not None:
                part.close()
        self.stft = self.ev = self.sets = self.g0 = self.filler_gen = None
        self.rooms = ()

    def close(self):
        self.close_group()
        if self.room is not None:
            self.room.close()

    def convolve(self, g0=0):
        self.room.convolve(g0)

    def mix(self, g0=0, sinr=10.0, snr=60.0, sources_var=None, noise=None, seed_keys=None):
        """as ``RoomBatch.mix`` with this handle's ``n_targets`` and ``ref_mic``"""
        self.room.mix(g0, n_targets=self.K, sinr=sinr, snr=snr, ref_mic=self.ref_mic, sources_var=sources_var, noise=noise,
                      seed_keys=seed_keys)

    def take_mix(self):
        """the open group's mix -> X on the device (float64 -> float32 and the analysis, no host copy): a ``DeviceBatch`` valid
        until the next ``take_mix`` or the group's end"""
        dev = C.c_void_p()
        _lib.check(self.lib.oiva_sweep_take_mix(self.h, self.room.h, self.g0, self.stft.h, C.byref(dev)))
        return DeviceBatch(dev.value, self.stft.frames, self.stft.n_freq, self.M, self.dense, owner=self.stft)

    def evaluate(self, Y, reorder):
        """Y: a ``DeviceBatch`` of n_targets..M channels (X itself, or a plan's ``demix_device``) -> sdr, sir, sar
        (rooms, K + 1) and perm (rooms, K + 1) of the open group, the permutation chosen on the host as ``bss_eval_batch`` does:
        one state, gathered into set 0 and evaluated at once"""
        self.gather(Y, reorder, 0)
        return self.evaluate_sets(1)[0]

    def gather(self, Y, reorder, e):
        """the synthesis of Y, ordered and aligned, into the ``BssEval`` handle (``oiva_sweep_evaluate``) and from there, device to
        device, into set e; the group's first gather also takes the references and prepares them"""
        if Y.frames != self.stft.frames or Y.n_freq != self.stft.n_freq:
            raise ValueError(f"Y holds frames {Y.frames} x {Y.n_freq} bins, the group {self.stft.frames} x {self.stft.n_freq}")
        if not 0 <= e < self.max_sets:
            raise ValueError(f"set {e} is not in 0..{self.max_sets - 1}")
        _lib.check(self.lib.oiva_sweep_evaluate(self.h, self.stft.h, C.c_void_p(Y.ptr), int(Y.n_chan), 1 if reorder else 0, self.ev.h,
                                                None if self.filler_gen is None else C.c_void_p(self.filler_gen.ptr)))
        self.last_C = int(Y.n_chan)
        if self.sets is None:                                      # no room for the sets: the full evaluation, now
            self.ev.run()
            self.reference_preparations += 1
            self.sets_evaluated += 1
            self.pending.append((e, self.ev.get_criteria()))
            return
        self.sets.take(self.ev, e, with_references=not self.references_taken)
        if not self.references_taken:
            self.sets.prepare()
            self.references_taken = True

    def evaluate_sets(self, n_sets):
        """the gathered sets 0 .. n_sets - 1 in one set of launches -> a list of (sdr, sir, sar, perm) as ``evaluate`` gives"""
        R = len(self.rooms)
        if self.sets is None:
            by_set = dict(self.pending)
            self.pending = []
            per_set = [by_set[e] for e in range(n_sets)]
        else:
            self.sets.evaluate(0, n_sets)
            mats = self.sets.get_criteria(0, n_sets)
            per_set = [tuple(m[:, e] for m in mats) for e in range(n_sets)]
        cols = np.arange(self.K + 1)
        out = []
        for mats in per_set:
            perm = np.stack([_metrics.best_permutation(mats[1][b]) for b in range(R)])
            out.append(tuple(np.stack([m[b][perm[b], cols] for b in range(R)]) for m in mats) + (perm,))
        return out

    def get_order(self):
        """test hook: (order, std), both (rooms, C), of the last ``evaluate`` or ``gather``"""
        n = len(self.rooms) * self.last_C
        order, std = (C.c_int * max(n, 1))(), np.empty(max(n, 1))
        _lib.check(self.lib.oiva_sweep_get_order(self.h, order, _lib.ptr(std)))
        return np.array(list(order), dtype=int)[:n].reshape(len(self.rooms), -1), std[:n].reshape(len(self.rooms), -1)

    def get_eval_signals(self):
        """test hook: (ref, est), two lists of (K + 1, m_b) arrays: what the last ``evaluate`` or ``gather`` left in the ``BssEval`` handle"""
        sizes = [(self.K + 1) * self.eval_lengths[b] for b in self.rooms]
        ref, est = np.empty(sum(sizes)), np.empty(sum(sizes))
        _lib.check(self.lib.oiva_sweep_get_signals(self.h, self.ev.h, _lib.ptr(ref), _lib.ptr(est)))
        off = np.concatenate([[0], np.cumsum(sizes)])
        cut = lambda a: [a[off[i]:off[i + 1]].reshape(self.K + 1, -1) for i in range(len(sizes))]      # noqa: E731
        return cut(ref), cut(est)

    def phase_ms(self):
        """device ms of the last analysis and synthesis (``BatchSTFT.phase_ms``) and of the kernels of the last ``evaluate``"""
        ms = C.c_float()
        _lib.check(self.lib.oiva_sweep_phase_ms(self.h, C.byref(ms)))
        return dict(self.stft.phase_ms(), align=ms.value)


def _run_entry(sb, Xd, entry, monitor, init):
    """one entry of ``algorithms`` on the open group -> (checkpoints, [evaluation per checkpoint], solver seconds, ogive info).
    Every checkpoint is gathered into a set of its own as it is reached; the entry's sets are evaluated together at its end"""
    algo, n_iter, proj_back, reorder = entry["algo"], entry["n_iter"], entry["proj_back"], entry["reorder"]
    F, M, K = sb.stft.n_freq, sb.M, entry["n_src"]
    plan = (_batch.BatchPlan(len(sb.rooms), sb.stft.frames[0], F, M, K, entry["model"], device=sb.device) if sb.dense else
            _batch.RaggedBatchPlan(sb.stft.frames, F, M, K, entry["model"], device=sb.device))
    marks, evals, extra, gathered = [], [], {}, []
    spent = [0.0, time.perf_counter()]      # solver seconds so far, start of the running stretch

    def look(epoch):
        plan.status()                                              # (waits for the iterations: they are queued, not run, on return)
        spent[0] += time.perf_counter() - spent[1]
        marks.append(epoch)
        sb.gather(plan.demix_device(proj_back), reorder, len(gathered))
        gathered.append(len(evals))
        evals.append(None)
        spent[1] = time.perf_counter()

    with plan:
        plan.set_x_device(Xd.ptr, keepalive=Xd)
        plan.covariance()
        watched = monitor and algo != "auxiva_pca"
        if not watched:
            marks.append(0)
            evals.append(init)
        if algo == "ogive":
            every_100 = (lambda: look(100 * len(marks))) if watched else None
            epochs, converged = _batch._run_ogive(plan, n_iter, entry["W0"], entry["init_eig"], entry["model"], every_100=every_100,
                                                  **entry["ogive"])
            extra = dict(epochs=[int(e) for e in epochs], converged=[bool(c) for c in converged])
        elif algo == "auxiva_pca" and K < M:
            _pca_batch.reduce_and_solve(plan, n_iter, entry["W0"], entry["init_eig"], entry["model"])
        else:
            if entry["W0"] is None and entry["init_eig"]:
                plan.set_w_eig()
            else:
                plan.set_w(entry["W0"])
            epoch = 0
            while epoch < n_iter:                                  # the cadence of batch._run_overiva
                if watched and epoch % 10 == 0:
                    look(epoch)
                step = min(n_iter - epoch, 10 - epoch % 10) if watched else n_iter - epoch
                if algo in _IP2:
                    plan.ip2_iterate(epoch, step)
                else:
                    plan.iterate(step)
                epoch += step
        look(n_iter)
    for at, res in zip(gathered, sb.evaluate_sets(len(gathered))):
        evals[at] = res
    return marks, evals, spent[0], extra


def _merge(per_group, n_targets):
    """the groups' evaluations along the room axis; a group whose OGIVE cadence ended early repeats its final state"""
    marks = max((g[0] for g in per_group), key=len)
    out = []
    for field in range(4):
        rows = []
        for g_marks, evals, _, _ in per_group:
            padded = evals[:-1] + [evals[-1]] * (len(marks) - len(g_marks) + 1)
            rows.append(np.stack([e[field] for e in padded], axis=1))          # (rooms, checkpoints, K + 1)
        out.append(np.concatenate(rows, axis=0))
    sdr, sir, sar, perm = out
    return marks, sdr[:, :, :n_targets], sir[:, :, :n_targets], sar[:, :, :n_targets], perm


def sweep_batch(signals, room_dim, sources, mics, frame, hop=None, algorithms=None, n_targets=1, fs=16000, max_order=17,
                absorption=0.35, c=343.0, rir_length=None, sinr=10.0, snr=60.0, ref_mic=0, sources_var=None, noise=None, filler=None,
                filter_length=512, monitor_convergence=False, win_a=None, win_s=None, overdet_algos=OVERDET_ALGOS, max_group=0,
                seed=None):
    """
    One step of the reference's Monte-Carlo sweep (``overiva_sim.py:140-350``) for B rooms at once: shoebox rooms, mix-down, one
    STFT, every entry of ``algorithms`` on it, inverse STFT and BSS Eval at every checkpoint.  Between ``oiva_room_mix`` and the
    criteria the audio, X, Y, y and the references stay on the device.  **What still crosses the bus**: signals and geometry in,
    ``noise`` in, the filler in, the criteria out; with ``seed``: signals, geometry and seeds in, criteria out.  The criteria
    equal, bit for bit, those of ``simulate_batch`` -> ``mix.astype(float32)`` -> ``BatchSTFT`` / the batch plans /
    ``synthesis_device`` -> the ordering below -> ``bss_eval_batch``.

    Parameters
    ----------
    signals, room_dim, sources, mics, fs, max_order, absorption, c, rir_length, sinr, snr, ref_mic, sources_var, noise:
        as ``simulate_batch()``; 1..8 microphones; ``n_targets`` in 1..min(n_mics, 7)
    frame, hop, win_a, win_s: as ``separate_batch()``
    algorithms: dict ``{full_name: {"algo": "auxiva" | "overiva" | "auxiva_pca" | "ogive" | "auxiva_ip2" | "overiva_ip2", "kwargs": {...}}}``, the reference's
        ``algorithm_kwargs`` block as it stands (default: one "overiva" entry with ``n_iter=20``).  "auxiva" is ``overiva`` without
        ``n_src``; "overiva" and "auxiva_pca" get ``n_src=n_targets``; "auxiva_ip2" and "overiva_ip2" are "auxiva" and "overiva" with
        pairwise IP2 updates (``overiva_ip2_batch``), the same kwargs and checkpoints.  kwargs: ``n_iter``, ``proj_back``, ``model``,
        ``init_eig``, ``W0`` and, for "ogive", ``step_size``, ``tol``, ``update``.  Skipped as the reference skips them:
        "auxiva_pca" with one target, "ogive" with more than one.  "ilrma" is refused.  "ogive" needs rooms of one output length.
    filler: (batch, >= m_b) or a sequence of 1-D arrays: the row that is held against the background (``overiva_sim.py:200``);
        default without ``seed``: every room's first m_b draws of its own ``numpy.random.default_rng(0).standard_normal``
    seed: None, or the seed of what is drawn on the device (``standard_normal_batch()``): whichever of ``noise``
        and ``filler`` is None.  Room b's noise is the row-major (n_out_b, n_mics) array of its purpose-0 stream, its filler the
        first m_b values of its purpose-1 stream.  An int s in 0..2**64 - 1 gives room b the key (s, b): its draws then **depend
        on the room's index in the batch**.  A sequence of B such ints gives room b the key (seed[b], 0), one seed per run as
        the reference's argument lists carry them, and a room's draws do not depend on the batch.  ``seed`` with both ``noise``
        and ``filler`` given is refused: nothing would be drawn.  Without ``seed`` nothing is drawn: ``noise=None`` is no noise
    filter_length: taps of the BSS Eval filter, 1..512
    monitor_convergence: evaluate along the way, at ``checkpoints(algo, n_iter, True)``; otherwise ``[0, n_iter]`` with the shared
        evaluation of the unprocessed microphones at 0
    overdet_algos: the ``algo`` values whose channels keep their order; every other output (and the unprocessed microphones) is
        ordered by descending standard deviation before the first ``n_targets`` channels are kept (``overiva_sim.py:220-222``)
    max_group: 0, or the most rooms that go through the stages together, as ``RoomBatch.set_signals``; a room's bits do not
        depend on it

    Returns
    -------
    a list of dicts, one per entry that ran: "algorithm" (the full name), "n_targets", "n_mics", "checkpoints" (iteration
    counts), "sdr", "sir", "sar" (batch, n_checkpoints, n_targets), "perm" (batch, n_checkpoints, n_targets + 1), "n_samples"
    (output samples per room), "runtime" (seconds of the solver stage for the whole batch, host clock) and, for "ogive",
    "epochs" and "converged" per room.  A room whose filters end non-finite has NaN criteria from there on.
    """
    geometry = _room._check_geometry(room_dim, sources, mics, fs, max_order, absorption, c, rir_length)
    B, S, M = geometry[0].shape[0], geometry[1].shape[1], geometry[2].shape[1]
    sig, ragged = _room._check_signals(signals, B, S)
    if not 1 <= M <= MAX_MICS:
        raise ValueError(f"sweep_batch runs on 1..{MAX_MICS} microphones, got {M}")
    if _room._is_int(n_targets) and n_targets > min(M, MAX_TARGETS):
        raise ValueError(f"n_targets must be at most min(n_mics, {MAX_TARGETS}) = {min(M, MAX_TARGETS)}, got {n_targets}")
    K, sinr, snr, ref_mic, var, noise = _room._check_mix(B, S, M, ragged, n_targets, sinr, snr, ref_mic, sources_var, noise)
    if not _room._is_int(filter_length) or not 1 <= filter_length <= _metrics.MAX_FILTER:
        raise ValueError(f"filter_length must be an integer in 1..{_metrics.MAX_FILTER}, got {filter_length!r}")
    if not _room._is_int(frame):
        raise ValueError(f"frame must be an integer, got {frame!r}")
    hop = frame // 2 if hop is None else hop
    # the output lengths are the signals' plus the impulse responses': known here with an integer rir_length; otherwise what
    # depends on them is checked once the device has told the impulse responses' lengths
    L = geometry[7]
    _separate._check_stft_args([hop] * B, M, frame, hop)
    lens = [a.shape[1] + L - 1 if L else max(a.shape[1] + _room.FDL - 1, frame) for a in sig]
    if L:
        _separate._check_stft_args(lens, M, frame, hop)
        _eval_lengths(lens, frame, hop)
    entries = _check_algorithms(algorithms, K, lens, M, frame, hop, win_a, win_s, overdet_algos)
    filler = _check_filler(filler, B)
    keys = None
    if seed is not None:
        if noise is not None and filler is not None:
            raise ValueError("seed with both noise and filler given: nothing is left to draw on the device")
        keys = _rng.check_seed(seed, B)
    if not _room._is_int(max_group) or max_group < 0:
        raise ValueError(f"max_group must be an integer >= 0, got {max_group!r}")
    _room._refuse_sharding("sweep_batch")
    with SweepBatch(geometry[0], geometry[1], geometry[2], frame, hop, n_targets=K, fs=geometry[4], max_order=geometry[6],
                    absorption=geometry[3], c=geometry[5], rir_length=L, ref_mic=ref_mic, filter_length=filter_length, win_a=win_a,
                    win_s=win_s) as sb:
        sb.set_signals(sig, max_group)
        if noise is not None:
            for b, a in enumerate(noise):
                if a.shape[0] != sb.out_lengths[b]:
                    raise ValueError(f"noise: room {b} has {a.shape[0]} samples, its output has {sb.out_lengths[b]}")
        if any(e["algo"] == "ogive" for e in entries) and len(set(sb.out_lengths)) > 1:
            raise ValueError(f"OGIVE needs rooms of one output length, the rooms come out {sb.out_lengths} samples long: give "
                             "rir_length and signals of one length")
        if keys is not None and filler is None:
            sb.set_filler(seed=seed)
        else:
            sb.set_filler(filler)
        draw_noise = keys is not None and noise is None
        watched = lambda e: monitor_convergence and e["algo"] != "auxiva_pca"      # noqa: E731
        results = [[] for _ in entries]
        for g0 in range(0, B, sb.group):
            sb.open_group(g0, max_sets=max([1] + [len(checkpoints(e["algo"], e["n_iter"], True)) for e in entries if watched(e)]))
            sb.convolve(g0)
            sb.mix(g0, sinr, snr, var, None if noise is None else [noise[b] for b in sb.rooms],
                   tuple(k[sb.rooms.start:sb.rooms.stop] for k in keys) if draw_noise else None)
            Xd = sb.take_mix()
            init = None
            if not monitor_convergence or any(e["algo"] == "auxiva_pca" for e in entries):
                init = sb.evaluate(Xd, True)                     # "init" is not an over-determined algorithm
            for e, res in zip(entries, results):
                res.append(_run_entry(sb, Xd, e, monitor_convergence, init))
        groups = [len(sb.room.group_rooms(g0)) for g0 in range(0, B, sb.group)]
        phase_ms = sb.phase_ms()                                 # (of the last group's last calls)
        sb.close_group()                                         # (the counts of the last group)
        _batch._info = {"algorithm": "sweep", "precision": "precise", "batched": B, "sharded": False, "n_mics": M, "n_targets": K,
                        "rooms_per_group": sb.group, "groups": groups, "algorithms": [e["name"] for e in entries],
                        "filter_length": int(filter_length), "phase_ms": phase_ms, "noise": sb.room.noise_source,
                        "evaluation": "bss_eval" if sb.groups_without_sets else "bss_eval_sets",
                        "groups_without_sets": sb.groups_without_sets, "reference_preparations": sb.reference_preparations,
                        "sets_evaluated": sb.sets_evaluated}
        n_samples = list(sb.out_lengths)
    out = []
    for e, per_group in zip(entries, results):
        marks, sdr, sir, sar, perm = _merge(per_group, K)
        row = {"algorithm": e["name"], "n_targets": K, "n_mics": M, "checkpoints": marks, "sdr": sdr, "sir": sir, "sar": sar,
               "perm": perm, "n_samples": n_samples, "runtime": float(sum(g[2] for g in per_group))}
        if e["algo"] == "ogive":
            row["epochs"] = [v for g in per_group for v in g[3]["epochs"]]
            row["converged"] = [v for g in per_group for v in g[3]["converged"]]
        out.append(row)
    return out
