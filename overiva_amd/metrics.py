"""``bss_eval_batch()`` and ``bss_eval_sources()``: SDR, SIR and SAR (BSS Eval v3, the "sources" criteria with a time-invariant
filter of ``filter_length`` taps; Vincent, Gribonval, Fevotte 2006) of B rooms per set of launches, in float64 on the device
(``oiva_bsseval_*``, csrc/kernels_bsseval.hip).

The reference's Monte-Carlo sweep measures every separation with ``mir_eval.separation.bss_eval_sources``
(``overiva_sim.py:210-231``), once per room and algorithm.  mir_eval is a third-party package whose source is not part of the
reference, so **the contract is the algorithm as DESIGN.md 3.10 states it**, checked against a NumPy/SciPy restatement written
from that statement (tests/helpers/bss_eval_oracle.py); bit parity with ``mir_eval`` is not pinned.

Per room, with the N*Lf references delayed by 0..Lf-1 samples: one Gram matrix G (symmetric, Toeplitz blocks) from direct
float64 lag sums, one Cholesky factorisation of G and one of each of its N diagonal blocks, 2N right-hand sides each, and five
quadratic forms per (estimate, reference) pair.  The energies of the time-domain decomposition (s_target, e_interf, e_artif)
follow without filtering any signal.  One difference from ``mir_eval`` in behaviour: where its ``np.linalg.solve`` fails it
falls back to ``lstsq``; here a room whose factorisation meets a pivot that is not finite or not above
``N * filter_length * eps * max_diag(G)`` (linearly dependent references) raises ``numpy.linalg.LinAlgError`` naming the room.
A room's bits do not depend on B, on its place in the batch or on the lengths of the other rooms.

``bss_eval_sets_batch()`` and ``bss_eval_sets()`` evaluate E sets of estimates against one set of references
(``oiva_bsssets_*``, the same kernels with a set axis): the lag sums of the references, G and its factors are made once per room and the
E sets go through one set of launches.  For every room and set the results have the bits of ``bss_eval_batch`` on that set alone.
"""
import ctypes as C
import itertools

import numpy as np

from . import _lib, sharded
from . import batch as _batch
from .overiva import get_device

MAX_SOURCES = 8
MAX_FILTER = 512
STAGES = ("correlate", "factor", "solve", "criteria")


def _check_signals(name, sig):
    """-> (list of B float64 C-contiguous (N, n_b) arrays, ragged)"""
    ragged = isinstance(sig, (list, tuple))
    if ragged:
        rooms = [np.asarray(a) for a in sig]
        if not rooms:
            raise ValueError(f"{name} is empty: bss_eval_batch needs at least one room")
        for b, a in enumerate(rooms):
            if a.ndim != 2:
                raise ValueError(f"{name}[{b}] has shape {a.shape}: every room must be (n_sources, n_samples)")
    else:
        arr = np.asarray(sig)
        if arr.ndim != 3:
            raise ValueError(f"{name} must have shape (batch, n_sources, n_samples), or be a sequence of (n_sources, n_samples_b) "
                             f"arrays; got shape {arr.shape}")
        if arr.shape[0] < 1:
            raise ValueError(f"{name} holds no room")
        rooms = list(arr)
    out = []
    for b, a in enumerate(rooms):
        if a.dtype.kind not in "fiu":
            raise ValueError(f"{name} must be real (float32, float64 or integer), got dtype {a.dtype} in room {b}")
        if a.shape[1] < 1:
            raise ValueError(f"{name}: room {b} has no samples")
        a = np.ascontiguousarray(a, dtype=np.float64)
        if not np.all(np.isfinite(a)):
            raise ValueError(f"{name}: room {b} holds non-finite samples")
        out.append(a)
    return out, ragged


def _check_args(reference_sources, estimated_sources, filter_length):
    if isinstance(filter_length, bool) or not isinstance(filter_length, (int, np.integer)) or not 1 <= filter_length <= MAX_FILTER:
        raise ValueError(f"filter_length must be an integer in 1..{MAX_FILTER}, got {filter_length!r}")
    ref, ragged = _check_signals("reference_sources", reference_sources)
    est, ragged_e = _check_signals("estimated_sources", estimated_sources)
    if ragged != ragged_e or len(ref) != len(est):
        raise ValueError("reference_sources and estimated_sources must have the same shapes")
    N = ref[0].shape[0]
    if not 1 <= N <= MAX_SOURCES:
        raise ValueError(f"bss_eval_batch runs on 1..{MAX_SOURCES} sources, got {N}")
    for b, (r, e) in enumerate(zip(ref, est)):
        if r.shape != e.shape:
            raise ValueError(f"room {b}: reference_sources has shape {r.shape}, estimated_sources {e.shape}: they must agree")
        if r.shape[0] != N:
            raise ValueError(f"room {b} has {r.shape[0]} sources, room 0 has {N}: the source count must agree")
        for name, a in (("reference", r), ("estimated", e)):
            zero = np.flatnonzero(~np.any(a != 0, axis=1))
            if zero.size:
                raise ValueError(f"room {b}: {name} source(s) {', '.join(str(i) for i in zero)} are all zeros: the criteria are "
                                 "not defined for a silent source")
    if sharded.active_group() is not None:
        raise ValueError("bss_eval_batch does not run under enable_bin_sharding(): disable bin sharding for batched calls")
    return ref, est, ragged, int(N), int(filter_length)


def best_permutation(sir):
    """the ``perm`` that maximises ``mean_j sir[perm[j], j]`` of one (N, N) SIR matrix [estimate, reference]; ties go to the
    first permutation in ``itertools.permutations(range(N))`` order"""
    sir = np.asarray(sir)
    N = sir.shape[0]
    cols = np.arange(N)
    best, best_mean = None, None
    for perm in itertools.permutations(range(N)):
        m = np.mean(sir[list(perm), cols])
        if best is None or m > best_mean:
            best, best_mean = perm, m
    return np.array(best, dtype=int)


class _BssHandle(_lib.Handle):
    """what ``BssEval`` and ``BssEvalSets`` share: B rooms of ``lengths[b]`` samples x N sources and one ``filter_length`` on one
    GPU.  A subclass names its C functions by ``_prefix`` and gives ``create`` its own last-but-one argument (``extra``)."""

    def __init__(self, lengths, N, filter_length, diag_only, extra, device, stream):
        lens = [int(n) for n in lengths]
        if not lens or min(lens) < 1:
            raise ValueError("at least one room of at least one sample is needed")
        if not 1 <= N <= MAX_SOURCES:
            raise ValueError(f"bss_eval runs on 1..{MAX_SOURCES} sources, got {N}")
        if not 1 <= filter_length <= MAX_FILTER:
            raise ValueError(f"filter_length must be in 1..{MAX_FILTER}, got {filter_length}")
        self.lib = _lib.load()
        self.lengths, self.B, self.N, self.Lf, self.diag_only = lens, len(lens), int(N), int(filter_length), bool(diag_only)
        self.device = get_device() if device is None else int(device)
        h = C.c_void_p()
        ns = (C.c_int * self.B)(*lens)
        _lib.check(self._fn("create")(C.byref(h), self.device, self.B, ns, self.N, self.Lf, int(self.diag_only), int(extra),
                                      C.c_void_p(stream) if stream else None))
        self.h = h

    def _fn(self, name):
        return getattr(self.lib, self._prefix + name)

    def _info(self, algorithm, rooms_per_group):
        out = {"algorithm": algorithm, "precision": "float64", "batched": self.B, "sharded": False, "n_sources": self.N,
               "filter_length": self.Lf, "rooms_per_group": rooms_per_group}
        if len(set(self.lengths)) > 1:
            out.update(ragged=True, lengths=list(self.lengths))
        else:
            out["n_samples"] = self.lengths[0]
        return out

    def _packed(self, name, sig):
        if len(sig) != self.B or any(np.shape(a) != (self.N, n) for a, n in zip(sig, self.lengths)):
            raise ValueError(f"{name} must be {self.B} arrays of shapes ({self.N}, n_b), n_b = {self.lengths}")
        return np.concatenate([np.ascontiguousarray(a, dtype=np.float64).ravel() for a in sig])

    def _gram(self, with_g, *set_index):
        nt = self.N * self.Lf
        G = np.empty((self.B, nt, nt)) if with_g else None
        D, E = np.empty((self.B, self.N, nt)), np.empty((self.B, self.N))
        _lib.check(self._fn("get_gram")(self.h, *set_index, None if G is None else _lib.ptr(G), _lib.ptr(D), _lib.ptr(E)))
        return G, D, E

    def _filters(self, *set_index):
        Cb, cs = np.empty((self.B, self.N, self.N * self.Lf)), np.empty((self.B, self.N, self.N, self.Lf))
        _lib.check(self._fn("get_filters")(self.h, *set_index, _lib.ptr(Cb), _lib.ptr(cs)))
        return Cb, np.ascontiguousarray(cs.transpose(0, 2, 1, 3))            # (the device keeps c as [room, j, k])

    def _criteria(self, shape, check, *sets):
        out = [np.empty(shape) for _ in range(3)]
        rc = self._fn("get_criteria")(self.h, *sets, *[_lib.ptr(a) for a in out])
        if rc != _lib.ERR_NUMERIC or check:
            _lib.check(rc)
        return tuple(out)

    def status(self):
        """(B,) bool: True where the room's factorisation was flagged"""
        st = (C.c_int * self.B)()
        _lib.check(self._fn("status")(self.h, st))
        return np.array(list(st), dtype=bool)


class BssEval(_BssHandle):
    """one handle = B rooms of ``lengths[b]`` samples x N sources and one ``filter_length`` on one GPU (``oiva_bsseval``).

    Stages: ``set_signals``, then ``correlate``, ``factor``, ``solve``, ``criteria`` in order (or ``run`` for all four, which
    also walks the room groups when the Gram matrices of all rooms do not fit the device at once; ``max_group`` asks for groups
    of at most that many rooms).  ``get_gram`` / ``get_filters`` / ``get_criteria`` / ``status`` read what the stages left."""

    _prefix = "oiva_bsseval_"
    _destroy = "oiva_bsseval_destroy"

    def __init__(self, lengths, N, filter_length=512, diag_only=False, max_group=0, device=None, stream=None):
        super().__init__(lengths, N, filter_length, diag_only, max_group, device, stream)
        g = C.c_int()
        _lib.check(self.lib.oiva_bsseval_groups(self.h, C.byref(g)))
        self.group = g.value

    def info(self):
        """what ``last_batch_info()`` reports after a run on this handle"""
        return self._info("bss_eval", self.group)

    def set_signals(self, ref, est):
        """ref, est: B arrays (N, n_b) each"""
        ref, est = self._packed("ref", ref), self._packed("est", est)
        _lib.check(self.lib.oiva_bsseval_set_signals(self.h, _lib.ptr(ref), _lib.ptr(est)))

    def stage(self, name):
        _lib.check(self.lib.oiva_bsseval_stage(self.h, STAGES.index(name)))

    def correlate(self):
        """the lag sums r_ij, D_k and E_k of every room"""
        self.stage("correlate")

    def factor(self):
        """G and its copy from the lag sums; Cholesky of the copy and of the N diagonal blocks"""
        self.stage("factor")

    def solve(self):
        """C_k = G^-1 D_k and c_kj = G_jj^-1 D_k[j]"""
        self.stage("solve")

    def criteria(self):
        """the quadratic forms and the three ratios of every evaluated pair"""
        self.stage("criteria")

    def run(self):
        _lib.check(self.lib.oiva_bsseval_run(self.h))

    def get_gram(self, with_g=True):
        """G (B, N Lf, N Lf) (None unless ``with_g``; needs ``factor``), D (B, N, N Lf), E (B, N)"""
        return self._gram(with_g)

    def get_filters(self):
        """the large solutions C (B, N[k], N Lf) and the small ones c (B, N[k], N[j], Lf): ``c[b, k, j] = G_jj^-1 D_k[j]``"""
        return self._filters()

    def get_criteria(self, check=True):
        """sdr, sir, sar (B, N, N) indexed [room, estimate, reference], NaN where a pair was not evaluated; with ``check`` a
        flagged room raises ``LinAlgError`` naming every such room"""
        return self._criteria((self.B, self.N, self.N), check)

    def time_stages(self, n):
        """n full runs with events around every stage: {stage: ms per run}"""
        ms = (C.c_float * len(STAGES))()
        _lib.check(self.lib.oiva_bsseval_time_stages(self.h, int(n), ms))
        return dict(zip(STAGES, list(ms)))


def bss_eval_batch(reference_sources, estimated_sources, compute_permutation=True, filter_length=512, return_matrices=False):
    """
    SDR, SIR and SAR of B rooms at once.

    Parameters
    ----------
    reference_sources, estimated_sources: ndarray (batch, n_sources, n_samples) real, or two sequences of B arrays
        (n_sources, n_samples_b) whose lengths may differ from room to room; 1..8 sources, the same for all rooms; float32,
        float64 or integer (all arithmetic is float64)
    compute_permutation: bool
        evaluate all N^2 (estimate, reference) pairs and choose, on the host, the ``perm`` that maximises
        ``mean_j sir[perm[j], j]`` (ties: the first in ``itertools.permutations`` order); otherwise only the pairs k = j
    filter_length: int, 1..512
        taps of the allowed distortion filter (``mir_eval`` hard-wires 512)
    return_matrices: bool
        also return the three (batch, n_sources, n_sources) matrices indexed [room, estimate, reference] (NaN off the diagonal
        without ``compute_permutation``)

    Returns
    -------
    sdr, sir, sar (batch, n_sources) float64 with ``sdr[b, j] = SDR[b, perm[b, j], j]``, and perm (batch, n_sources) int.  A zero
    denominator gives +inf; for one source the SIR is +inf.  A room whose Gram matrix is not positive definite to working
    precision raises ``numpy.linalg.LinAlgError`` naming every such room (``mir_eval`` would fall back to ``lstsq`` there).
    """
    ref, est, ragged, N, Lf = _check_args(reference_sources, estimated_sources, filter_length)
    B = len(ref)
    with BssEval([a.shape[1] for a in ref], N, Lf, diag_only=not compute_permutation) as ev:
        ev.set_signals(ref, est)
        ev.run()
        _batch._info = ev.info()
        mats = ev.get_criteria()                    # (raises LinAlgError naming the flagged rooms)
    cols = np.arange(N)
    if compute_permutation:
        perm = np.stack([best_permutation(mats[1][b]) for b in range(B)])
    else:
        perm = np.tile(cols, (B, 1))
    out = tuple(np.stack([m[b][perm[b], cols] for b in range(B)]) for m in mats) + (perm,)
    return out + mats if return_matrices else out


def bss_eval_sources(reference_sources, estimated_sources, compute_permutation=True, filter_length=512):
    """``mir_eval.separation.bss_eval_sources`` for one room: (n_sources, n_samples) references and estimates (a 1-D signal is
    one source) -> ``sdr, sir, sar, perm``: ``bss_eval_batch`` on a batch of one, without the batch axis"""
    ref, est = np.asarray(reference_sources), np.asarray(estimated_sources)
    if ref.ndim == 1:
        ref = ref[None]
    if est.ndim == 1:
        est = est[None]
    if ref.ndim != 2 or est.ndim != 2:
        raise ValueError("reference_sources and estimated_sources must have shape (n_sources, n_samples)")
    return tuple(o[0] for o in bss_eval_batch(ref[None], est[None], compute_permutation, filter_length))


SETS_PHASES = ("prepare", "correlate", "solve", "criteria")


class BssEvalSets(_BssHandle):
    """one handle = B rooms of ``lengths[b]`` samples x N sources, one ``filter_length`` and room for ``max_sets`` sets of
    estimates against one set of references on one GPU (``oiva_bsssets``).

    ``set_references`` (or ``take(..., with_references=True)``), then ``prepare`` once: the lag sums of the references, G, its
    Cholesky factor and those of its N diagonal blocks.  ``set_estimates(e, est)`` / ``take(handle, e)`` fill set e;
    ``evaluate(e0, n_sets)`` runs the estimate half of those sets in one set of launches.  All rooms are resident at once: a
    handle that does not fit the device fails to be created (``HipError``), and the caller makes smaller ones."""

    _prefix = "oiva_bsssets_"
    _destroy = "oiva_bsssets_destroy"

    def __init__(self, lengths, N, filter_length=512, diag_only=False, max_sets=1, device=None, stream=None):
        if int(max_sets) < 1:
            raise ValueError(f"max_sets must be >= 1, got {max_sets}")
        self.max_sets = int(max_sets)
        super().__init__(lengths, N, filter_length, diag_only, max_sets, device, stream)

    def info(self):
        """what ``last_batch_info()`` reports after a run on this handle"""
        prep, done = self.counts()
        return dict(self._info("bss_eval_sets", self.B), n_sets=self.max_sets, reference_preparations=prep, sets_evaluated=done)

    def set_references(self, ref):
        """ref: B arrays (N, n_b); drops the preparation"""
        _lib.check(self.lib.oiva_bsssets_set_references(self.h, _lib.ptr(self._packed("ref", ref))))

    def set_estimates(self, e, est):
        """est: B arrays (N, n_b), the estimates of set e"""
        _lib.check(self.lib.oiva_bsssets_set_estimates(self.h, int(e), _lib.ptr(self._packed("est", est))))

    def take(self, bss_eval_handle, e, with_references=False):
        """device to device from a ``BssEval`` whose signals are set: its estimates into set e, and its references too
        with ``with_references`` (which drops the preparation)"""
        _lib.check(self.lib.oiva_bsssets_take(self.h, bss_eval_handle.h, int(e), int(bool(with_references))))

    def prepare(self):
        """the reference half: lag sums r_ij, G, Cholesky of G and of its N diagonal blocks"""
        _lib.check(self.lib.oiva_bsssets_prepare(self.h))

    def evaluate(self, e0=0, n_sets=None):
        """the estimate half of sets e0 .. e0 + n_sets - 1 (default: all from e0 on) in one set of launches"""
        n_sets = self.max_sets - int(e0) if n_sets is None else int(n_sets)
        _lib.check(self.lib.oiva_bsssets_evaluate(self.h, int(e0), n_sets))

    def get_criteria(self, e0=0, n_sets=None, check=True):
        """sdr, sir, sar (B, n_sets, N, N) indexed [room, set, estimate, reference], NaN where a pair was not evaluated; with
        ``check`` a flagged room raises ``LinAlgError`` naming every such room"""
        n_sets = self.max_sets - int(e0) if n_sets is None else int(n_sets)
        return self._criteria((self.B, max(n_sets, 0), self.N, self.N), check, int(e0), n_sets)

    def get_gram(self, e, with_g=True):
        """G (B, N Lf, N Lf) (None unless ``with_g``), and D (B, N, N Lf), E (B, N) of the evaluated set e"""
        return self._gram(with_g, int(e))

    def get_filters(self, e):
        """of the evaluated set e, the large solutions C (B, N[k], N Lf) and the small ones c (B, N[k], N[j], Lf)"""
        return self._filters(int(e))

    def counts(self):
        """(preparations, sets evaluated) since the handle was made"""
        prep, done = C.c_longlong(), C.c_longlong()
        _lib.check(self.lib.oiva_bsssets_counts(self.h, C.byref(prep), C.byref(done)))
        return prep.value, done.value

    def phase_ms(self):
        """device ms of the last ``prepare`` and of the stages of the last ``evaluate``: {phase: ms}"""
        ms = (C.c_float * len(SETS_PHASES))()
        _lib.check(self.lib.oiva_bsssets_phase_ms(self.h, ms))
        return dict(zip(SETS_PHASES, list(ms)))


def _check_estimates(ref, ragged, N, estimated_sources):
    """what ``_check_args`` asks of the estimates, against references it has already checked -> B arrays (N, n_b)"""
    est, ragged_e = _check_signals("estimated_sources", estimated_sources)
    if ragged != ragged_e or len(ref) != len(est):
        raise ValueError("reference_sources and estimated_sources must have the same shapes")
    for b, (r, e) in enumerate(zip(ref, est)):
        if r.shape != e.shape:
            raise ValueError(f"room {b}: reference_sources has shape {r.shape}, estimated_sources {e.shape}: they must agree")
        zero = np.flatnonzero(~np.any(e != 0, axis=1))
        if zero.size:
            raise ValueError(f"room {b}: estimated source(s) {', '.join(str(i) for i in zero)} are all zeros: the criteria are "
                             "not defined for a silent source")
    return est


def _check_sets(reference_sources, estimated_sets, filter_length):
    """-> (ref: B arrays (N, n_b), sets: E lists of B arrays (N, n_b), N, Lf): set 0 goes through ``_check_args`` with the
    references, every further set through the same checks of the estimates; no set is copied"""
    ragged = isinstance(estimated_sets, (list, tuple))
    if ragged:
        rooms = [np.asarray(a) for a in estimated_sets]
        if not rooms:
            raise ValueError("estimated_sets is empty: bss_eval_sets_batch needs at least one room")
        for b, a in enumerate(rooms):
            if a.ndim != 3:
                raise ValueError(f"estimated_sets[{b}] has shape {a.shape}: every room must be (n_sets, n_sources, n_samples)")
    else:
        arr = np.asarray(estimated_sets)
        if arr.ndim != 4:
            raise ValueError("estimated_sets must have shape (batch, n_sets, n_sources, n_samples), or be a sequence of "
                             f"(n_sets, n_sources, n_samples_b) arrays; got shape {arr.shape}")
        if arr.shape[0] < 1:
            raise ValueError("estimated_sets holds no room")
        rooms = arr
    E = rooms[0].shape[0]
    if E < 1:
        raise ValueError("estimated_sets holds no set: n_sets must be >= 1")
    for b, a in enumerate(rooms):
        if a.shape[0] != E:
            raise ValueError(f"room {b} has {a.shape[0]} sets, room 0 has {E}: the set count must agree")
    ref = N = Lf = None
    sets = []
    for e in range(E):
        est_e = [a[e] for a in rooms] if ragged else rooms[:, e]           # (views)
        try:
            if e == 0:
                ref, est, ref_ragged, N, Lf = _check_args(reference_sources, est_e, filter_length)
            else:
                est = _check_estimates(ref, ref_ragged, N, est_e)
        except ValueError as err:
            raise ValueError(f"set {e}: {err}".replace("bss_eval_batch", "bss_eval_sets_batch")) from None
        sets.append(est)
    return ref, sets, N, Lf


def _is_out_of_memory(err):
    return isinstance(err, _lib.HipError) and "allocation failed" in str(err)


def bss_eval_sets_batch(reference_sources, estimated_sets, compute_permutation=True, filter_length=512, return_matrices=False,
                        max_group=0):
    """
    SDR, SIR and SAR of E sets of estimates of B rooms against one set of references per room: what ``bss_eval_batch`` gives on
    every set, bit for bit, with the work that depends on the references alone done once per room.

    Parameters
    ----------
    reference_sources: as in ``bss_eval_batch``
    estimated_sets: ndarray (batch, n_sets, n_sources, n_samples) real, or a sequence of B arrays
        (n_sets, n_sources, n_samples_b); n_sets >= 1, the same for every room
    compute_permutation, filter_length: as in ``bss_eval_batch``; the permutation is chosen per (room, set)
    return_matrices: bool
        also return the three (batch, n_sets, n_sources, n_sources) matrices indexed [room, set, estimate, reference]
    max_group: int
        0: all rooms in one handle; otherwise at most that many rooms per handle, one handle after the other.  When a handle
        cannot be created for lack of memory the group is halved.  A room's bits do not depend on the grouping.

    Returns
    -------
    sdr, sir, sar (batch, n_sets, n_sources) float64 and perm (batch, n_sets, n_sources) int.  A room whose Gram matrix is not
    positive definite to working precision raises ``numpy.linalg.LinAlgError`` naming every such room.
    """
    if isinstance(max_group, bool) or not isinstance(max_group, (int, np.integer)) or max_group < 0:
        raise ValueError(f"max_group must be an integer >= 0, got {max_group!r}")
    ref, sets, N, Lf = _check_sets(reference_sources, estimated_sets, filter_length)
    B, E = len(ref), len(sets)
    mats = [np.empty((B, E, N, N)) for _ in range(3)]
    flagged, info, preparations = [], None, 0
    group = B if max_group == 0 else min(B, int(max_group))
    b0 = 0
    while b0 < B:
        n = min(group, B - b0)
        try:
            ev = BssEvalSets([a.shape[1] for a in ref[b0:b0 + n]], N, Lf, diag_only=not compute_permutation, max_sets=E)
        except _lib.HipError as err:
            if not _is_out_of_memory(err) or group == 1:
                raise
            group = (group + 1) // 2
            continue
        with ev:
            ev.set_references(ref[b0:b0 + n])
            ev.prepare()
            for e in range(E):
                ev.set_estimates(e, sets[e][b0:b0 + n])
            ev.evaluate(0, E)
            part = ev.get_criteria(0, E, check=False)
            flagged += [b0 + int(b) for b in np.flatnonzero(ev.status())]
            preparations += ev.counts()[0]
            if info is None:
                info = ev.info()
        for m, p in zip(mats, part):
            m[b0:b0 + n] = p
        b0 += n
    lens = [a.shape[1] for a in ref]
    info.update(batched=B, rooms_per_group=group, n_sets=E, reference_preparations=preparations, sets_evaluated=E * preparations)
    info.pop("n_samples", None), info.pop("ragged", None), info.pop("lengths", None)
    if len(set(lens)) > 1:
        info.update(ragged=True, lengths=lens)
    else:
        info["n_samples"] = lens[0]
    _batch._info = info
    if flagged:
        raise np.linalg.LinAlgError("the Gram matrix of the delayed references is not positive definite to working precision "
                                    "(linearly dependent references) in problem(s) " + ", ".join(str(b) for b in flagged))
    cols = np.arange(N)
    if compute_permutation:
        perm = np.array([[best_permutation(mats[1][b, e]) for e in range(E)] for b in range(B)]).reshape(B, E, N)
    else:
        perm = np.tile(cols, (B, E, 1))
    out = tuple(np.array([[m[b, e][perm[b, e], cols] for e in range(E)] for b in range(B)]).reshape(B, E, N) for m in mats) + (perm,)
    return out + tuple(mats) if return_matrices else out


def bss_eval_sets(reference_sources, estimated_sets, compute_permutation=True, filter_length=512):
    """``bss_eval_sets_batch`` for one room: (n_sources, n_samples) references and (n_sets, n_sources, n_samples) estimates ->
    ``sdr, sir, sar, perm``, each (n_sets, n_sources): a batch of one, without the batch axis"""
    ref, est = np.asarray(reference_sources), np.asarray(estimated_sets)
    if ref.ndim != 2 or est.ndim != 3:
        raise ValueError("reference_sources must have shape (n_sources, n_samples) and estimated_sets (n_sets, n_sources, n_samples)")
    return tuple(o[0] for o in bss_eval_sets_batch(ref[None], est[None], compute_permutation, filter_length))
