"""``overiva_batch()``: many same-shape OverIVA problems per set of launches (``oiva_batch``, csrc/kernels_batch.hip),
``overiva_batch_ragged()``, the same on problems of different frame counts (one path: a same-shape batch is the case of equal
frame counts), and ``ogive_batch()``, OGIVE on same-shape problems with a stopping rule per problem
(csrc/kernels_ogive_batch.hip).

The reference's own calls separate 10-second rooms -- 2049 bins x 160-235 frames x 2-8 microphones -- one ``overiva()`` call
each, and a single call of that size leaves the GPU mostly idle (every kernel is a few workgroup lifetimes long, and a launch
costs 4-5 us of each).  ``overiva_batch(X)`` takes B such problems as one (B, T, F, M) array and runs every stage for all of them
at once: the iteration is four launches whatever B, replayed from one captured graph.  Problem ``b``'s result is that of
``overiva(X[b], ...)`` with the same arguments in the ``precise`` arithmetic, and its bits do not depend on B or on its place in
the batch.

``data="complex128"`` (``overiva_batch``, ``overiva_batch_ragged``, ``BatchPlan``, ``RaggedBatchPlan``) is the opt-in complex128
data path: X is held on the device as the caller's complex128 and every stage -- powers, activations, the scale of W, both
covariances, the per-bin algebra, Y and the projection back -- runs in float64 (csrc/kernels_batch_c128.hip): the
reference's complex128 arithmetic on the reference's complex128 data.  It has its own bits (not those of the default path on
complex64-representable input) and the same independence of B and of the room's place.

Arithmetic: always ``precise`` (float64 sums of exact float64 products in the covariance passes, float64 per-bin algebra, W_hat
carried in complex128) -- what ``"auto"`` picks for these call sizes anyway; ``set_precision()`` does not change it.  X lives on
the device as complex64 and complex128 input is converted on the device, unless ``data="complex128"`` is given.
"""
import ctypes as C
import sys

import numpy as np

from . import _lib, sharded
from . import ive as _ive
from .overiva import _complex_dtype, get_device

_overiva_module = sys.modules[__package__ + ".overiva"]   # (the package's attribute `overiva` is the function)
MAX_CHANNELS = 8
DATA_MODES = ("complex64", "complex128")
ILRMA_STAGES = ("t_update", "v_update", "r_rewrite", "weighted_cov", "ip_update", "power", "normalise")   # OIVA_ILRMA_STAGE_*
ISS_STAGES = ("activation", "sweep")   # OIVA_ISS_STAGE_*
ISS_MAX_SLAB = 8192                    # frames x channels of one room at most: one bin's complex128 slab of 128 KiB of LDS
FIVE_STAGES = ("power", "activation", "cov", "update")   # OIVA_FIVE_STAGE_*
IP2_STAGES = ("power", "activation", "cov", "update")    # OIVA_IP2_STAGE_*
_info = {}


def last_batch_info():
    """what the last batched call ran: ``{"precision": "precise", "batched": B, "data": "complex64" | "complex128", ...}``; after ``auxiva_pca_batch()`` also
    ``algorithm`` ("auxiva_pca") and ``reduced`` (the channel count of the inner solve); after
    ``ogive_batch()`` also ``epochs`` (B ints: epochs each problem ran) and ``converged`` (B bools: its stopping rule fired); after
    ``ilrma_batch()`` also ``algorithm`` ("ilrma") and ``n_components``; after ``auxiva_iss_batch()`` ``algorithm`` ("auxiva_iss"); after ``five_batch()`` ``algorithm`` ("five"); after
    ``overiva_batch_ragged()`` also ``ragged`` (True) and ``frames`` (B ints), ``shape`` then holding the largest T; after
    ``bss_eval_batch()`` ``algorithm`` ("bss_eval"), ``batched``, ``n_sources``, ``filter_length`` and, for rooms of different
    lengths, ``ragged`` (True) and ``lengths`` (B ints); after ``sweep_batch()`` ``algorithm`` ("sweep"), ``batched``,
    ``rooms_per_group``, ``groups`` (the group sizes), ``algorithms`` (the entries that ran) and ``phase_ms``"""
    return dict(_info)


class DeviceBatch:
    """A complex64 array in the memory of this process's GPU in the layout of a batch plan: ``shape`` (B, T, F, C) when ``dense``,
    else packed (sum T_b, F, C); ``frames`` the B frame counts, ``n_freq`` F, ``ptr`` the device address, ``owner`` whatever
    keeps it alive.  ``get_x()`` copies it to the host."""

    def __init__(self, ptr, frames, n_freq, n_chan, dense, owner=None):
        self.ptr = int(ptr)
        self.frames = [int(t) for t in frames]
        self.n_freq, self.n_chan, self.dense = int(n_freq), int(n_chan), bool(dense)
        self.owner = owner
        total = sum(self.frames)
        self.shape = (len(self.frames), self.frames[0], self.n_freq, self.n_chan) if dense else (total, self.n_freq, self.n_chan)
        self.dtype = np.dtype(np.complex64)

    def get_x(self):
        """the (B, T, F, C) host array of a dense batch, or the list of B (T_b, F, C) arrays"""
        out = np.empty(self.shape, np.complex64)
        _lib.check(_lib.load().oiva_device_to_host(_lib.ptr(out), C.c_void_p(self.ptr), out.nbytes))
        if self.dense:
            return out
        off = np.concatenate([[0], np.cumsum(self.frames)]).astype(int)
        return [out[off[b]:off[b + 1]] for b in range(len(self.frames))]


class BatchPlan(_lib.Handle):
    """Owns the device state of B problems of shape (T, F, M) with K sources (``oiva_batch``).

    Stages as ``Plan``'s: ``set_x``, ``covariance``, ``set_w`` / ``set_w_eig``, ``iterate``, ``demix``, ``get_w``; ``status``
    reports which problems hold a non-finite W.  ``set_w_pca`` / ``project_device`` / ``compose_w`` are the PCA front end of
    ``auxiva_pca_batch()`` (pca_batch.py).  With K = 1, ``ogive_begin`` / ``ogive_iterate`` run OGIVE instead of
    ``iterate`` (``get_cx`` reads the input covariance for the host's ``init_eig``).  With K = M, ``ilrma_begin`` /
    ``ilrma_iterate`` run ILRMA (ilrma.py); ``ilrma_stage`` runs one stage of an epoch, ``get_nmf`` reads the source model.
    With K = M, ``iss_begin`` / ``iss_iterate`` run determined AuxIVA by rank-1 ISS updates (iss.py), on a ragged plan too;
    ``iss_stage`` runs one stage of an iteration.  With K = 1, ``five_begin`` / ``five_iterate`` run FIVE (five.py), on a ragged
    plan too; ``five_stage`` runs one stage of an iteration, ``get_five_reduction`` reads the reduction of the pencil.

    On the device X and Y are packed along the frames, (sum T_b, F, .): ``frames`` holds the B frame counts (here B times T)
    and ``offsets`` every problem's first frame.

    ``data="complex128"``: X is held as complex128 and every stage runs in float64.  ``set_x`` then takes complex128 only and
    uploads it as it is, ``set_x_device`` borrows a complex128 device array, ``demix(dtype=np.complex128)`` returns what the
    device computed and ``demix(dtype=np.complex64)`` its rounded copy.  OGIVE, ILRMA, the PCA entry points and ``demix_device``
    raise ``ValueError`` on such a plan; ``get_weights`` / ``get_weighted_cov`` read the last iteration's stages back."""

    _destroy = "oiva_batch_destroy"
    dense = True          # X and Y are handed over as one (B, T, F, .) array
    n_components = 0      # columns of the ILRMA source model, set by ilrma_begin
    data = "complex64"    # the data path: "complex128" holds X as complex128 and runs every stage in float64

    def __init__(self, B, T, F, M, K, model="laplace", device=None, stream=None, data="complex64"):
        self._open([int(T)] * int(B), int(T), F, M, K, model, device, stream, data)

    def _open(self, frames, T, F, M, K, model, device, stream, data="complex64"):
        if model not in _lib.MODEL_IDS:
            raise ValueError(f"model must be 'laplace' or 'gauss', got {model!r}")
        _check_data(data)
        self.data = data
        self.lib = _lib.load()
        self.frames = frames
        self.offsets = np.concatenate([[0], np.cumsum(frames)]).astype(int)
        self.B, self.T, self.F, self.M, self.K = len(frames), T, int(F), int(M), int(K)
        self.model = model
        self.device = get_device() if device is None else int(device)
        h = C.c_void_p()
        _lib.check(self._create(h, C.c_void_p(stream) if stream else None))
        self.h = h
        self._keep = None
        if data == "complex128":
            _lib.check(self.lib.oiva_batch_set_data_c128(self.h))

    def _no_c128(self, what):
        if self.data == "complex128":
            raise ValueError(f"{what} does not run on a complex128 plan (data='complex128'): use the default data='complex64'")

    def _create(self, h, stream):
        return self.lib.oiva_batch_create(C.byref(h), self.device, self.B, self.T, self.F, self.M, self.K,
                                          _lib.MODEL_IDS[self.model], stream)

    @property
    def shape(self):
        return (self.B, self.T, self.F, self.M)

    def info(self):
        """what ``last_batch_info()`` reports after a run on this plan"""
        return {"precision": "precise", "batched": self.B, "sharded": False, "shape": (self.T, self.F, self.M, self.K),
                "data": self.data}

    def set_x(self, X):
        """X: (B, T, F, M) complex64 or complex128 host array (complex128 is converted on the device); on a complex128 plan
        complex128 only, uploaded as it is"""
        X = np.asarray(X)
        if X.shape != self.shape:
            raise ValueError(f"X has shape {X.shape}, batch expects {self.shape}")
        _check_data(self.data, X.dtype)
        if X.dtype != np.complex128:
            X = np.ascontiguousarray(X, dtype=np.complex64)
        else:
            X = np.ascontiguousarray(X)
        _lib.check(self.lib.oiva_batch_set_x_host(self.h, _lib.ptr(X), 1 if X.dtype == np.complex128 else 0))

    def set_x_device(self, dev_ptr, keepalive=None):
        """borrow a complex64 device array of ``shape`` (e.g. a torch tensor's data_ptr()); on a complex128 plan a complex128 one"""
        self._keep = keepalive
        _lib.check(self.lib.oiva_batch_set_x_dev(self.h, C.c_void_p(int(dev_ptr))))

    def covariance(self):
        _lib.check(self.lib.oiva_batch_covariance(self.h))

    def get_cx(self, dtype=np.complex128):
        """input covariance (B, F, M, M); the device holds it in float64"""
        out = np.empty((self.B, self.F, self.M, self.M), dtype)
        _lib.check(self.lib.oiva_batch_get_cx(self.h, _lib.ptr(out), 1 if out.dtype == np.complex128 else 0))
        return out

    def set_w(self, W0=None):
        """W0: None (identity), broadcastable to (F, M, K) (one start for every problem), or (B, F, M, K)"""
        if W0 is None:
            _lib.check(self.lib.oiva_batch_set_w(self.h, None, 0))
            return
        W0 = np.asarray(W0)
        dt = np.complex64 if W0.dtype == np.complex64 else np.complex128
        W0 = np.ascontiguousarray(np.broadcast_to(W0, (self.B, self.F, self.M, self.K)), dtype=dt)
        _lib.check(self.lib.oiva_batch_set_w(self.h, _lib.ptr(W0), 1 if dt == np.complex128 else 0))

    def set_w_eig(self):
        _lib.check(self.lib.oiva_batch_set_w_eig(self.h))

    def set_w_pca(self, return_eigenvalues=False):
        """W = the K principal eigenvectors of every bin's input covariance, ascending (the reference's ``w[:, :, -K:]``,
        auxiva_pca.py:75-81), from the Jacobi eigensolver on the device; optionally returns all eigenvalues (B, F, M), ascending"""
        self._no_c128("set_w_pca")
        ev = np.empty((self.B, self.F, self.M), np.float64) if return_eigenvalues else None
        _lib.check(self.lib.oiva_batch_set_w_pca(self.h, _lib.ptr(ev) if ev is not None else None))
        return ev

    def project_device(self):
        """x -> W^H x for every problem in one launch (auxiva_pca.py:79-81 after ``set_w_pca``): a ``DeviceBatch`` of K channels in
        a device array of this plan that ``demix`` does not write, valid until the next ``project_device`` on the plan"""
        self._no_c128("project_device")
        dev = C.c_void_p()
        _lib.check(self.lib.oiva_batch_project_dev(self.h, C.byref(dev)))
        return DeviceBatch(dev.value, self.frames, self.F, self.K, self.dense, owner=self)

    def compose_w(self, inner):
        """W[:, :K] <- W[:, :K] @ W_red on the device in float64, W_red the (K, K) matrices of ``inner``, the determined plan that
        ran on ``project_device()``'s output: y = W_red^H (P^H x) = (P W_red)^H x"""
        if not isinstance(inner, BatchPlan) or inner is self:
            raise ValueError("compose_w takes the plan of the reduced problems")
        self._no_c128("compose_w")
        inner._no_c128("compose_w")
        if (inner.B, inner.F) != (self.B, self.F):
            raise ValueError(f"the reduced plan holds {inner.B} problems of {inner.F} bins, this one {self.B} of {self.F}")
        if not inner.M == inner.K == self.K:
            raise ValueError(f"the reduced plan must be determined on {self.K} channels, it has {inner.M} channels and {inner.K} sources")
        _lib.check(self.lib.oiva_batch_compose_w(self.h, inner.h))

    def iterate(self, n=1):
        _lib.check(self.lib.oiva_batch_iterate(self.h, int(n)))

    def ogive_begin(self, update="demix", model="laplace"):
        self._no_c128("OGIVE")
        _lib.check(self.lib.oiva_batch_ogive_begin(self.h, _ive.UPDATE_IDS[update], _lib.MODEL_IDS[model]))

    def ogive_iterate(self, first_epoch, n, step_size=0.1, tol=1e-3):
        """up to n epochs; returns, per problem, (epochs of this call that changed its state, stopping rule met, max ||delta|| of
        its last epoch) as (B,) arrays"""
        self._no_c128("OGIVE")
        ran, conv, md = (C.c_int * self.B)(), (C.c_int * self.B)(), (C.c_double * self.B)()
        _lib.check(self.lib.oiva_batch_ogive_iterate(self.h, int(first_epoch), int(n), float(step_size), float(tol), ran, conv, md))
        return np.array(list(ran), dtype=int), np.array(list(conv), dtype=bool), np.array(list(md))

    def ilrma_begin(self, T0, V0):
        """start ILRMA (needs K = M, X, the covariance and W set): T0 (B, K, F, L) and V0 (B, K, L, T) float64, strictly
        positive; forms R = T0 V0 and P = |y|^2 from the current W"""
        self._no_c128("ILRMA")
        T0 = np.ascontiguousarray(T0, dtype=np.float64)
        V0 = np.ascontiguousarray(V0, dtype=np.float64)
        if T0.ndim != 4 or T0.shape[:3] != (self.B, self.K, self.F) or V0.shape != (self.B, self.K, T0.shape[3], self.T):
            raise ValueError(f"T0 must be {(self.B, self.K, self.F, 'L')} and V0 {(self.B, self.K, 'L', self.T)}, got {T0.shape} and {V0.shape}")
        _lib.check(self.lib.oiva_batch_ilrma_begin(self.h, T0.shape[3], _lib.ptr(T0), _lib.ptr(V0)))
        self.n_components = int(T0.shape[3])

    def ilrma_iterate(self, n=1):
        self._no_c128("ILRMA")
        _lib.check(self.lib.oiva_batch_ilrma_iterate(self.h, int(n)))

    def ilrma_stage(self, stage):
        """one stage of an epoch: a name of ``ILRMA_STAGES`` or its index"""
        self._no_c128("ILRMA")
        _lib.check(self.lib.oiva_batch_ilrma_stage(self.h, ILRMA_STAGES.index(stage) if isinstance(stage, str) else int(stage)))

    def get_nmf(self):
        """(Tn (B, K, F, L), Vn (B, K, L, T)) of the ILRMA source model"""
        Tn = np.empty((self.B, self.K, self.F, self.n_components))
        Vn = np.empty((self.B, self.K, self.n_components, self.T))
        _lib.check(self.lib.oiva_batch_ilrma_get_nmf(self.h, _lib.ptr(Tn), _lib.ptr(Vn)))
        return Tn, Vn

    def get_pr(self):
        """test hook: (P, R), both (B, K, F, T): the source powers |y|^2 and the model Tn Vn as the device holds them"""
        P = np.empty((self.B, self.K, self.F, self.T))
        R = np.empty_like(P)
        _lib.check(self.lib.oiva_batch_ilrma_get_pr(self.h, _lib.ptr(P), _lib.ptr(R)))
        return P, R

    def get_ilrma_cov(self):
        """test hook: (C (B, F, K, M*M), lambda (B, K)): the packed Hermitian partials of the last covariance stage added over
        the frame splits (not divided by T) and the scales of the last normalisation"""
        Cp = np.empty((self.B, self.F, self.K, self.M * self.M))
        lam = np.empty((self.B, self.K))
        _lib.check(self.lib.oiva_batch_ilrma_get_cov(self.h, _lib.ptr(Cp), _lib.ptr(lam)))
        return Cp, lam

    def ilrma_time_stages(self, n):
        """n epochs with events around every stage: {stage: ms per epoch}; advances the state"""
        arr = (C.c_float * len(ILRMA_STAGES))()
        _lib.check(self.lib.oiva_batch_ilrma_time_stages(self.h, int(n), arr))
        return dict(zip(ILRMA_STAGES, list(arr)))

    def iss_begin(self):
        """start ISS (iss.py; needs K = M, X and W set, ``T_b * M <= 8192`` in every room): forms the source powers of the
        current W"""
        self._no_c128("ISS")
        _lib.check(self.lib.oiva_batch_iss_begin(self.h))

    def iss_iterate(self, n=1):
        self._no_c128("ISS")
        _lib.check(self.lib.oiva_batch_iss_iterate(self.h, int(n)))

    def iss_stage(self, stage):
        """one stage of an iteration: a name of ``ISS_STAGES`` or its index"""
        self._no_c128("ISS")
        _lib.check(self.lib.oiva_batch_iss_stage(self.h, ISS_STAGES.index(stage) if isinstance(stage, str) else int(stage)))

    def iss_sweep_steps(self, n_steps):
        """test hook: the sweep with its first ``n_steps`` rank-1 steps only (0: demix and powers)"""
        self._no_c128("ISS")
        _lib.check(self.lib.oiva_batch_iss_sweep_steps(self.h, int(n_steps)))

    def _iss_frames_by_k(self, fn):
        out = np.empty((int(self.offsets[-1]), self.K), np.float64)
        _lib.check(fn(self.h, _lib.ptr(out)))
        return out.reshape(self.B, self.T, self.K) if self.dense else out

    def get_iss_weights(self):
        """test hook: the weights 1 / max(r / gamma, eps) of the last ISS activation, (B, T, K) float64, or packed
        (sum T_b, K) on a ragged plan"""
        return self._iss_frames_by_k(self.lib.oiva_batch_iss_get_weights)

    def get_iss_powers(self):
        """test hook: the source powers sum_f |y|^2 the last ISS sweep left, shaped as ``get_iss_weights``"""
        return self._iss_frames_by_k(self.lib.oiva_batch_iss_get_powers)

    def iss_time_stages(self, n):
        """n iterations with events around every stage: {stage: ms per iteration}; advances the state"""
        arr = (C.c_float * len(ISS_STAGES))()
        _lib.check(self.lib.oiva_batch_iss_time_stages(self.h, int(n), arr))
        return dict(zip(ISS_STAGES, list(arr)))

    def five_begin(self):
        """start FIVE (five.py; needs K = 1, X, the covariance and W set): forms the complex128 copy of X its float64 stages
        stream and the reduction of every bin's input covariance; afterwards ``demix(dtype=np.complex128)`` forms Y in float64"""
        self._no_c128("FIVE")
        _lib.check(self.lib.oiva_batch_five_begin(self.h))

    def five_iterate(self, n=1):
        self._no_c128("FIVE")
        _lib.check(self.lib.oiva_batch_five_iterate(self.h, int(n)))

    def five_stage(self, stage):
        """one stage of an iteration: a name of ``FIVE_STAGES`` or its index"""
        self._no_c128("FIVE")
        _lib.check(self.lib.oiva_batch_five_stage(self.h, FIVE_STAGES.index(stage) if isinstance(stage, str) else int(stage)))

    def get_five_reduction(self):
        """test hook: Li (B, F, M, M) complex128 with Li Cx Li^H = I, the inverse of the lower Cholesky factor of every bin's Cx"""
        self._no_c128("FIVE")
        out = np.empty((self.B, self.F, self.M, self.M), np.complex128)
        _lib.check(self.lib.oiva_batch_five_get_reduction(self.h, _lib.ptr(out)))
        return out

    def five_time_stages(self, n):
        """n iterations with events around every stage: {stage: ms per iteration}; advances the state"""
        self._no_c128("FIVE")
        arr = (C.c_float * len(FIVE_STAGES))()
        _lib.check(self.lib.oiva_batch_five_time_stages(self.h, int(n), arr))
        return dict(zip(FIVE_STAGES, list(arr)))

    def ip2_iterate(self, first, n=1):
        """iterations ``first .. first + n - 1`` of IP2 (ip2.py; needs X, the covariance and W set): the index of an iteration,
        counted from the start of the separation, selects its schedule, so a run may be cut into calls anywhere"""
        self._no_c128("IP2")
        _lib.check(self.lib.oiva_batch_ip2_iterate(self.h, int(first), int(n)))

    def ip2_stage(self, stage, iteration=0):
        """one stage of iteration ``iteration``: a name of ``IP2_STAGES`` or its index"""
        self._no_c128("IP2")
        _lib.check(self.lib.oiva_batch_ip2_stage(self.h, IP2_STAGES.index(stage) if isinstance(stage, str) else int(stage),
                                                 int(iteration)))

    def ip2_time_stages(self, n):
        """iterations 0 .. n - 1 with events around every stage: {stage: ms per iteration}; advances the state"""
        self._no_c128("IP2")
        arr = (C.c_float * len(IP2_STAGES))()
        _lib.check(self.lib.oiva_batch_ip2_time_stages(self.h, int(n), arr))
        return dict(zip(IP2_STAGES, list(arr)))

    def _demix_packed(self, proj_back, dtype):
        out = np.empty((int(self.offsets[-1]), self.F, self.K), dtype)
        _lib.check(self.lib.oiva_batch_demix(self.h, _lib.ptr(out), 1 if out.dtype == np.complex128 else 0, 1 if proj_back else 0))
        return out

    def demix(self, proj_back=True, dtype=np.complex64):
        """Y (B, T, F, K) in complex64 or complex128; on a complex128 plan complex128 is what the device computed in float64
        and complex64 its rounded copy"""
        return self._demix_packed(proj_back, dtype).reshape(self.B, self.T, self.F, self.K)

    def demix_device(self, proj_back=True):
        """Y stays on the device: a ``DeviceBatch`` (B, T, F, K), or packed (sum T_b, F, K) on a ragged plan; valid until the next
        call on the plan (the contract of ``Plan.demix_device``).  A ``DeviceBatch`` and its consumers are complex64: refused on
        a complex128 plan"""
        self._no_c128("demix_device")
        dev = C.c_void_p()
        _lib.check(self.lib.oiva_batch_demix_dev(self.h, 1 if proj_back else 0, C.byref(dev)))
        return DeviceBatch(dev.value, self.frames, self.F, self.K, self.dense, owner=self)

    def get_w(self, dtype=np.complex128, check=True):
        """W (B, F, M, K); with ``check`` a non-finite W of any problem raises ``LinAlgError`` naming them"""
        out = np.empty((self.B, self.F, self.M, self.K), dtype)
        rc = self.lib.oiva_batch_get_w(self.h, _lib.ptr(out), 1 if out.dtype == np.complex128 else 0)
        if rc != _lib.ERR_NUMERIC or check:
            _lib.check(rc)
        return out

    def status(self):
        """(B,) bool: True where the problem's W holds a non-finite value"""
        st = (C.c_int * self.B)()
        _lib.check(self.lib.oiva_batch_status(self.h, st))
        return np.array(list(st), dtype=bool)

    def get_weights(self):
        """test hook of a complex128 plan: the activation weights 1 / max(r / gamma, eps) of the last iteration, (B, T, K)
        float64, or packed (sum T_b, K) on a ragged plan"""
        out = np.empty((int(self.offsets[-1]), self.K), np.float64)
        _lib.check(self.lib.oiva_batch_c128_get_weights(self.h, _lib.ptr(out)))
        return out.reshape(self.B, self.T, self.K) if self.dense else out

    def get_weighted_cov(self):
        """test hook: the weighted covariances V of the last iteration (of the last ``cov`` stage of FIVE), every room's frame
        splits added in order and divided by its T: (B, F, K, M, M) complex128; on either data path"""
        out = np.empty((self.B, self.F, self.K, self.M, self.M), np.complex128)
        _lib.check(self.lib.oiva_batch_c128_get_cov(self.h, _lib.ptr(out)))
        return out

    def time_stages(self, n):
        """n eager iterations with events around every stage (ms per iteration per stage), and ms per iteration of a replayed
        graph of n (<= 32) iterations; both advance the state"""
        total = C.c_float()
        arr = (C.c_float * _lib.N_STAGES)()
        _lib.check(self.lib.oiva_batch_time_stages(self.h, int(n), C.byref(total), arr))
        return total.value, dict(zip(_lib.STAGE_NAMES, list(arr)))


def _check_data(data, dtype=None):
    """``data`` names a data path; with ``dtype``: the complex128 path takes complex128 input only"""
    if data not in DATA_MODES:
        raise ValueError(f"data must be one of {DATA_MODES}, got {data!r}")
    if data == "complex128" and dtype is not None and np.dtype(dtype) != np.complex128:
        raise ValueError(f"data='complex128' needs complex128 input, got {np.dtype(dtype)}")


def _check_common(name, found, B, F, M, n_src, model, W0, n_iter, update=None, bool_counts=True, w0_reduced=False):
    """what the batched entry points check once the shapes are known (``name`` of the entry point, ``found``: how its message
    names the channel count it met; ``bool_counts``: ``n_src=True`` is one source, as ``overiva_batch`` has always taken it;
    ``w0_reduced``: W0 starts the determined solve on K channels of ``auxiva_pca_batch``, (F, K, K)); returns K"""
    if not 1 <= M <= MAX_CHANNELS:
        raise ValueError(f"{name} runs on 1..{MAX_CHANNELS} channels, {found} {M}")
    K = M if n_src is None else n_src
    if (isinstance(K, bool) and not bool_counts) or not isinstance(K, (int, np.integer)) or not 1 <= K <= M:
        raise ValueError(f"n_src must be in 1..{M}")
    if model not in ("laplace", "gauss"):
        raise ValueError(f"model must be 'laplace' or 'gauss', got {model!r}")
    if update is not None and update not in _ive.UPDATE_IDS:
        raise ValueError(f"update must be one of {sorted(_ive.UPDATE_IDS)}, got {update!r}")
    if n_iter < 0:
        raise ValueError("n_iter must be >= 0")
    _check_w0(W0, B, F, K if w0_reduced else M, K)
    if sharded.active_group() is not None:
        raise ValueError(f"{name} does not run under enable_bin_sharding(): disable bin sharding for batched calls")
    return int(K)


def _check_w0(W0, B, F, M, K):
    """W0: None, broadcastable to (F, M, K), or (B, F, M, K)"""
    if W0 is None:
        return
    W0 = np.asarray(W0)
    try:
        shared = np.broadcast_shapes(W0.shape, (F, M, K)) == (F, M, K)
    except ValueError:
        shared = False
    if not shared and W0.shape != (B, F, M, K):
        raise ValueError(f"W0 has shape {W0.shape}: expected one broadcastable to {(F, M, K)} or {(B, F, M, K)}")


def _check_dense_x(X):
    X = np.asarray(X)
    if X.ndim != 4:
        raise ValueError("X must have shape (batch, n_frames, n_freq, n_chan)")
    dtype = _complex_dtype(X)
    B, T, F, M = X.shape
    if B < 1 or T < 1 or F < 1:
        raise ValueError(f"X has shape {X.shape}: every dimension must be >= 1")
    return X, dtype


def _check_args(X, n_src, model, W0, n_iter):
    X, dtype = _check_dense_x(X)
    B, T, F, M = X.shape
    return X, dtype, _check_common("overiva_batch", "X has", B, F, M, n_src, model, W0, n_iter)


def _check_ogive_args(X, update, model, W0, n_iter):
    X, dtype = _check_dense_x(X)
    B, T, F, M = X.shape
    _check_common("ogive_batch", "X has", B, F, M, 1, model, W0, n_iter, update=update)
    return X, dtype


def _check_ragged_xs(Xs, name="overiva_batch_ragged"):
    """the list of problems as arrays, their common complex dtype"""
    if not hasattr(Xs, "__len__"):
        raise ValueError("Xs must be a sequence of (n_frames, n_freq, n_chan) arrays")
    Xs = [np.asarray(x) for x in Xs]
    if not Xs:
        raise ValueError(f"Xs is empty: {name} needs at least one problem")
    for b, x in enumerate(Xs):
        if x.ndim != 3:
            raise ValueError(f"Xs[{b}] has shape {x.shape}: every problem must be (n_frames, n_freq, n_chan)")
    dtypes = {x.dtype for x in Xs}
    if len(dtypes) != 1:
        raise ValueError(f"the problems have mixed dtypes {sorted(str(d) for d in dtypes)}: give them one complex dtype")
    dtype = _complex_dtype(Xs[0])
    F, M = Xs[0].shape[1:]
    for b, x in enumerate(Xs):
        if x.shape[1:] != (F, M):
            raise ValueError(f"Xs[{b}] has {x.shape[1]} bins and {x.shape[2]} channels, Xs[0] {F} and {M}: F and M must agree")
        if x.shape[0] < 1:
            raise ValueError(f"Xs[{b}] has {x.shape[0]} frames: every problem needs at least one")
    if F < 1:
        raise ValueError("every problem needs at least one frequency bin")
    return Xs, dtype


def _check_ragged_args(Xs, n_src, model, W0, n_iter):
    Xs, dtype = _check_ragged_xs(Xs)
    F, M = Xs[0].shape[1:]
    return Xs, dtype, _check_common("overiva_batch_ragged", "the problems have", len(Xs), F, M, n_src, model, W0, n_iter,
                                    bool_counts=False)


def _run_overiva(plan, X, dtype, n_iter, proj_back, W0, init_eig, return_filters, callback):
    """the stages of ``overiva()`` (overiva.py:87-199) on a plan: ``overiva_batch()`` and ``overiva_batch_ragged()``"""
    global _info
    plan.set_x(X)
    plan.covariance()
    if W0 is None and init_eig:
        plan.set_w_eig()                      # overiva.py:106-109, the device eigensolver per bin
    else:
        plan.set_w(W0)
    epoch = 0
    while epoch < n_iter:
        if callback is not None and epoch % 10 == 0:      # overiva.py:142-148
            callback(plan.demix(proj_back, dtype))
        step = n_iter - epoch if callback is None else min(n_iter - epoch, 10 - epoch % 10)
        plan.iterate(step)
        epoch += step
    Y = plan.demix(proj_back, dtype)
    _info = plan.info()
    _overiva_module._last_info = dict(_info)        # (what last_solver_info() reports)
    W = plan.get_w(np.complex128)               # (raises LinAlgError naming the non-finite problems, overiva.py:182)
    if return_filters:
        return Y, W.astype(dtype, copy=False)
    return Y


def overiva_batch(X, n_src=None, n_iter=20, proj_back=True, W0=None, model="laplace", init_eig=False, return_filters=False,
                  callback=None, data="complex64"):
    """
    ``overiva()`` (reference overiva.py:28-204) on B problems of one shape at once.

    Parameters
    ----------
    X: ndarray (batch, nframes, nfrequencies, nchannels), complex
        STFT representations, 1..8 channels
    n_src, n_iter, proj_back, model, init_eig, return_filters:
        as ``overiva()``, the same for every problem
    W0: ndarray broadcastable to (nfrequencies, nchannels, nsrc) (one start for all), or (batch, nfrequencies, nchannels, nsrc)
    callback: func
        Called with the current (batch, nframes, nfrequencies, nsrc) estimate at epochs 0, 10, 20, ...
    data: "complex64" (default) or "complex128"
        "complex128": X must be complex128; it is held as it is and every stage runs in float64 (the module docstring); Y, W
        and the callback's estimates are complex128

    Returns
    -------
    Y (batch, nframes, nfrequencies, nsrc) in the dtype of X, or ``(Y, W)`` with W (batch, nfrequencies, nchannels, nsrc).
    A problem whose W ends non-finite raises ``numpy.linalg.LinAlgError`` naming every such problem.
    """
    _check_data(data, np.asarray(X).dtype)
    X, dtype, K = _check_args(X, n_src, model, W0, n_iter)
    B, T, F, M = X.shape
    with BatchPlan(B, T, F, M, K, model, data=data) as plan:
        return _run_overiva(plan, X, dtype, n_iter, proj_back, W0, init_eig, return_filters, callback)


def _run_ogive(plan, n_iter, W0, init_eig, model, step_size=0.1, tol=1e-3, update="demix", every_100=None):
    """the epochs of OGIVE on a batch plan whose X and covariance are set: the start, ``ogive_begin`` and chunks of epochs until every
    problem's stopping rule has fired or ``n_iter`` is reached, ``every_100()`` called at epochs 0, 100, 200, ... while any problem
    runs; returns the (B,) arrays of epochs run and of rules met"""
    B, F, M = plan.B, plan.F, plan.M
    if W0 is None and init_eig:                                         # ive.py:111-126 per problem (host LAPACK; not conjugated)
        cx = plan.get_cx(np.complex128)
        W0 = np.empty((B, F, M, 1), np.complex128)
        for b in range(B):
            vals, vecs = np.linalg.eig(cx[b])
            W0[b, :, :, 0] = np.stack([vecs[f][:, np.argmax(vals[f])] for f in range(F)])
    plan.set_w(None if W0 is None else np.asarray(W0))
    plan.ogive_begin(update, model)
    epochs = np.zeros(B, dtype=int)
    converged = np.zeros(B, dtype=bool)
    epoch = 0
    while epoch < n_iter and not converged.all():
        if every_100 is not None and epoch % 100 == 0:                  # ive.py:199-205
            every_100()
        step = min(n_iter - epoch, _ive.CHUNK)
        if every_100 is not None:
            step = min(step, 100 - epoch % 100)
        ran, converged, _ = plan.ogive_iterate(epoch, step, step_size, tol)
        epochs += ran
        epoch += step
    return epochs, converged


def ogive_batch(X, n_iter=4000, step_size=0.1, tol=1e-3, update="demix", proj_back=True, W0=None, model="laplace", init_eig=False,
                return_filters=False, callback=None):
    """
    ``ogive()`` (reference ive.py:33-256) on B problems of one shape at once, each with its own stopping rule.

    Parameters
    ----------
    X: ndarray (batch, nframes, nfrequencies, nchannels), complex
        STFT representations, 1..8 channels
    n_iter, step_size, tol, update, proj_back, model, init_eig, return_filters:
        as ``ogive()``, the same for every problem
    W0: ndarray broadcastable to (nfrequencies, nchannels, 1) (one start for all), or (batch, nfrequencies, nchannels, 1)
    callback: func
        Called with the current (batch, nframes, nfrequencies, 1) estimate every 100 epochs while any problem is running;
        problems that have stopped appear with their final state

    Returns
    -------
    Y (batch, nframes, nfrequencies, 1) in the dtype of X, or ``(Y, w)`` with w (batch, nfrequencies, nchannels, 1).
    Problem b gets what ``ogive(X[b], ...)`` gives in the ``precise`` arithmetic, including the epoch at which its stopping rule
    fires (``last_batch_info()["epochs"]``).  A problem whose w ends non-finite raises ``numpy.linalg.LinAlgError`` naming every
    such problem.
    """
    global _info
    X, dtype = _check_ogive_args(X, update, model, W0, n_iter)
    B, T, F, M = X.shape
    with BatchPlan(B, T, F, M, 1, model) as plan:
        plan.set_x(X)
        plan.covariance()                                                   # ive.py:100
        every_100 = None if callback is None else lambda: callback(plan.demix(proj_back, dtype))
        epochs, converged = _run_ogive(plan, n_iter, W0, init_eig, model, step_size, tol, update, every_100)
        Y = plan.demix(proj_back, dtype)                                    # ive.py:249-256
        _info = dict(plan.info(), algorithm="ogive", epochs=[int(e) for e in epochs], converged=[bool(c) for c in converged])
        w = plan.get_w(np.complex128)               # (raises LinAlgError naming the non-finite problems)
        if return_filters:
            return Y, w.astype(dtype, copy=False)
        return Y


class RaggedBatchPlan(BatchPlan):
    """Owns the device state of B problems of ``frames[b]`` x F x M with K sources (``oiva_batch_create_ragged``).

    The stages are ``BatchPlan``'s, and so is the device state: the two differ in what the caller hands over and gets back.
    ``set_x`` takes the list of B (T_b, F, M) arrays or the packed (sum T_b, F, M) array, ``set_x_device`` borrows a packed
    complex64 device array, and ``demix`` returns the list of B (T_b, F, K) arrays.  W, ``set_w``'s W0 and ``status`` are
    (B, ...).  Neither OGIVE nor ILRMA runs on a ragged batch: ``ogive_*`` and ``ilrma_*`` raise."""

    dense = False

    def __init__(self, frames, F, M, K, model="laplace", device=None, stream=None, data="complex64"):
        frames = [int(t) for t in frames]
        self._open(frames, max(frames) if frames else 0, F, M, K, model, device, stream, data)

    def _create(self, h, stream):
        return self.lib.oiva_batch_create_ragged(C.byref(h), self.device, self.B, (C.c_int * self.B)(*self.frames), self.F, self.M,
                                                 self.K, _lib.MODEL_IDS[self.model], stream)

    @property
    def shape(self):
        """shape of the packed X"""
        return (int(self.offsets[-1]), self.F, self.M)

    def info(self):
        return dict(BatchPlan.info(self), ragged=True, frames=list(self.frames))

    def set_x(self, X):
        """X: the list of B (T_b, F, M) arrays or the packed (sum T_b, F, M) array, complex64 or complex128 (complex128 is
        converted on the device)"""
        if isinstance(X, (list, tuple)):
            if len(X) != self.B or any(np.shape(x) != (t, self.F, self.M) for x, t in zip(X, self.frames)):
                raise ValueError(f"X must be {self.B} arrays of shapes (T_b, {self.F}, {self.M}), T_b = {self.frames}")
            for x in X:
                _check_data(self.data, np.asarray(x).dtype)
            dt = np.complex128 if any(np.asarray(x).dtype == np.complex128 for x in X) else np.complex64
            X = np.concatenate([np.asarray(x, dtype=dt) for x in X], axis=0)
        BatchPlan.set_x(self, X)

    def ogive_begin(self, *args, **kwargs):
        raise ValueError("OGIVE does not run on a ragged batch (use ogive_batch on same-length problems)")

    ogive_iterate = ogive_begin

    def ilrma_begin(self, *args, **kwargs):
        raise ValueError("ILRMA does not run on a ragged batch (use ilrma_batch on same-length rooms)")

    ilrma_iterate = ilrma_stage = get_nmf = get_pr = get_ilrma_cov = ilrma_time_stages = ilrma_begin

    def demix(self, proj_back=True, dtype=np.complex64):
        """the list of B arrays Y_b (T_b, F, K), complex64 or complex128"""
        out = self._demix_packed(proj_back, dtype)
        return [out[self.offsets[b]:self.offsets[b + 1]] for b in range(self.B)]


def overiva_batch_ragged(Xs, n_src=None, n_iter=20, proj_back=True, W0=None, model="laplace", init_eig=False, return_filters=False,
                         callback=None, data="complex64"):
    """
    ``overiva()`` (reference overiva.py:28-204) on B problems of different frame counts at once.

    Parameters
    ----------
    Xs: sequence of B ndarrays (nframes_b, nfrequencies, nchannels), complex
        STFT representations; nfrequencies, nchannels (1..8) and the dtype are the same for all, nframes_b >= 1 may differ
    n_src, n_iter, proj_back, model, init_eig, return_filters:
        as ``overiva()``, the same for every problem
    W0: ndarray broadcastable to (nfrequencies, nchannels, nsrc) (one start for all), or (batch, nfrequencies, nchannels, nsrc)
    callback: func
        Called with the list of current estimates Y_b (nframes_b, nfrequencies, nsrc) at epochs 0, 10, 20, ...
    data: "complex64" (default) or "complex128"
        as ``overiva_batch``: complex128 problems held as they are, every stage in float64

    Returns
    -------
    The list of B arrays Y_b (nframes_b, nfrequencies, nsrc) in the dtype of the inputs, or ``(Ys, W)`` with W (batch,
    nfrequencies, nchannels, nsrc).  Problem b gets exactly the bits of ``overiva_batch(Xs[b][None], ...)`` with the same
    arguments, whatever the other problems.  A problem whose W ends non-finite raises ``numpy.linalg.LinAlgError`` naming
    every such problem.
    """
    _check_data(data)
    for x in Xs if hasattr(Xs, "__len__") else ():
        _check_data(data, np.asarray(x).dtype)
    Xs, dtype, K = _check_ragged_args(Xs, n_src, model, W0, n_iter)
    F, M = Xs[0].shape[1:]
    with RaggedBatchPlan([x.shape[0] for x in Xs], F, M, K, model, data=data) as plan:
        return _run_overiva(plan, Xs, dtype, n_iter, proj_back, W0, init_eig, return_filters, callback)
