"""``ilrma_batch()`` and ``ilrma()``: independent low-rank matrix analysis on B rooms of one shape per set of launches
(``oiva_batch_ilrma_*``, csrc/kernels_ilrma_batch.hip).

ILRMA is the fifth algorithm of the reference's drivers (``-a ilrma`` of ``overiva_oneshot.py``, ``overiva_sim.py:295-315``),
which call it as ``pra.bss.ilrma``.  pyroomacoustics is a third-party package whose source is not part of the reference, so **the
contract is the algorithm as DESIGN.md 3.9 states it**, checked stage by stage against a NumPy restatement; parity with
``pra.bss.ilrma``'s bits is not pinned (as for ``projection_back``).

The model: determined (as many sources as channels), every source with an NMF variance ``r[s,f,t] = (Tn[s] @ Vn[s])[f,t]`` of
``n_components`` columns.  One epoch is the multiplicative updates of Tn and Vn, the covariances ``C_s = mean_t x x^H / r[s,f,t]``,
the IP1 step per bin with the sources in sequence, and the scale normalisation.  All state is float64 and W is carried in
complex128: the ``precise`` arithmetic of the other batched calls.  A room's bits do not depend on B or on its place in the batch.
"""
import numpy as np

from . import batch as _batch


def default_nmf_init(B, T, F, M, n_components, seed=None):
    """the start of the source model when ``T0`` / ``V0`` are not given: ``rng = np.random.RandomState(seed)``, then
    ``T0 = 0.1 + 0.9 rng.rand(B, M, F, L)`` and ``V0 = 0.1 + 0.9 rng.rand(B, M, L, T)``"""
    rng = np.random.RandomState(seed)
    T0 = 0.1 + 0.9 * rng.rand(B, M, F, n_components)
    V0 = 0.1 + 0.9 * rng.rand(B, M, n_components, T)
    return T0, V0


def _check_nmf(name, A, shape):
    A = np.asarray(A)
    if A.shape != shape:
        raise ValueError(f"{name} has shape {A.shape}: expected {shape}")
    if A.dtype.kind not in "fiu":
        raise ValueError(f"{name} must be real")
    if not (np.all(np.isfinite(A)) and np.all(A > 0)):
        raise ValueError(f"{name} must be finite and > 0 everywhere")
    return np.ascontiguousarray(A, dtype=np.float64)


def _check_args(X, n_src, n_iter, W0, n_components, T0, V0):
    X, dtype = _batch._check_dense_x(X)
    B, T, F, M = X.shape
    if n_src is not None and (isinstance(n_src, bool) or not isinstance(n_src, (int, np.integer)) or n_src != M):
        raise ValueError(f"ilrma_batch is determined: n_src must be None or the channel count {M}, got {n_src!r}")
    if isinstance(n_components, bool) or not isinstance(n_components, (int, np.integer)) or not 1 <= n_components <= 16:
        raise ValueError(f"n_components must be in 1..16, got {n_components!r}")
    _batch._check_common("ilrma_batch", "X has", B, F, M, None, "laplace", W0, n_iter, bool_counts=False)
    L = int(n_components)
    if T0 is not None:
        T0 = _check_nmf("T0", T0, (B, M, F, L))
    if V0 is not None:
        V0 = _check_nmf("V0", V0, (B, M, L, T))
    return X, dtype, L, T0, V0


def ilrma_batch(X, n_src=None, n_iter=20, proj_back=True, W0=None, n_components=2, return_filters=False, callback=None, T0=None,
                V0=None, seed=None, return_nmf=False):
    """
    ILRMA on B rooms of one shape at once.

    Parameters
    ----------
    X: ndarray (batch, nframes, nfrequencies, nchannels), complex
        STFT representations, 1..8 channels; complex128 is converted to complex64 on the device
    n_src: None or nchannels
        ILRMA here is determined
    n_iter: int
        epochs
    proj_back: bool
        scale the result onto channel 0 of the input, as ``overiva_batch`` does
    W0: ndarray broadcastable to (nfrequencies, nchannels, nchannels) (one start for all), or (batch, ...); default identity
    n_components: int, 1..16
        columns of the NMF source model
    T0, V0: ndarray (batch, nchannels, nfrequencies, n_components) and (batch, nchannels, n_components, nframes), > 0
        start of the source model; by default drawn as ``default_nmf_init(..., seed)`` (both, even when one is given)
    callback: func
        Called with the current (batch, nframes, nfrequencies, nchannels) estimate at epochs 0, 10, 20, ...

    Returns
    -------
    Y (batch, nframes, nfrequencies, nchannels) in the dtype of X; then W (batch, nfrequencies, nchannels, nchannels) when
    ``return_filters``; then ``(Tn, Vn)`` when ``return_nmf``.  A room whose W ends non-finite (a model that collapsed, an
    all-zero room) raises ``numpy.linalg.LinAlgError`` naming every such room.
    """
    X, dtype, L, T0, V0 = _check_args(X, n_src, n_iter, W0, n_components, T0, V0)
    B, T, F, M = X.shape
    if T0 is None or V0 is None:
        dT, dV = default_nmf_init(B, T, F, M, L, seed)
        T0 = dT if T0 is None else T0
        V0 = dV if V0 is None else V0
    with _batch.BatchPlan(B, T, F, M, M) as plan:
        plan.set_x(X)
        plan.covariance()
        plan.set_w(W0)
        plan.ilrma_begin(T0, V0)
        epoch = 0
        while epoch < n_iter:
            if callback is not None and epoch % 10 == 0:
                callback(plan.demix(proj_back, dtype))
            step = n_iter - epoch if callback is None else min(n_iter - epoch, 10 - epoch % 10)
            plan.ilrma_iterate(step)
            epoch += step
        Y = plan.demix(proj_back, dtype)
        _batch._info = dict(plan.info(), algorithm="ilrma", n_components=L)
        W = plan.get_w(np.complex128)               # (raises LinAlgError naming the non-finite rooms)
        out = (Y,)
        if return_filters:
            out += (W.astype(dtype, copy=False),)
        if return_nmf:
            out += (plan.get_nmf(),)
    return out[0] if len(out) == 1 else out


def ilrma(X, n_src=None, n_iter=20, proj_back=True, W0=None, n_components=2, return_filters=False, callback=None, T0=None, V0=None,
          seed=None, return_nmf=False):
    """ILRMA on one room: ``ilrma_batch(X[None], ...)`` with the batch axis removed from X, ``T0``, ``V0``, the callback's
    estimate and every result (W0 is one room's, (nfrequencies, nchannels, nchannels))."""
    X = np.asarray(X)
    if X.ndim != 3:
        raise ValueError("X must have shape (n_frames, n_freq, n_chan)")
    if W0 is not None and np.ndim(W0) > 3:
        raise ValueError(f"W0 has shape {np.shape(W0)}: expected one broadcastable to {(X.shape[1], X.shape[2], X.shape[2])}")
    cb = None if callback is None else (lambda Y: callback(Y[0]))
    out = ilrma_batch(X[None], n_src, n_iter, proj_back, W0, n_components, return_filters, cb,
                      None if T0 is None else np.asarray(T0)[None], None if V0 is None else np.asarray(V0)[None], seed, return_nmf)
    if not isinstance(out, tuple):
        return out[0]
    return tuple((o[0][0], o[1][0]) if isinstance(o, tuple) else o[0] for o in out)
