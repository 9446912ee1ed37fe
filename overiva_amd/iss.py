"""``auxiva_iss_batch()`` and ``auxiva_iss()``: determined AuxIVA by iterative source steering (ISS) on B rooms per set of launches
(``oiva_batch_iss_*``, csrc/kernels_iss_batch.hip).

ISS (Scheibler & Ono, "Fast and stable blind source separation with rank-1 updates", ICASSP 2020) minimises the cost of
determined AuxIVA with the source models and the auxiliary weights of ``overiva()``, but replaces every IP1 row update by a
rank-1 update of the demixed signals: no covariance matrix is formed and no linear system solved, O(M^2) per (bin, frame) and
iteration instead of O(M^3).  A fixed point of IP1 is a fixed point of ISS.  The reference does not hold this algorithm, so **the
contract is the algorithm as DESIGN.md 3.15 states it**, checked stage by stage against a NumPy restatement.

Determined only: as many sources as channels, 1..8 channels, and ``n_frames * n_chan <= 8192`` in every room (a bin's demixed
signals stay in the LDS as complex128 through the M steps of an iteration).  X lives on the device as complex64 (complex128 input
is converted on the device); every stage is float64 and W is carried in complex128: the ``precise`` arithmetic of the other
batched calls.  A room's bits do not depend on B, on its place in the batch or on the lengths of the other rooms.
"""
import numpy as np

from . import batch as _batch

MAX_SLAB = _batch.ISS_MAX_SLAB


def _check_args(X, n_src, n_iter, W0, model):
    """the arguments of ``auxiva_iss_batch``, before the library is touched: (X or the list of rooms, ragged, dtype, frames)"""
    ragged = isinstance(X, (list, tuple))
    if ragged:
        X, dtype = _batch._check_ragged_xs(X, "auxiva_iss_batch")
        B, (F, M), frames, found = len(X), X[0].shape[1:], [x.shape[0] for x in X], "the rooms have"
    else:
        X, dtype = _batch._check_dense_x(X)
        B, T, F, M = X.shape
        frames, found = [T] * B, "X has"
    if n_src is not None and (isinstance(n_src, bool) or not isinstance(n_src, (int, np.integer)) or n_src != M):
        raise ValueError(f"auxiva_iss_batch: ISS is determined, n_src must be None or the channel count {M}, got {n_src!r}")
    if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)):
        raise ValueError(f"n_iter must be an integer, got {n_iter!r}")
    _batch._check_common("auxiva_iss_batch", found, B, F, M, None, model, W0, n_iter, bool_counts=False)
    for b, t in enumerate(frames):
        if t * M > MAX_SLAB:
            raise ValueError(f"auxiva_iss_batch needs n_frames * n_chan <= {MAX_SLAB} in every room: room {b} has {t} x {M} = {t * M}")
    return X, ragged, dtype, frames


def run_iss(plan, n_iter, W0, init_eig, every_10=None):
    """the iterations of ISS on a batch plan whose X and covariance are set: the start, ``iss_begin`` and ``n_iter`` iterations,
    ``every_10()`` called at epochs 0, 10, 20, ..."""
    if W0 is None and init_eig:
        plan.set_w_eig()                      # overiva.py:106-109, the device eigensolver per bin
    else:
        plan.set_w(W0)
    plan.iss_begin()
    epoch = 0
    while epoch < n_iter:
        if every_10 is not None and epoch % 10 == 0:
            every_10()
        step = n_iter - epoch if every_10 is None else min(n_iter - epoch, 10 - epoch % 10)
        plan.iss_iterate(step)
        epoch += step


def auxiva_iss_batch(X, n_src=None, n_iter=20, proj_back=True, W0=None, model="laplace", init_eig=False, return_filters=False,
                     callback=None):
    """
    Determined AuxIVA by rank-1 ISS updates on B rooms at once.

    Parameters
    ----------
    X: ndarray (batch, nframes, nfrequencies, nchannels), complex, or a sequence of B arrays (nframes_b, nfrequencies, nchannels)
        STFT representations, 1..8 channels, ``nframes * nchannels <= 8192``; the rooms of a sequence share nfrequencies,
        nchannels and the dtype, their frame counts may differ
    n_src: None or nchannels
        ISS is determined
    n_iter, proj_back, model, init_eig, return_filters:
        as ``overiva_batch()``, the same for every room
    W0: ndarray broadcastable to (nfrequencies, nchannels, nchannels) (one start for all), or (batch, ...); default identity
    callback: func
        Called with the current estimate (as the result is shaped) at epochs 0, 10, 20, ...

    Returns
    -------
    Y (batch, nframes, nfrequencies, nchannels) in the dtype of X, or for a sequence the list of B arrays Y_b; with
    ``return_filters`` ``(Y, W)``, W (batch, nfrequencies, nchannels, nchannels).  A room whose W ends non-finite raises
    ``numpy.linalg.LinAlgError`` naming every such room.
    """
    X, ragged, dtype, frames = _check_args(X, n_src, n_iter, W0, model)
    F, M = X[0].shape[-2:]
    plan = _batch.RaggedBatchPlan(frames, F, M, M, model) if ragged else _batch.BatchPlan(len(frames), frames[0], F, M, M, model)
    with plan:
        plan.set_x(X)
        plan.covariance()                     # (what set_w and the eigenvector start need)
        run_iss(plan, n_iter, W0, init_eig, None if callback is None else lambda: callback(plan.demix(proj_back, dtype)))
        Y = plan.demix(proj_back, dtype)
        _batch._info = dict(plan.info(), algorithm="auxiva_iss")
        W = plan.get_w(np.complex128)               # (raises LinAlgError naming the non-finite rooms)
        if return_filters:
            return Y, W.astype(dtype, copy=False)
        return Y


def auxiva_iss(X, n_src=None, n_iter=20, proj_back=True, W0=None, model="laplace", init_eig=False, return_filters=False,
               callback=None):
    """ISS on one room: ``auxiva_iss_batch(X[None], ...)`` with the batch axis removed from X, the callback's estimate and every
    result (W0 is one room's, (nfrequencies, nchannels, nchannels))."""
    X = np.asarray(X)
    if X.ndim != 3:
        raise ValueError("X must have shape (n_frames, n_freq, n_chan)")
    if W0 is not None and np.ndim(W0) > 3:
        raise ValueError(f"W0 has shape {np.shape(W0)}: expected one broadcastable to {(X.shape[1], X.shape[2], X.shape[2])}")
    cb = None if callback is None else (lambda Y: callback(Y[0]))
    out = auxiva_iss_batch(X[None], n_src, n_iter, proj_back, W0, model, init_eig, return_filters, cb)
    if return_filters:
        return out[0][0], out[1][0]
    return out[0]
