"""``five_batch()`` and ``five()``: single-source extraction by FIVE on B rooms per set of launches (``oiva_batch_five_*``,
csrc/kernels_five_batch.hip).

FIVE (Scheibler & Ono, "Fast independent vector extraction by iterative SINR maximization", ICASSP 2020) extracts one source
from M microphones with the source models and the cost of ``ogive()`` / ``overiva(n_src=1)``, but solves the surrogate of every
iteration exactly: per bin the eigenpair of ``V_f u = lambda Cx_f u`` with the smallest ``lambda``, ``V_f`` the covariance
weighted by the source's activation.  It settles in about ten iterations where OGIVE's gradient steps take thousands.  The
reference does not hold this algorithm, so **the contract is the algorithm as DESIGN.md 3.16 states it**, checked against a NumPy
restatement (tests/helpers/five_oracle.py).

1..8 channels, one source.  X lives on the device as complex64 (complex128 input is converted on the device) and ``five_begin``
widens it to a complex128 copy: the demix and power pass, the activation and the weighted covariance are the float64 stages of
the complex128 data path (``overiva_batch(..., data="complex128")``) with one source on that copy, the per-bin eigenproblem is
float64 and w is carried in complex128, so an iterate follows the float64 restatement to its own rounding.  A complex128 Y is
formed in float64 too; a complex64 Y leaves through the batch's complex64 output path.  A room's bits do not depend on B, on its
place in the batch or on the lengths of the other rooms.
"""
import numpy as np

from . import batch as _batch


def _check_args(X, n_src, n_iter, W0, model):
    """the arguments of ``five_batch``, before the library is touched: (X or the list of rooms, ragged, dtype, frames)"""
    ragged = isinstance(X, (list, tuple))
    if ragged:
        X, dtype = _batch._check_ragged_xs(X, "five_batch")
        B, (F, M), frames, found = len(X), X[0].shape[1:], [x.shape[0] for x in X], "the rooms have"
    else:
        X, dtype = _batch._check_dense_x(X)
        B, T, F, M = X.shape
        frames, found = [T] * B, "X has"
    if n_src is not None and (isinstance(n_src, bool) or not isinstance(n_src, (int, np.integer)) or n_src != 1):
        raise ValueError(f"five_batch: FIVE extracts one source, n_src must be None or 1, got {n_src!r}")
    if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)):
        raise ValueError(f"n_iter must be an integer, got {n_iter!r}")
    _batch._check_common("five_batch", found, B, F, M, 1, model, W0, n_iter, bool_counts=False)
    return X, ragged, dtype, frames


def run_five(plan, n_iter, W0, init_eig, every_10=None):
    """the iterations of FIVE on a batch plan (K = 1) whose X and covariance are set: the start, ``five_begin`` and ``n_iter``
    iterations, ``every_10()`` called at epochs 0, 10, 20, ..."""
    if W0 is None and init_eig:
        plan.set_w_eig()                      # the principal eigenvector of every bin's Cx, the device eigensolver
    else:
        plan.set_w(W0)
    plan.five_begin()
    epoch = 0
    while epoch < n_iter:
        if every_10 is not None and epoch % 10 == 0:
            every_10()
        step = n_iter - epoch if every_10 is None else min(n_iter - epoch, 10 - epoch % 10)
        plan.five_iterate(step)
        epoch += step


def five_batch(X, n_iter=10, proj_back=True, W0=None, model="laplace", init_eig=True, return_filters=False, callback=None,
               n_src=None):
    """
    FIVE on B rooms at once: one source out of each.

    Parameters
    ----------
    X: ndarray (batch, nframes, nfrequencies, nchannels), complex, or a sequence of B arrays (nframes_b, nfrequencies, nchannels)
        STFT representations, 1..8 channels; the rooms of a sequence share nfrequencies, nchannels and the dtype, their frame
        counts may differ
    n_iter, proj_back, model, return_filters:
        as ``overiva_batch()``, the same for every room
    W0: ndarray broadcastable to (nfrequencies, nchannels, 1) (one start for all), or (batch, nfrequencies, nchannels, 1)
    init_eig: bool
        without ``W0``: start from the principal eigenvector of every bin's input covariance (the default, FIVE's published
        start), else from the first column of the identity
    callback: func
        Called with the current estimate (as the result is shaped) at epochs 0, 10, 20, ...
    n_src: None or 1

    Returns
    -------
    Y (batch, nframes, nfrequencies, 1) in the dtype of X, or for a sequence the list of B arrays Y_b; with ``return_filters``
    ``(Y, W)``, W (batch, nfrequencies, nchannels, 1).  A room whose w ends non-finite (an input covariance that is not positive
    definite) raises ``numpy.linalg.LinAlgError`` naming every such room.
    """
    X, ragged, dtype, frames = _check_args(X, n_src, n_iter, W0, model)
    F, M = X[0].shape[-2:]
    plan = _batch.RaggedBatchPlan(frames, F, M, 1, model) if ragged else _batch.BatchPlan(len(frames), frames[0], F, M, 1, model)
    with plan:
        plan.set_x(X)
        plan.covariance()
        run_five(plan, n_iter, W0, init_eig, None if callback is None else lambda: callback(plan.demix(proj_back, dtype)))
        Y = plan.demix(proj_back, dtype)
        _batch._info = dict(plan.info(), algorithm="five")
        W = plan.get_w(np.complex128)               # (raises LinAlgError naming the non-finite rooms)
        if return_filters:
            return Y, W.astype(dtype, copy=False)
        return Y


def five(X, n_iter=10, proj_back=True, W0=None, model="laplace", init_eig=True, return_filters=False, callback=None, n_src=None):
    """FIVE on one room: ``five_batch(X[None], ...)`` with the batch axis removed from X, the callback's estimate and every result
    (W0 is one room's, (nfrequencies, nchannels, 1))."""
    X = np.asarray(X)
    if X.ndim != 3:
        raise ValueError("X must have shape (n_frames, n_freq, n_chan)")
    if W0 is not None and np.ndim(W0) > 3:
        raise ValueError(f"W0 has shape {np.shape(W0)}: expected one broadcastable to {(X.shape[1], X.shape[2], 1)}")
    cb = None if callback is None else (lambda Y: callback(Y[0]))
    out = five_batch(X[None], n_iter, proj_back, W0, model, init_eig, return_filters, cb, n_src)
    if return_filters:
        return out[0][0], out[1][0]
    return out[0]
