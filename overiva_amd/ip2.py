"""``overiva_ip2_batch()`` and ``overiva_ip2()``: OverIVA / AuxIVA with pairwise IP2 updates on B rooms per set of launches
(``oiva_batch_ip2_*``, csrc/kernels_ip2_batch.hip).

IP2 (Ono, IWAENC 2012; Scheibler & Ono's OverIVA-IP2) updates two demixing vectors jointly, by the exact minimiser of the
surrogate over the pair, where IP1 updates one at a time.  The source models, the auxiliary weights and the weighted covariances
are ``overiva()``'s; only the per-bin algebra changes, and with it the number of iterations a separation needs.  The reference
does not hold this algorithm, so **the contract is the algorithm as DESIGN.md 3.17 states it**, checked against a NumPy
restatement.

1..8 channels, 1 <= n_src <= n_chan (``n_src=None``: determined AuxIVA).  X lives on the device as complex64 (complex128 input
is converted on the device); every stage is float64 on a complex128 copy of X and W is carried in complex128.  A room's bits do
not depend on B, on its place in the batch or on the lengths of the other rooms.
"""
import numpy as np

from . import batch as _batch


def schedule(K, iteration):
    """the steps of iteration ``iteration`` (0-based, counted from the start of the separation) for K sources: a list of
    ``(a, b)`` pair steps and ``(s,)`` single IP1 steps in which every source appears once

    even: (0,1), (2,3), ..., then (K-1) alone if K is odd; odd and K > 2: (0) alone, (1,2), (3,4), ..., then (K-1) alone if K is
    even; K = 2: (0,1) in every iteration; K = 1: (0) alone"""
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K < 1:
        raise ValueError(f"K must be an integer >= 1, got {K!r}")
    if isinstance(iteration, bool) or not isinstance(iteration, (int, np.integer)) or iteration < 0:
        raise ValueError(f"iteration must be an integer >= 0, got {iteration!r}")
    steps, s = [], 0
    if K == 1 or (K > 2 and iteration % 2 == 1):
        steps.append((0,))
        s = 1
    while s + 1 < K:
        steps.append((s, s + 1))
        s += 2
    if s < K:
        steps.append((s,))
    return steps


def _check_args(X, n_src, n_iter, W0, model):
    """the arguments of ``overiva_ip2_batch``, before the library is touched: (X or the list of rooms, ragged, dtype, frames, K)"""
    ragged = isinstance(X, (list, tuple))
    if ragged:
        X, dtype = _batch._check_ragged_xs(X, "overiva_ip2_batch")
        B, (F, M), frames, found = len(X), X[0].shape[1:], [x.shape[0] for x in X], "the rooms have"
    else:
        X, dtype = _batch._check_dense_x(X)
        B, T, F, M = X.shape
        frames, found = [T] * B, "X has"
    if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)):
        raise ValueError(f"n_iter must be an integer, got {n_iter!r}")
    K = _batch._check_common("overiva_ip2_batch", found, B, F, M, n_src, model, W0, n_iter, bool_counts=False)
    return X, ragged, dtype, frames, K


def run_ip2(plan, n_iter, W0, init_eig, every_10=None):
    """the iterations of IP2 on a batch plan whose X and covariance are set: the start and ``n_iter`` iterations, ``every_10()``
    called at iterations 0, 10, 20, ..."""
    if W0 is None and init_eig:
        plan.set_w_eig()                      # overiva.py:106-109, the device eigensolver per bin
    else:
        plan.set_w(W0)
    epoch = 0
    while epoch < n_iter:
        if every_10 is not None and epoch % 10 == 0:
            every_10()
        step = n_iter - epoch if every_10 is None else min(n_iter - epoch, 10 - epoch % 10)
        plan.ip2_iterate(epoch, step)
        epoch += step


def overiva_ip2_batch(X, n_src=None, n_iter=20, proj_back=True, W0=None, model="laplace", init_eig=False, return_filters=False,
                      callback=None):
    """
    OverIVA (``n_src`` < nchannels) or determined AuxIVA with pairwise IP2 updates on B rooms at once.

    Parameters
    ----------
    X: ndarray (batch, nframes, nfrequencies, nchannels), complex, or a sequence of B arrays (nframes_b, nfrequencies, nchannels)
        STFT representations, 1..8 channels; the rooms of a sequence share nfrequencies, nchannels and the dtype, their frame
        counts may differ
    n_src, n_iter, proj_back, model, init_eig, return_filters:
        as ``overiva_batch()``, the same for every room
    W0: ndarray broadcastable to (nfrequencies, nchannels, nsrc) (one start for all), or (batch, ...); default identity
    callback: func
        Called with the current estimate (as the result is shaped) at iterations 0, 10, 20, ...

    Returns
    -------
    Y (batch, nframes, nfrequencies, nsrc) in the dtype of X, or for a sequence the list of B arrays Y_b; with
    ``return_filters`` ``(Y, W)``, W (batch, nfrequencies, nchannels, nsrc).  A room whose W ends non-finite raises
    ``numpy.linalg.LinAlgError`` naming every such room.
    """
    X, ragged, dtype, frames, K = _check_args(X, n_src, n_iter, W0, model)
    F, M = X[0].shape[-2:]
    plan = _batch.RaggedBatchPlan(frames, F, M, K, model) if ragged else _batch.BatchPlan(len(frames), frames[0], F, M, K, model)
    with plan:
        plan.set_x(X)
        plan.covariance()
        run_ip2(plan, n_iter, W0, init_eig, None if callback is None else lambda: callback(plan.demix(proj_back, dtype)))
        Y = plan.demix(proj_back, dtype)
        _batch._info = dict(plan.info(), algorithm="overiva_ip2")
        W = plan.get_w(np.complex128)               # (raises LinAlgError naming the non-finite rooms)
        if return_filters:
            return Y, W.astype(dtype, copy=False)
        return Y


def overiva_ip2(X, n_src=None, n_iter=20, proj_back=True, W0=None, model="laplace", init_eig=False, return_filters=False,
                callback=None):
    """IP2 on one room: ``overiva_ip2_batch(X[None], ...)`` with the batch axis removed from X, the callback's estimate and every
    result (W0 is one room's, (nfrequencies, nchannels, nsrc))."""
    X = np.asarray(X)
    if X.ndim != 3:
        raise ValueError("X must have shape (n_frames, n_freq, n_chan)")
    if W0 is not None and np.ndim(W0) > 3:
        raise ValueError(f"W0 has shape {np.shape(W0)}: expected one broadcastable to (n_freq, n_chan, n_src)")
    cb = None if callback is None else (lambda Y: callback(Y[0]))
    out = overiva_ip2_batch(X[None], n_src, n_iter, proj_back, W0, model, init_eig, return_filters, cb)
    if return_filters:
        return out[0][0], out[1][0]
    return out[0]
