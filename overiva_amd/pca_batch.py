"""``auxiva_pca_batch()``: PCA to ``n_src`` channels followed by determined AuxIVA (reference ``auxiva_pca.py:63-92``) on B rooms
per call, of one length or of different lengths.

The stages of ``auxiva_pca()`` on two batch plans, with nothing crossing the host in between: the outer plan (M channels) forms
every bin's input covariance and its principal subspace (``set_w_pca``, the Jacobi eigensolver of csrc/kernels_evd.hip on B * F
bins) and projects all rooms onto it in one launch (``project_device``, csrc/kernels_pca_batch.hip); a determined inner plan of K
channels borrows the projected X and runs the iterations -- on K channels, where the batched path is fastest; the outer plan
composes P W_red on the device (``compose_w``) and demixes the ORIGINAL input with it, projecting back onto its channel 0.  X is
read three times in all: the covariance, the projection and the final demix.
"""
import numpy as np

from . import batch as _batch


def reduce_and_solve(outer, n_iter=20, W0=None, init_eig=False, model="laplace"):
    """the PCA front end and the determined solve on ``outer``, a batch plan with K < M whose X is set and whose covariance is
    computed: leaves the composed filters P W_red in ``outer`` (``demix(proj_back=True)`` / ``get_w`` read the result)"""
    outer.set_w_pca()                                                         # auxiva_pca.py:75: eigh, w[:, :, -n_src:]
    new_X = outer.project_device()                                            # x -> P^H x, auxiva_pca.py:79-81
    K = outer.K
    inner = (_batch.BatchPlan(outer.B, outer.T, outer.F, K, K, model, device=outer.device) if outer.dense else
             _batch.RaggedBatchPlan(outer.frames, outer.F, K, K, model, device=outer.device))
    with inner:
        inner.set_x_device(new_X.ptr, keepalive=new_X)
        inner.covariance()
        if W0 is None and init_eig:                                           # auxiva_pca.py:87: overiva() on the reduced channels
            inner.set_w_eig()
        else:
            inner.set_w(W0)
        inner.iterate(n_iter)
        outer.compose_w(inner)                                                # y = W_red^H (P^H x) = (P W_red)^H x


def auxiva_pca_batch(X, n_src=None, n_iter=20, proj_back=True, W0=None, model="laplace", init_eig=False, return_filters=False):
    """
    ``auxiva_pca()`` (reference auxiva_pca.py:30-92) on B problems at once.

    Parameters
    ----------
    X: ndarray (batch, nframes, nfrequencies, nchannels), or a sequence of B ndarrays (nframes_b, nfrequencies, nchannels), complex
        STFT representations, 1..8 channels; a sequence may hold problems of different frame counts (one nfrequencies,
        nchannels and dtype)
    n_src: int
        channels kept by the PCA = sources of the determined solve (default: nchannels, no PCA)
    n_iter, model, init_eig:
        as ``overiva()`` for the inner determined solve, the same for every problem
    proj_back:
        accepted and ignored: the result is always projected back onto channel 0 of the ORIGINAL input (auxiva_pca.py:89-90).
        (The single call's ``KeyError`` when it is missing is not reproduced.)
    W0: ndarray broadcastable to (nfrequencies, nsrc, nsrc) (one start for all), or (batch, nfrequencies, nsrc, nsrc)
        start of the inner solve, on the reduced channels
    return_filters: bool
        an extension (the reference returns Y only): also return the composed filters W_tot = P W_red

    Returns
    -------
    Y (batch, nframes, nfrequencies, nsrc), or the list of B arrays (nframes_b, nfrequencies, nsrc) for a sequence, in the dtype
    of X; with ``return_filters`` ``(Y, W_tot)``, W_tot (batch, nfrequencies, nchannels, nsrc).  Problem b's bits do not depend
    on the other problems.  With nsrc == nchannels the call is ``overiva_batch`` / ``overiva_batch_ragged`` with
    ``proj_back=True``.  There is no ``callback`` (the reference would hand it estimates in the reduced space).  A problem whose
    filters end non-finite raises ``numpy.linalg.LinAlgError`` naming every such problem.
    """
    ragged = isinstance(X, (list, tuple))
    if ragged:
        X, dtype = _batch._check_ragged_xs(X, "auxiva_pca_batch")
        B, (F, M) = len(X), X[0].shape[1:]
        found = "the problems have"
    else:
        X, dtype = _batch._check_dense_x(X)
        B, _, F, M = X.shape
        found = "X has"
    K = _batch._check_common("auxiva_pca_batch", found, B, F, M, n_src, model, W0, n_iter, bool_counts=False, w0_reduced=True)
    if K == M:                                                                # no PCA: determined AuxIVA on the input itself
        run = _batch.overiva_batch_ragged if ragged else _batch.overiva_batch
        out = run(X, n_src=None, n_iter=n_iter, proj_back=True, W0=W0, model=model, init_eig=init_eig, return_filters=return_filters)
        _batch._info = dict(_batch._info, algorithm="auxiva_pca", reduced=K)
        return out
    plan = _batch.RaggedBatchPlan([x.shape[0] for x in X], F, M, K, model) if ragged else _batch.BatchPlan(B, X.shape[1], F, M, K, model)
    with plan:
        plan.set_x(X)
        plan.covariance()                                                     # auxiva_pca.py:71
        reduce_and_solve(plan, n_iter, W0, init_eig, model)
        Y = plan.demix(True, dtype)                                           # auxiva_pca.py:89-90
        _batch._info = dict(plan.info(), algorithm="auxiva_pca", reduced=K)
        W = plan.get_w(np.complex128)               # (raises LinAlgError naming the non-finite problems)
    if return_filters:
        return Y, W.astype(dtype, copy=False)
    return Y
