"""The batched PCA front end with as many sources as channels, through the staged plan methods (``set_w_pca``, ``project_device``,
``compose_w``): ``auxiva_pca_batch`` hands a determined problem to ``overiva_batch``, so pca_project_kernel<1, 1>, <2, 2>, <3, 4> and
pca_compose_kernel<8> ran in no test (tools/kernel_census.py), while a caller of the plan methods reaches them.

The projection against X conj(P) formed in float64 from the float32 P the device holds: TOL_KERNEL, the bound of the float32
stages (tests/test_gpu_parity.py).  The composed filters against np.matmul: the 1e-13 of tests/test_pca_batch_gpu.py::test_compose
(at most 8 terms of float64 products per element)."""
import numpy as np
import pytest

from oracle import overiva_oracle as orc

pytestmark = pytest.mark.gpu

TOL_KERNEL = 3e-6
# 67 bins leave a last bin batch of 3; frame counts on both sides of the 64-frame power split
CASES = [(1, 1), (2, 2), (3, 3), (8, 8)]
FRAMES, F = (16, 63, 65), 67


@pytest.fixture(scope="module")
def oa():
    import overiva_amd

    overiva_amd._lib.load()
    return overiva_amd


@pytest.mark.parametrize("dense", [False, True], ids=["ragged", "dense"])
@pytest.mark.parametrize("M, K", CASES)
def test_determined_projection_and_compose(oa, M, K, dense):
    frames = (65, 65, 65) if dense else FRAMES
    Xs = [orc.synth_iid(T, F, M, seed=500 + 10 * M + b) for b, T in enumerate(frames)]
    if dense:
        X = np.stack(Xs)
        plan = oa.BatchPlan(X.shape[0], X.shape[1], X.shape[2], M, K)
        plan.set_x(X)
    else:
        plan = oa.RaggedBatchPlan(list(frames), F, M, K)
        plan.set_x(Xs)
    with plan:
        plan.covariance()
        plan.set_w_pca()
        P32 = plan.get_w(np.complex64)
        P = plan.get_w(np.complex128)
        new_X = plan.project_device()
        got = new_X.get_x()
        inner = oa.BatchPlan(plan.B, plan.T, plan.F, K, K) if dense else oa.RaggedBatchPlan(plan.frames, plan.F, K, K)
        with inner:
            inner.set_x_device(new_X.ptr, keepalive=new_X)
            inner.covariance()
            inner.set_w(None)
            inner.iterate(2)
            W_red = inner.get_w(np.complex128)
            plan.compose_w(inner)
        W = plan.get_w(np.complex128)
    want_W = np.matmul(P, W_red)
    for b, T in enumerate(frames):
        want = np.einsum("tfm,fmk->tfk", Xs[b].astype(np.complex128), np.conj(P32[b].astype(np.complex128)))
        e, ew = orc.rel_err(got[b], want), orc.rel_err(W[b], want_W[b])
        print(f"\n[census] PCA {M} / {K}, room {b} ({T} frames): projection {e:.2e}, composed filters {ew:.2e}")
        assert got[b].shape == (T, F, K) and e < TOL_KERNEL, (b, e)
        assert ew < 1e-13, (b, ew)
