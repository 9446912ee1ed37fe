"""Kernels of the epilogue, the exchanges and the 9..16-channel covariance pass that a public call reaches and no test launched
(tools/kernel_census.py), each at a small shape against the float64 reference of the same operation.  Every bound is the one of
the test of the kernel's siblings, named at the case.

* the batched STFT with 5..8 sources (bstft_from_tfc_kernel<5..8>, bstft_overlap_add_kernel<5..8>) and 8 channels on a frame
  length that is no multiple of 4 (bstft_frame_kernel<8, false>): TOL of tests/test_separate_gpu.py;
* the X-resident kernel at 6 channels, one source, 8 frames per lane in registers (resident_kernel<6, 1, 8, float|double, false>):
  TOL of tests/test_resident_gpu.py::test_resident_shard_against_oracle;
* the in-activation exchange with 3 and with 8 parts per block (activation_xchg_kernel<0>, <8>): TOL_KERNEL of
  tests/test_gpu_parity.py::test_activation;
* the push exchange on a part that is no multiple of 16 bytes (push_kernel<float>): a copy, compared exactly;
* the float64 matrix-core covariance pass with flat loads (cov_hmfma64_kernel<false>, $OIVA_HMFMA_FLAT=1, read at every launch):
  the 1e-12 of tests/test_cov_quad_gpu.py::test_sources_on_the_fp64_matrix_cores_against_the_vector_alu_kernel."""
import numpy as np
import pytest

from oracle import overiva_oracle as orc
from oracle import stft_oracle as so

pytestmark = pytest.mark.gpu

TOL = 1e-5
TOL_KERNEL = 3e-6
TOL_KERNEL_F64 = 1e-12


@pytest.fixture(scope="module")
def oa():
    import overiva_amd

    overiva_amd._lib.load()
    return overiva_amd


def _windows(frame, hop):
    wa = so.hann(frame)
    return wa, so.compute_synthesis_window(wa, hop)


@pytest.mark.parametrize("k", [5, 6, 7, 8])
def test_synthesis_of_5_to_8_sources(oa, k):
    """rooms of different lengths, one of a single frame, one that ends inside a hop"""
    frame, hop, C = 64, 32, 8
    rng = np.random.default_rng(frame + k)
    lens = [hop * 7, hop * 5 + 1, hop, hop * 6 + hop - 1]
    xs = [rng.standard_normal((n, C)).astype(np.float32) for n in lens]
    wa, ws = _windows(frame, hop)
    with oa.BatchSTFT(lens, C, frame, hop, win_a=wa, win_s=ws) as st:
        Xd = st.analysis_device(xs)
        with oa.RaggedBatchPlan(st.frames, st.n_freq, C, k) as plan:
            plan.set_x_device(Xd.ptr, keepalive=Xd)
            plan.covariance()
            plan.set_w(None)
            Yd = plan.demix_device(True)
            Ys = Yd.get_x()
            ys = st.synthesis_device(Yd)
        for b, (Y, y) in enumerate(zip(Ys, ys)):
            yr = so.synthesis(Y, frame, hop, ws)
            assert y.shape == yr.shape == (st.frames[b] * hop, k) and y.dtype == np.float32
            err = orc.rel_err(y, yr)
            print(f"\n[census] synthesis K={k} room {b}: {err:.2e}")
            assert err < TOL


@pytest.mark.parametrize("B", [1, 3])
def test_analysis_of_8_channels_on_a_frame_length_that_is_no_multiple_of_4(oa, B):
    frame, hop, C = 30, 10, 8
    rng = np.random.default_rng(frame + C + B)
    n = hop * 9 + hop // 3
    x = rng.standard_normal((B, n, C))
    wa, ws = _windows(frame, hop)
    with oa.BatchSTFT(n, C, frame, hop, win_a=wa, win_s=ws, B=B) as st:
        X = st.analysis_device(x).get_x()
    for b in range(B):
        err = orc.rel_err(X[b], so.analysis(x[b], frame, hop, wa))
        print(f"\n[census] analysis L={frame} C={C} room {b}: {err:.2e}")
        assert err < TOL


@pytest.mark.parametrize("mode", ["fast", "mixed"])
def test_resident_6_channels_one_source_with_register_frames(oa, mode):
    """4000 frames x 200 bins: 13 bin groups, 14 frames per lane of which 8 in registers; 3 iterations against the oracle"""
    T, F, M, K = 4000, 200, 6, 1
    X = orc.synth_iid(T, F, M, seed=1)
    Yr, Wr = orc.overiva_staged(X.astype(np.complex128), n_src=K, n_iter=3, proj_back=False, return_filters=True)
    with oa.Plan(T, F, M, K, "laplace") as p:
        p.set_precision(mode)
        p.set_x(X)
        p.covariance()
        p.set_w(None)
        p.set_resident(True)
        p.iterate(3)
        W = p.get_w(np.complex128)
        Y = p.demix(False)
        info = p.resident_info()
    eW, eY = orc.rel_err(W, Wr), orc.rel_err(Y, Yr)
    print(f"\n[census] resident {M} / {K} {mode}: W {eW:.1e} Y {eY:.1e}, {info['frames_per_lane']} frames per lane, {info['frames_in_registers']} in registers")
    assert info["fallbacks"] == 0 and info["launches"] == 1 and info["frames_in_registers"] == 8
    assert eW < TOL and eY < TOL


@pytest.mark.parametrize("F", [1100, 3700], ids=["3-parts-per-block", "8-parts-per-block"])
@pytest.mark.parametrize("world", [2, 8])
def test_activation_with_the_exchange_at_many_bins(oa, F, world):
    """18 and 58 parts of 64 bins in 6 and 8 blocks; this GPU plays every rank (the others send zeros): r_inv and the scale of W
    after one iteration against the oracle from the same start"""
    T, M, K = 40, 4, 3
    X = orc.synth_iid(T, F, M, seed=F)
    for model in ("laplace", "gauss"):
        with oa.Plan(T, F, M, K, model) as p:
            p.set_x(X)
            p.covariance()
            p.set_w(None)
            W0 = p.t_get_what()
            p.fused_loopback(world)
            p.iterate(1)
            p.sync()
            rinv, wscale = p.t_get_rinv()
        ref_rinv, ref_ws = orc.finalize_activation(orc.demix_power(X, W0[:, :, :K]), F, model)
        e, ew = orc.rel_err(rinv, ref_rinv), orc.rel_err(wscale, ref_ws)
        print(f"\n[census] activation with exchange F={F} world {world} {model}: r_inv {e:.2e}, scale {ew:.2e}")
        assert e < TOL_KERNEL and ew < TOL_KERNEL


@pytest.mark.parametrize("nfloats", [67, 1, 1027, 64], ids=lambda n: f"{4 * n}-bytes")
def test_push_exchange_of_a_part_that_is_no_multiple_of_16_bytes(oa, nfloats):
    """a world of one: what is gathered is the part (64 floats: the 16-byte form, for comparison)"""
    import torch

    from overiva_amd import exchange

    part = torch.arange(1, nfloats + 1, dtype=torch.float32, device="cuda:0") * 0.37
    stream = torch.cuda.Stream(device=0)
    with exchange.PushExchange(0, 0, 1, part.data_ptr(), nfloats * 4, stream.cuda_stream) as ex:
        for epoch in range(2):
            part += 1.0
            stream.wait_stream(torch.cuda.current_stream())
            got = exchange._device_view(torch, ex.gather(), nfloats, "cuda:0")
            stream.synchronize()
            assert ex.poll(1000)
            assert torch.equal(got.cpu(), part.cpu()), epoch


@pytest.mark.parametrize("shape", [(70, 2, 16, 12), (97, 3, 15, 15), (33, 1, 16, 9)])
def test_fp64_matrix_core_covariance_with_flat_loads(oa, shape, monkeypatch):
    """`precise`, 9..16 sources, the flat form of the loads (it clamps the addresses of the frames past T where the buffer form's
    range check zeroes them): the same bits as the buffer form, and the oracle's float64 sums"""
    T, F, M, K = shape
    X = orc.synth_iid(T, F, M, seed=33)
    rinv = np.random.default_rng(6).gamma(2.0, 1.0, (T, K)).astype(np.float32)
    V = {}
    for flat in ("0", "1"):
        monkeypatch.setenv("OIVA_HMFMA_FLAT", flat)
        with oa.Plan(T, F, M, K, "laplace") as p:
            p.set_precision("precise")
            p.set_x(X)
            p.covariance()
            p.t_set_rinv(rinv)
            p.t_run_weighted_cov()
            V[flat] = p.t_get_v(np.complex128)
    w = 1.0 / (np.float32(1) / rinv).astype(np.float64)
    e = orc.rel_err(V["1"], orc.weighted_cov_all(X, w))
    print(f"\n[census] cov_hmfma64 flat loads {shape}: {e:.2e}")
    assert e < TOL_KERNEL_F64
    assert np.array_equal(V["1"], V["0"])
