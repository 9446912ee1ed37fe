"""separate_batch(): audio in, audio out for B rooms with X and Y staying on the device (overiva_amd/separate.py -> oiva_bstft_*,
csrc/kernels_bstft.hip), checked stage by stage so that no tolerance has to absorb the solver's amplification of rounding
differences in X: the analysis against the NumPy oracle, the solver on the device array against the solver on the same bits from
the host (bit-identical), the synthesis against the oracle, the whole chain by its time-domain SIR, and the composed path a user
ran before (one stft.analysis / stft.synthesis per room around overiva_batch_ragged).  Needs an MI355X: run with ``-m gpu``."""
import numpy as np
import pytest

from oracle import overiva_oracle as orc
from oracle import stft_oracle as so

pytestmark = pytest.mark.gpu
TOL = 1e-5      # float32 FFT of length <= 4096 against float64 (tests/test_stft_gpu.py)
ROOMS = [(11, 102400), (12, 85348), (13, 70407), (14, 102400), (15, 77056), (16, 100095), (17, 89600)]
L, HOP, M, K, N_ITER = 512, 256, 4, 2, 30


def _windows(frame, hop):
    wa = so.hann(frame) if hop < frame else None
    ws = so.compute_synthesis_window(wa, hop) if hop < frame else None
    return wa, ws


def _room(seed, n, M=M, K=K):
    """the generator of test_stft_gpu.test_audio_in_audio_out_separation, safe for any n"""
    rng = np.random.default_rng(seed)
    env = np.repeat(rng.gamma(0.3, 1.0, (n // 512 + 1, K)), 512, axis=0)[:n]
    src = env * rng.standard_normal((n, K))
    A = rng.standard_normal((M, K))
    A[:K] += 2 * np.eye(K)
    x = src @ A.T + 0.01 * rng.standard_normal((n, M))
    return x, src


def _sir(sig, src):
    """best-permutation SIR via projections on the sources (the sir() of test_audio_in_audio_out_separation)"""
    k = sig.shape[1]
    G = np.linalg.lstsq(src[: len(sig)], sig, rcond=None)[0]
    P = (G ** 2) * np.sum(src[: len(sig)] ** 2, axis=0)[:, None]
    return max(np.mean([10 * np.log10(P[perm[j], j] / (P[:, j].sum() - P[perm[j], j])) for j in range(k)])
               for perm in ((0, 1), (1, 0)))


# ---- 1. analysis -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame,hop,C", [(64, 32, 3), (512, 256, 8), (4096, 2048, 4), (128, 128, 1), (256, 64, 2), (96, 32, 5), (30, 10, 4),
                                         (96, 32, 6), (64, 32, 7)])
@pytest.mark.parametrize("B", [1, 5])
def test_analysis_dense_matches_the_oracle(frame, hop, C, B):
    from overiva_amd import BatchSTFT

    rng = np.random.default_rng(frame + C + B)
    n = hop * 9 + hop // 3
    x = rng.standard_normal((B, n, C))
    wa, ws = _windows(frame, hop)
    with BatchSTFT(n, C, frame, hop, win_a=wa, win_s=ws, B=B) as st:
        Xd = st.analysis_device(x)
        assert Xd.shape == (B, n // hop, frame // 2 + 1, C) and Xd.frames == [n // hop] * B and Xd.n_freq == frame // 2 + 1
        X = Xd.get_x()
    for b in range(B):
        err = orc.rel_err(X[b], so.analysis(x[b], frame, hop, wa))
        print(f"[analysis dense] L={frame} hop={hop} C={C} B={B} room {b}: rel_err {err:.2e}")
        assert err < TOL


@pytest.mark.parametrize("frame,hop,C", [(64, 32, 3), (512, 256, 8), (4096, 2048, 4), (128, 128, 1), (96, 32, 6), (64, 32, 7)])
def test_analysis_ragged_matches_the_oracle(frame, hop, C):
    """lengths that are and are not multiples of hop, a room of exactly one hop, a loud room in front of a silent-start room"""
    from overiva_amd import BatchSTFT

    rng = np.random.default_rng(frame + C)
    lens = [hop * 7, hop * 5 + 1, hop, hop * 6 + hop - 1, hop * 3]
    xs = [rng.standard_normal((n, C)) for n in lens]
    xs[2] *= 1e3                                       # loud, one hop long
    xs[3][: 2 * frame] = 0.0                          # silent start behind it: leakage across the boundary would show in frame 0
    xs[3] *= 1e-3
    wa, ws = _windows(frame, hop)
    with BatchSTFT(lens, C, frame, hop, win_a=wa, win_s=ws) as st:
        assert st.frames == [n // hop for n in lens]
        Xd = st.analysis_device(xs)
        assert Xd.shape == (sum(st.frames), frame // 2 + 1, C)
        Xs = Xd.get_x()
    for b, (x, X) in enumerate(zip(xs, Xs)):
        Xr = so.analysis(x, frame, hop, wa)
        assert X.shape == Xr.shape
        err = orc.rel_err(X, Xr)
        print(f"[analysis ragged] L={frame} hop={hop} C={C} room {b} ({lens[b]} samples): rel_err {err:.2e}")
        assert err < TOL
    assert not np.any(Xs[3][0])                        # frame 0 of the silent-start room: its own zero state and its own zeros only
    assert np.array_equal(so.analysis(xs[3], frame, hop, wa)[0], np.zeros_like(Xs[3][0]))


# ---- 2. solver on the device array = solver on the host array ------------------------------------------------------------------------
@pytest.mark.parametrize("C,k", [(4, 2), (8, 4)])
@pytest.mark.parametrize("model", ["laplace", "gauss"])
@pytest.mark.parametrize("init_eig", [False, True])
def test_solver_bits_do_not_depend_on_where_x_lives(C, k, model, init_eig):
    import overiva_amd as oa

    frame, hop, n_iter = 256, 128, 12
    # dense
    xd = np.stack([_room(100 + b, hop * 60, C, k)[0] for b in range(3)]).astype(np.float32)
    y, W = oa.separate_batch(xd, frame, hop, n_src=k, n_iter=n_iter, model=model, init_eig=init_eig, return_filters=True)
    info = oa.last_batch_info()
    assert info["audio"] is True and info["batched"] == 3 and "ragged" not in info
    with oa.BatchSTFT(hop * 60, C, frame, hop, B=3) as st:
        Xd = st.analysis_device(xd)
        Xh = Xd.get_x()
        Yh, Wh = oa.overiva_batch(Xh, n_src=k, n_iter=n_iter, model=model, init_eig=init_eig, return_filters=True)
        assert "audio" not in oa.last_batch_info()
        with oa.BatchPlan(3, st.frames[0], st.n_freq, C, k, model) as plan:
            plan.set_x_device(Xd.ptr, keepalive=Xd)
            plan.covariance()
            plan.set_w_eig() if init_eig else plan.set_w(None)
            plan.iterate(n_iter)
            Yd = plan.demix_device(True)
            assert Yd.shape == Yh.shape
            assert np.array_equal(Yd.get_x(), Yh)
            assert np.array_equal(plan.get_w(np.complex128).astype(np.complex64), Wh)
            y2 = st.synthesis_device(Yd)
    assert np.array_equal(W.astype(np.complex64), Wh)
    assert np.array_equal(y, y2)
    # ragged
    lens = [hop * 60, hop * 41 + 17, hop * 52]
    xr = [_room(200 + b, n, C, k)[0].astype(np.float32) for b, n in enumerate(lens)]
    ys, Wr = oa.separate_batch(xr, frame, hop, n_src=k, n_iter=n_iter, model=model, init_eig=init_eig, return_filters=True)
    info = oa.last_batch_info()
    assert info["audio"] is True and info["ragged"] is True and info["frames"] == [n // hop for n in lens]
    with oa.BatchSTFT(lens, C, frame, hop) as st:
        Xd = st.analysis_device(xr)
        Xs = Xd.get_x()
        Ys, Ws = oa.overiva_batch_ragged(Xs, n_src=k, n_iter=n_iter, model=model, init_eig=init_eig, return_filters=True)
        with oa.RaggedBatchPlan(st.frames, st.n_freq, C, k, model) as plan:
            plan.set_x_device(Xd.ptr, keepalive=Xd)
            plan.covariance()
            plan.set_w_eig() if init_eig else plan.set_w(None)
            plan.iterate(n_iter)
            for Ya, Yb in zip(plan.demix_device(True).get_x(), Ys):
                assert np.array_equal(Ya, Yb)
    assert np.array_equal(Wr.astype(np.complex64), Ws)


@pytest.mark.parametrize("update", ["demix", "switching"])
def test_ogive_bits_do_not_depend_on_where_x_lives(update):
    import overiva_amd as oa

    frame, hop, C = 256, 128, 4
    xd = np.stack([_room(300 + b, hop * 80, C, 1)[0] for b in range(3)]).astype(np.float32)
    kw = dict(n_iter=300, step_size=0.1, tol=1e-3, update=update)
    y, w = oa.separate_batch(xd, frame, hop, algorithm="ogive", return_filters=True, **kw)
    info = oa.last_batch_info()
    assert info["audio"] is True and info["algorithm"] == "ogive"
    assert y.shape == (3, hop * 80, 1) and y.dtype == np.float32
    with oa.BatchSTFT(hop * 80, C, frame, hop, B=3) as st:
        Xh = st.analysis_device(xd).get_x()
    Yh, wh = oa.ogive_batch(Xh, return_filters=True, **kw)
    ref = oa.last_batch_info()
    assert np.array_equal(w.astype(np.complex64), wh)
    assert info["epochs"] == ref["epochs"] and info["converged"] == ref["converged"]
    with pytest.raises(ValueError):
        oa.separate_batch([a for a in xd], frame, hop, algorithm="ogive")


# ---- 3. synthesis ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame,hop,C,k", [(64, 32, 3, 2), (512, 256, 8, 4), (4096, 2048, 4, 2), (128, 128, 1, 1), (256, 64, 2, 2)])
def test_synthesis_matches_the_oracle_and_stays_inside_a_room(frame, hop, C, k):
    import torch

    import overiva_amd as oa

    rng = np.random.default_rng(frame + k)
    lens = [hop * 7, hop * 5 + 1, hop, hop * 6 + hop - 1]
    xs = [rng.standard_normal((n, C)).astype(np.float32) for n in lens]
    wa, ws = _windows(frame, hop)
    with oa.BatchSTFT(lens, C, frame, hop, win_a=wa, win_s=ws) as st:
        Xd = st.analysis_device(xs)
        with oa.RaggedBatchPlan(st.frames, st.n_freq, C, k) as plan:
            plan.set_x_device(Xd.ptr, keepalive=Xd)
            plan.covariance()
            plan.set_w(None)                                      # (rooms of a few frames: the projected-back identity demix)
            Yd = plan.demix_device(True)
            Ys = Yd.get_x()
            ys = st.synthesis_device(Yd)
        for b, (Y, y) in enumerate(zip(Ys, ys)):
            yr = so.synthesis(Y, frame, hop, ws)
            assert y.shape == yr.shape == (st.frames[b] * hop, k) and y.dtype == np.float32
            err = orc.rel_err(y, yr)
            print(f"[synthesis] L={frame} hop={hop} K={k} room {b}: rel_err {err:.2e}")
            assert err < TOL
        # room b - 1's Y replaced by zeros: no sample of room b changes
        for b in range(1, len(lens)):
            Yz = [Y.copy() for Y in Ys]
            Yz[b - 1][:] = 0
            packed = torch.from_numpy(np.ascontiguousarray(np.concatenate(Yz, axis=0)).view(np.float32)).cuda()
            yz = st.synthesis_device(packed.data_ptr(), k)
            assert np.array_equal(yz[b], ys[b]) and not np.any(yz[b - 1])
        with pytest.raises(ValueError):
            st.synthesis_device(Yd.ptr, C + 1)                    # K outside 1..M


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------------
def _check_sir(ys, rooms, tag):
    for b, ((x, src), y) in enumerate(zip(rooms, ys)):
        n_out = x.shape[0] // HOP * HOP
        assert y.shape == (n_out, K)
        sir_in, sir_out = _sir(x[:n_out, :K], src), _sir(np.asarray(y, dtype=np.float64), src)
        print(f"[separate_batch {tag}] room {b} ({x.shape[0]} samples): time-domain SIR {sir_in:.1f} dB -> {sir_out:.1f} dB")
        assert sir_out > sir_in + 10.0


def test_separate_batch_separates_every_room_ragged():
    import overiva_amd as oa

    rooms = [_room(seed, n) for seed, n in ROOMS]
    ys = oa.separate_batch([x.astype(np.float32) for x, _ in rooms], L, HOP, n_src=K, n_iter=N_ITER)
    assert isinstance(ys, list) and all(y.dtype == np.float32 for y in ys)
    _check_sir(ys, rooms, "ragged")
    ys64 = oa.separate_batch([x for x, _ in rooms], L, HOP, n_src=K, n_iter=N_ITER)       # float64 in, float64 out
    assert all(y.dtype == np.float64 for y in ys64)
    _check_sir(ys64, rooms, "ragged f64")


def test_separate_batch_separates_every_room_dense():
    import overiva_amd as oa

    n = 102400
    rooms = [_room(seed, n) for seed, _ in ROOMS]
    x = np.stack([r[0] for r in rooms])
    y = oa.separate_batch(x.astype(np.float32), L, HOP, n_src=K, n_iter=N_ITER)
    assert y.shape == (7, n // HOP * HOP, K) and y.dtype == np.float32
    _check_sir(list(y), rooms, "dense")
    y64 = oa.separate_batch(x, L, HOP, n_src=K, n_iter=N_ITER)
    assert y64.dtype == np.float64 and np.array_equal(y64, y.astype(np.float64))      # a cast of the float32 result


# ---- 5. agreement with the composed path --------------------------------------------------------------------------------------------------
def test_agreement_with_the_composed_path():
    """per room stft.analysis -> overiva_batch_ragged -> stft.synthesis (what a user ran before) against separate_batch.

    hipFFT does not promise that a transform's bits are independent of the plan's batch count; measured on an MI355X (DESIGN.md
    3.7) they are for these plans: the batched plan gives every frame the bits of the one-room plan, so X, W and y of the two
    paths are bit-identical and the test asserts that (the stronger of the two forms; X within 2e-5 is the fallback form)."""
    import overiva_amd as oa
    from overiva_amd import stft

    xs = [_room(seed, n)[0].astype(np.float32) for seed, n in ROOMS]
    wa = stft.hann(L)
    ws = stft.compute_synthesis_window(wa, HOP)
    Xc = [stft.analysis(x, L, HOP, win=wa) for x in xs]
    with oa.BatchSTFT([len(x) for x in xs], M, L, HOP) as st:
        Xb = st.analysis_device(xs).get_x()
    errs = [orc.rel_err(a, b) for a, b in zip(Xb, Xc)]
    same = [bool(np.array_equal(a, b)) for a, b in zip(Xb, Xc)]
    print(f"[composed] X batched vs one-room plans: rel_err {['%.2e' % e for e in errs]}, bit-identical {same}")
    assert max(errs) < 2e-5
    Ys, Wc = oa.overiva_batch_ragged(Xc, n_src=K, n_iter=N_ITER, return_filters=True)
    yc = [stft.synthesis(Y, L, HOP, win=ws) for Y in Ys]
    yb, Wb = oa.separate_batch(xs, L, HOP, n_src=K, n_iter=N_ITER, return_filters=True)
    print(f"[composed] W bit-identical {bool(np.array_equal(Wb.astype(np.complex64), Wc))}, "
          f"y bit-identical {[bool(np.array_equal(a, b)) for a, b in zip(yb, yc)]}")
    assert all(same)
    assert np.array_equal(Wb.astype(np.complex64), Wc)
    for a, b in zip(yb, yc):
        assert a.shape == b.shape and np.array_equal(a, b)


# ---- 6. handles -----------------------------------------------------------------------------------------------------------------------------
def test_handles_are_reusable_and_kept_alive():
    import gc

    import overiva_amd as oa

    frame, hop, C = 128, 64, 3
    rng = np.random.default_rng(5)
    lens = [hop * 20, hop * 13 + 5]
    xa = [rng.standard_normal((n, C)) for n in lens]
    xb = [rng.standard_normal((n, C)) for n in lens]
    wa, _ = _windows(frame, hop)
    st = oa.BatchSTFT(lens, C, frame, hop)
    Xa = st.analysis_device(xa).get_x()
    Xb = st.analysis_device(xb).get_x()                       # the same handle, other audio
    for x, X in zip(xa + xb, Xa + Xb):
        assert orc.rel_err(X, so.analysis(x, frame, hop, wa)) < TOL
    Xd = st.analysis_device(xa)
    assert Xd.owner is st
    plan = oa.RaggedBatchPlan(st.frames, st.n_freq, C, 2)
    plan.set_x_device(Xd.ptr, keepalive=Xd)
    assert plan._keep is Xd
    del st, Xd
    gc.collect()                                              # the plan keeps X (and through it the handle) alive
    plan.covariance()
    plan.set_w(None)
    plan.iterate(2)
    Y = plan.demix_device(True)
    assert Y.owner is plan and all(np.all(np.isfinite(y)) for y in Y.get_x())
    st2 = plan._keep.owner
    y = st2.synthesis_device(Y)
    assert [a.shape for a in y] == [(n // hop * hop, 2) for n in lens]
    plan.close()
    plan.close()
    st2.close()
    st2.close()                                               # twice
    with pytest.raises(RuntimeError):
        st2.analysis_device(xa)
