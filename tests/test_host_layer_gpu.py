"""The host layer the handles share (csrc/host_util.h) on the GPU: the graph caches of a plan and of a batch across evictions, the
captured chunk of OGIVE epochs across recaptures, and the calling thread's current device after a call on a handle of another
device.  Everything is compared bit for bit against the same work done without the machinery under test."""
import numpy as np
import pytest

from oracle import overiva_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oa():
    import overiva_amd

    overiva_amd._lib.load()
    return overiva_amd


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- graph cache of a plan: seven lengths against a cache of six, then an evicted and a kept length ---------------------------
def test_plan_graph_cache_eviction_bits(oa):
    T, F, M, K = 64, 24, 4, 2
    X = orc.synth_mixture(T, F, M, K, seed=11).astype(np.complex64)
    lengths = [1, 2, 3, 4, 5, 6, 7, 1, 3]
    assert sum(lengths) == 32
    out = []
    for graph in (True, False):
        with oa.Plan(T, F, M, K) as p:
            p.set_precision("mixed")
            p.set_x(X)
            p.covariance()
            p.set_w(None)
            p.use_graph(graph)
            for n in (lengths if graph else [32]):
                p.iterate(n)
            out.append((p.get_w(np.complex128), p.demix()))
    (Wg, Yg), (We, Ye) = out
    assert np.all(np.isfinite(We)) and np.all(np.isfinite(Ye))
    assert _same_bits(Wg, We)
    assert _same_bits(Yg, Ye)


# ---- graph cache of a batch: five lengths against a cache of four, then two evicted ones -----------------------------------------
def _batch_plans(oa):
    B, T, F, M, K = 2, 40, 20, 3, 2
    Xd = np.stack([orc.synth_mixture(T, F, M, K, seed=21 + b) for b in range(B)]).astype(np.complex64)
    frames = [40, 17]
    Xr = [orc.synth_mixture(t, F, M, K, seed=31 + b).astype(np.complex64) for b, t in enumerate(frames)]
    return {"dense": (lambda: oa.BatchPlan(B, T, F, M, K), Xd), "ragged": (lambda: oa.RaggedBatchPlan(frames, F, M, K), Xr)}


@pytest.mark.parametrize("kind", ["dense", "ragged"])
def test_batch_graph_cache_eviction_bits(oa, kind):
    make, X = _batch_plans(oa)[kind]
    lengths = [1, 2, 3, 4, 5, 1, 2]
    assert sum(lengths) == 18
    out = []
    for steps in (lengths, [18]):
        with make() as p:
            p.set_x(X)
            p.covariance()
            p.set_w(None)
            for n in steps:
                p.iterate(n)
            Y = p.demix()
            out.append((p.get_w(np.complex128), np.concatenate(Y) if isinstance(Y, list) else Y))
    (Wc, Yc), (Wf, Yf) = out
    assert np.all(np.isfinite(Wf)) and np.all(np.isfinite(Yf))
    assert _same_bits(Wc, Wf)
    assert _same_bits(Yc, Yf)


# ---- OGIVE chunk graph: recaptured on a changed length and on a changed phase of the switching cadence ---------------------------
@pytest.mark.parametrize("kind", ["plan", "batch"])
def test_ogive_chunk_graph_recapture_bits(oa, kind):
    T, F, M = 48, 10, 3
    if kind == "plan":
        X = orc.synth_mixture(T, F, M, 1, seed=41).astype(np.complex64)
        make = lambda: oa.Plan(T, F, M, 1)
    else:
        X = np.stack([orc.synth_mixture(T, F, M, 1, seed=51 + b) for b in range(2)]).astype(np.complex64)
        make = lambda: oa.BatchPlan(2, T, F, M, 1)
    graph_chunks = [(0, 8), (8, 8), (16, 12), (28, 8)]          # >= 8 epochs: captured
    eager_chunks = [(e, 4) for e in range(0, 36, 4)]             # < 8 epochs: launched one by one
    out = []
    for chunks in (graph_chunks, eager_chunks):
        with make() as p:
            p.set_x(X)
            p.covariance()
            p.set_w(None)
            p.ogive_begin("switching", "laplace")
            ran = 0
            for first, n in chunks:
                ran = ran + np.asarray(p.ogive_iterate(first, n, 0.1, 0.0)[0])
            out.append((ran, p.get_w(np.complex128)))
    (ran_g, Wg), (ran_e, We) = out
    assert np.all(ran_g == 36) and np.all(ran_e == 36)
    assert np.all(np.isfinite(We))
    assert _same_bits(Wg, We)


# ---- the calling thread's current device ------------------------------------------------------------------------------------
def _calls_on(oa, dev, after):
    """one handle of every kind on device ``dev`` and one call each; ``after(what)`` behind every call"""
    import torch

    from overiva_amd import exchange, separate, stft

    rng = np.random.default_rng(5)
    x = rng.standard_normal((1024, 2)).astype(np.float32)
    with stft.STFT(1024, 2, 64, 32, device=dev) as s:
        after("STFT create")
        Xs = s.analysis(x)
        after("STFT analysis")
        s.synthesis(Xs)
        after("STFT synthesis")
    after("STFT destroy")
    rooms = [rng.standard_normal((n, 2)).astype(np.float32) for n in (1024, 700)]
    with separate.BatchSTFT([1024, 700], 2, 64, 32, device=dev) as bs:
        after("BatchSTFT create")
        Xd = bs.analysis_device(rooms)
        after("BatchSTFT analysis")
        bs.synthesis_device(Xd)
        after("BatchSTFT synthesis")
    after("BatchSTFT destroy")
    X = orc.synth_mixture(40, 20, 3, 2, seed=61).astype(np.complex64)
    with oa.Plan(40, 20, 3, 2, device=dev) as p:
        after("Plan create")
        p.set_x(X)
        p.covariance()
        p.set_w(None)
        p.iterate(2)
        p.demix()
        after("Plan calls")
    after("Plan destroy")
    with oa.BatchPlan(2, 40, 20, 3, 2, device=dev) as b:
        after("BatchPlan create")
        b.set_x(np.stack([X, X]))
        b.covariance()
        b.set_w(None)
        b.iterate(2)
        b.demix()
        after("BatchPlan calls")
    after("BatchPlan destroy")
    part = torch.zeros(64, dtype=torch.float32, device=f"cuda:{dev}")
    stream = torch.cuda.Stream(device=dev)
    with exchange.PushExchange(dev, 0, 1, part.data_ptr(), part.numel() * 4, stream.cuda_stream) as ex:      # a world of one
        after("PushExchange create")
        ex.gather()
        after("PushExchange push / wait")
        assert ex.poll(1000)
        after("PushExchange poll")
    after("PushExchange destroy")


def test_calls_leave_current_device(oa):
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda:0")
    torch.zeros(1, device="cuda:1")

    def still_on_0(what):
        assert torch.cuda.current_device() == 0, what

    _calls_on(oa, 1, still_on_0)


# ---- one owner of every handle's device memory, stream and events (DeviceArena, HandleStream) ------------------------------------
def _live():
    """(buffers, bytes) the library has handed out and not taken back, over all handles of the process"""
    import ctypes as C

    from overiva_amd import _lib

    n, nbytes = C.c_longlong(), C.c_longlong()
    _lib.check(_lib.load().oiva_test_live_buffers(C.byref(n), C.byref(nbytes)))
    return n.value, nbytes.value


def _prepared(p, X, iters=2):
    p.set_x(X)
    p.covariance()
    p.set_w(None)
    if iters:
        p.iterate(iters)
    return p


def _leak_plan_c128(oa, mid):
    T, F, M, K = 40, 20, 3, 2
    X = orc.synth_mixture(T, F, M, K, seed=61).astype(np.complex128)
    with oa.Plan(T, F, M, K) as p:
        _prepared(p, X)
        p.save_w()
        p.set_io_slab(F * K * 16)              # one frame row per slab: the ring and its three staging slots
        p.demix(dtype=np.complex128)
        p.set_io_slab(0)                       # ... and the staged copy of a small output
        p.demix(dtype=np.complex128)
        mid()
    with oa.Plan(T, F, M, 1) as p:
        _prepared(p, X, iters=0)
        p.ogive_begin("switching", "laplace")
        p.ogive_iterate(0, 2, 0.1, 0.0)
        mid()


def _leak_plan_padded(oa, mid):
    with oa.Plan(40, 20, 9, 2) as p:
        _prepared(p, orc.synth_mixture(40, 20, 9, 2, seed=62).astype(np.complex64)).demix()
        mid()


def _leak_plan_wide(oa, mid):
    with oa.Plan(24, 8, 17, 2) as p:
        _prepared(p, orc.synth_mixture(24, 8, 17, 2, seed=63).astype(np.complex64)).demix()
        mid()


def _leak_plan_resident(oa, mid):
    T, F, M, K = 64, 32, 4, 2
    with oa.Plan(T, F, M, K) as p:
        if not p.resident_info()["qualifies"]:
            pytest.skip("the shape does not qualify for the X-resident iteration on this device")
        p.set_precision("mixed")
        _prepared(p, orc.synth_mixture(T, F, M, K, seed=64).astype(np.complex64), iters=0)
        p.set_resident(True)
        p.iterate(2)
        p.sync()
        mid()
        p.set_resident(False)
        with_block = _live()
        p.set_resident_splits(0)               # the buffers of the old geometry go at once
        assert _live()[0] == with_block[0] - 1 and _live()[1] < with_block[1]
        mid()


def _leak_batch_dense(oa, mid):
    B, T, F, M, K = 2, 40, 20, 3, 2
    rng = np.random.default_rng(8)
    X = np.stack([orc.synth_mixture(T, F, M, K, seed=21 + b) for b in range(B)])
    with oa.BatchPlan(B, T, F, M, K) as b:
        _prepared(b, X.astype(np.complex128))
        b.get_cx()
        b.demix(dtype=np.complex128)
        mid()
    with oa.BatchPlan(B, T, F, M, 1) as b:
        _prepared(b, X.astype(np.complex64), iters=0)
        b.ogive_begin("switching", "laplace")
        b.ogive_iterate(0, 2, 0.1, 0.0)
        mid()
    with oa.BatchPlan(B, T, F, M, M) as b:
        _prepared(b, X.astype(np.complex64), iters=0)
        for L in (2, 3):                       # (another component count: the state is freed and taken again)
            b.ilrma_begin(rng.uniform(0.5, 1.5, (B, M, F, L)), rng.uniform(0.5, 1.5, (B, M, L, T)))
            b.ilrma_iterate(1)
        mid()


def _leak_batch_ragged(oa, mid):
    frames, F, M, K = [40, 17], 20, 3, 2
    X = [orc.synth_mixture(t, F, M, K, seed=31 + i).astype(np.complex64) for i, t in enumerate(frames)]
    with oa.RaggedBatchPlan(frames, F, M, K) as b:
        b.set_x(X)
        b.covariance()
        b.set_w_pca()
        b.project_device()
        b.iterate(2)
        b.demix()
        mid()


def _leak_bss_eval(oa, mid):
    from overiva_amd import metrics

    rng = np.random.default_rng(7)
    lengths, N = [700, 1024], 2
    ref = [rng.standard_normal((N, n)) for n in lengths]
    est = [r + 0.1 * rng.standard_normal(r.shape) for r in ref]
    for max_group in (0, 1):                   # (1: the rooms run in groups, the group buffers are sized for one room)
        with metrics.BssEval(lengths, N, filter_length=16, max_group=max_group) as ev:
            assert ev.group == (1 if max_group else 2)
            ev.set_signals(ref, est)
            ev.run()
            ev.get_criteria()
            mid()


_LEAK_CASES = {"plan_c128": _leak_plan_c128, "plan_padded": _leak_plan_padded, "plan_wide": _leak_plan_wide,
               "plan_resident": _leak_plan_resident, "batch_dense": _leak_batch_dense, "batch_ragged": _leak_batch_ragged,
               "bss_eval": _leak_bss_eval}


@pytest.mark.parametrize("kind", sorted(_LEAK_CASES))
def test_no_handle_leaks(oa, kind):
    """every buffer a handle took, at creation or on first use, is back after its destroy: the library's count of live buffers
    and of their bytes returns to what it was, and was larger while the handle lived"""
    import gc

    gc.collect()
    before = _live()
    during = []
    _LEAK_CASES[kind](oa, lambda: during.append(_live()))
    assert _live() == before
    assert during and all(n > before[0] and nbytes > before[1] for n, nbytes in during)


def test_no_handle_leaks_one_call_on_every_kind(oa):
    """STFT, BatchSTFT, Plan, BatchPlan and PushExchange as ``_calls_on`` uses them: more live buffers than before behind every
    call on a live handle, the same as before behind every destroy"""
    import gc

    gc.collect()
    before = _live()
    seen = {}
    _calls_on(oa, 0, lambda what: seen.__setitem__(what, _live()))
    destroys = [w for w in seen if w.endswith("destroy")]
    assert len(destroys) == 5 and len(seen) > 10
    for what, (n, nbytes) in seen.items():
        if what in destroys:
            assert (n, nbytes) == before, what
        else:
            assert n > before[0] and nbytes > before[1], what


def test_regrown_buffers_replace_the_old_ones(oa):
    """a buffer that is grown is a new one in place of the old: more bytes, not more buffers"""
    T, F, M = 64, 24, 4
    with oa.Plan(T, F, M, 2) as p:
        _prepared(p, orc.synth_mixture(T, F, M, 2, seed=65).astype(np.complex64))
        n0, b0 = _live()
        splits = p.cov_splits()
        p.set_cov_splits(splits + 3)
        n1, b1 = _live()
        assert n1 == n0 and b1 > b0
        p.set_cov_splits(splits)               # (fewer splits fit in what is there)
        assert _live() == (n1, b1)
        p.iterate(1)
        p.sync()
    with oa.Plan(T, F, M, 1) as p:
        _prepared(p, orc.synth_mixture(T, F, M, 1, seed=66).astype(np.complex64), iters=0)
        n0, _ = _live()
        p.ogive_begin("demix", "laplace")
        first = _live()
        assert first[0] > n0
        p.ogive_begin("switching", "gauss")
        assert _live() == first


def test_setters_and_x_installation_drop_graphs(oa):
    """a geometry setter and a new X between replays of captured graphs: the same bits as without graphs"""
    T, F, M, K = 64, 24, 4, 2
    X = orc.synth_mixture(T, F, M, K, seed=11).astype(np.complex64)
    out = []
    for graph in (True, False):
        with oa.Plan(T, F, M, K) as p:
            p.set_precision("mixed")
            _prepared(p, X, iters=0)
            p.use_graph(graph)
            p.iterate(3)
            p.set_pow_splits(2)
            p.iterate(3)
            p.set_x(X.copy())
            p.covariance()
            p.iterate(3)
            out.append((p.get_w(np.complex128), p.demix()))
    (Wg, Yg), (We, Ye) = out
    assert np.all(np.isfinite(We)) and np.all(np.isfinite(Ye))
    assert _same_bits(Wg, We)
    assert _same_bits(Yg, Ye)


def test_staged_copies_plan(oa):
    """complex128 in and out of a plan goes through the staged copy: the bits of the complex64 path, dense and with a row pitch
    larger than the row, for the small-output form and for the ring of slabs"""
    T, F, M, K, Fa, f0 = 40, 20, 3, 2, 25, 2
    Xa = orc.synth_mixture(T, Fa, M, K, seed=67).astype(np.complex128)
    for X128, at in ((np.ascontiguousarray(Xa[:, f0:f0 + F]), 0), (Xa, f0)):
        with oa.Plan(T, F, M, K) as p, oa.Plan(T, F, M, K) as q:
            p.set_x(X128, f0=at)
            q.set_x(np.ascontiguousarray(Xa[:, f0:f0 + F]).astype(np.complex64))
            for h in (p, q):
                h.covariance()
                h.set_w(None)
                h.iterate(2)
            assert _same_bits(p.get_cx(), q.get_cx())
            Y64 = q.demix()
            assert _same_bits(p.demix(), Y64)
            for slab in (0, F * K * 16):       # the staged copy of a small output | one frame row per slab of the ring
                p.set_io_slab(slab)
                assert _same_bits(p.demix(dtype=np.complex128), Y64.astype(np.complex128))
                wide = np.zeros((T, Fa, K), np.complex128)
                p.demix(out=wide, f0=f0)
                assert _same_bits(np.ascontiguousarray(wide[:, f0:f0 + F]), Y64.astype(np.complex128))
                wide[:, f0:f0 + F] = 0
                assert not wide.any()


def test_staged_copies_batch(oa):
    B, T, F, M, K = 2, 40, 20, 3, 2
    X128 = np.stack([orc.synth_mixture(T, F, M, K, seed=21 + b) for b in range(B)]).astype(np.complex128)
    with oa.BatchPlan(B, T, F, M, K) as p, oa.BatchPlan(B, T, F, M, K) as q:
        p.set_x(X128)
        q.set_x(X128.astype(np.complex64))
        for h in (p, q):
            h.covariance()
            h.set_w(None)
            h.iterate(2)
        assert _same_bits(p.get_cx(), q.get_cx())
        Y64 = q.demix()
        assert _same_bits(p.demix(), Y64)
        assert _same_bits(p.demix(dtype=np.complex128), Y64.astype(np.complex128))
