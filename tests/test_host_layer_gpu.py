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
