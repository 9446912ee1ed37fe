"""sweep_batch() without a GPU: the ABI is declared, bound and exported, every refusal comes before the library is touched (in
Python) or before a device call (in the library: on a machine without a GPU any device call gives ERR_HIP, so ERR_ARG shows the
order), the skip rules and the checkpoint lists, and the scenes of tests/helpers/sweep_chain.py order their unprocessed
microphones with a clear gap, not as the identity in every room and not the same way in all rooms."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

import room_oracle as ro  # noqa: E402
import sweep_chain as sc  # noqa: E402

HEADER = os.path.join(os.path.dirname(HERE), "include", "overiva_hip.h")
SYMBOLS = ("oiva_sweep_create", "oiva_sweep_destroy", "oiva_sweep_set_filler", "oiva_sweep_take_mix", "oiva_sweep_evaluate",
           "oiva_sweep_phase_ms", "oiva_sweep_get_order", "oiva_sweep_get_signals", "oiva_bstft_analysis_dev",
           "oiva_bstft_synthesis_keep")
KERNELS = ("sweep_cast_kernel", "sweep_std_kernel", "sweep_order_kernel", "sweep_align_kernel")


@pytest.fixture(scope="module")
def lib():
    from overiva_amd import _lib, build

    build.build_library()
    return _lib.load()


def test_symbols_declared_bound_and_exported(lib):
    import overiva_amd
    from overiva_amd import _lib, build, sweep

    header = open(HEADER).read()
    for sym in SYMBOLS:
        assert re.search(r"oiva_status\s+%s\s*\(" % sym, header), sym
        assert sym in _lib.SIGNATURES, sym
        assert hasattr(lib, sym), sym
    assert {s for s in _lib.SIGNATURES if s.startswith("oiva_sweep_")} == {s for s in SYMBOLS if s.startswith("oiva_sweep_")}
    assert "kernels_sweep.hip" in build.SOURCES and "sweep.hip" in build.SOURCES
    for name in ("sweep_batch", "SweepBatch"):
        assert name in overiva_amd.__all__ and getattr(overiva_amd, name) is getattr(sweep, name)
    assert issubclass(sweep.SweepBatch, _lib.Handle)
    for method in ("set_signals", "set_filler", "open_group", "convolve", "mix", "take_mix", "evaluate", "get_order", "get_eval_signals"):
        assert callable(getattr(sweep.SweepBatch, method))
    for doc in (sweep.__doc__, sweep.sweep_batch.__doc__):
        assert "What still crosses the bus" in doc


def test_sweep_kernels_use_no_scratch_memory():
    from overiva_amd import build

    build.build_library()
    usage = build.kernel_usage(("kernels_sweep",))
    for kernel in KERNELS:
        hit = [u for name, u in usage.items() if kernel in name]
        assert len(hit) == 1, (kernel, sorted(usage))
        assert hit[0]["scratch"] == 0, (kernel, hit[0])
    assert all(any(k in name for k in KERNELS) for name in usage), sorted(usage)


# ---- the library: arguments before any device call ----------------------------------------------------------------------------
def _create(lib, n_out=(500, 600), M=3, K=2, frame=64, hop=32, ref_mic=0, Lf=16, out=True):
    h = C.c_void_p()
    ns = (C.c_int * len(n_out))(*n_out)
    return lib.oiva_sweep_create(C.byref(h) if out else None, 0, len(n_out), ns, M, K, frame, hop, ref_mic, Lf, None)


def test_create_checks_its_arguments_before_the_device(lib):
    from overiva_amd import _lib
    from conftest import has_gpu

    bad = [dict(out=False), dict(M=0), dict(M=9), dict(K=0), dict(K=4), dict(M=8, K=8), dict(frame=63), dict(frame=0), dict(hop=0),
           dict(hop=65), dict(ref_mic=3), dict(ref_mic=-1), dict(Lf=0), dict(Lf=513), dict(n_out=(500, 0)),
           dict(n_out=(500, 63)), dict(n_out=(500, 32)), dict(n_out=(31, 500), frame=32, hop=32)]
    for kw in bad:
        assert _create(lib, **kw) == _lib.ERR_ARG, kw
    msg = lambda: lib.oiva_last_error().decode()      # noqa: E731
    assert _create(lib, n_out=(500, 63)) == _lib.ERR_ARG and "room 1 is too short for one complete frame" in msg()
    h = C.c_void_p()
    assert lib.oiva_sweep_create(C.byref(h), 0, 1, None, 3, 2, 64, 32, 0, 16, None) == _lib.ERR_ARG
    if not has_gpu():      # the control: arguments in order reach the device, which is not there; m_b = 64 - 32 = 32 >= 1 passes
        assert _create(lib, n_out=(500, 64)) == _lib.ERR_HIP


def test_null_handles_and_pointers(lib):
    from overiva_amd import _lib

    x = np.zeros(4)
    p, out = _lib.ptr(x), C.c_void_p()
    one = C.c_void_p(8)           # a handle that is not null: never followed, a null argument is met first
    assert lib.oiva_sweep_destroy(None) == _lib.OK
    assert lib.oiva_sweep_set_filler(None, p) == lib.oiva_sweep_set_filler(one, None) == _lib.ERR_ARG
    assert lib.oiva_sweep_take_mix(None, one, 0, one, C.byref(out)) == _lib.ERR_ARG
    assert lib.oiva_sweep_take_mix(one, None, 0, one, C.byref(out)) == lib.oiva_sweep_take_mix(one, one, 0, None, C.byref(out)) == _lib.ERR_ARG
    assert lib.oiva_sweep_take_mix(one, one, 0, one, None) == _lib.ERR_ARG
    for args in ((None, one, p, 2, 1, one, None), (one, None, p, 2, 1, one, None), (one, one, None, 2, 1, one, None),
                 (one, one, p, 2, 1, None, None)):
        assert lib.oiva_sweep_evaluate(*args) == _lib.ERR_ARG, args
    assert lib.oiva_sweep_phase_ms(None, (C.c_float * 1)()) == lib.oiva_sweep_phase_ms(one, None) == _lib.ERR_ARG
    assert lib.oiva_sweep_get_order(None, (C.c_int * 4)(), p) == lib.oiva_sweep_get_order(one, None, p) == _lib.ERR_ARG
    assert lib.oiva_sweep_get_order(one, (C.c_int * 4)(), None) == _lib.ERR_ARG
    assert lib.oiva_sweep_get_signals(None, one, p, p) == lib.oiva_sweep_get_signals(one, None, p, p) == _lib.ERR_ARG
    assert lib.oiva_sweep_get_signals(one, one, None, p) == lib.oiva_sweep_get_signals(one, one, p, None) == _lib.ERR_ARG
    assert lib.oiva_bstft_analysis_dev(None, p, 1, C.byref(out)) == lib.oiva_bstft_analysis_dev(one, None, 1, C.byref(out)) == _lib.ERR_ARG
    assert lib.oiva_bstft_analysis_dev(one, p, 1, None) == _lib.ERR_ARG
    assert lib.oiva_bstft_synthesis_keep(None, p, 1, C.byref(out)) == lib.oiva_bstft_synthesis_keep(one, None, 1, C.byref(out)) == _lib.ERR_ARG
    assert lib.oiva_bstft_synthesis_keep(one, p, 1, None) == _lib.ERR_ARG


# ---- Python: every refusal before the library ---------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """any use of the library fails the test: validation must come first"""
    from overiva_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was touched before the arguments were validated")

    monkeypatch.setattr(_lib, "load", boom)
    import overiva_amd

    return overiva_amd


def _good(B=2, S=4, M=3, n=900):
    rng = np.random.default_rng(0)
    dim = np.tile([4.0, 5.0, 3.0], (B, 1))
    return dict(signals=rng.standard_normal((B, S, n)), room_dim=dim, sources=dim[:, None, :] * rng.uniform(0.15, 0.85, (B, S, 3)),
                mics=dim[:, None, :] * rng.uniform(0.15, 0.85, (B, M, 3)), frame=64, hop=32, n_targets=2, fs=8000, max_order=2,
                rir_length=200, filter_length=16)


def _entry(algo, **kwargs):
    return {"x": {"algo": algo, "kwargs": kwargs}}


def _mics(M):
    g = _good()
    return g["room_dim"][:, None, :] * np.linspace(0.2, 0.8, M)[None, :, None] * np.ones((2, 1, 3))


G = _good()
BAD = {
    "nine microphones": dict(mics=_mics(9)),
    "eight targets": dict(mics=_mics(8), n_targets=8, signals=np.ones((2, 9, 900)),
                          sources=G["room_dim"][:, None, :] * np.linspace(0.25, 0.75, 9)[None, :, None] * np.ones((2, 1, 3))),
    "more targets than microphones": dict(n_targets=4, sinr=np.inf),
    "no targets": dict(n_targets=0),
    "ilrma": dict(algorithms=_entry("ilrma", n_iter=10)),
    "unknown algo": dict(algorithms=_entry("fastica")),
    "entry without algo": dict(algorithms={"x": {"kwargs": {}}}),
    "algorithms not a dict": dict(algorithms=["overiva"]),
    "no algorithms": dict(algorithms={}),
    "unknown kwarg": dict(algorithms=_entry("overiva", n_iterations=3)),
    "ogive kwarg on overiva": dict(algorithms=_entry("overiva", step_size=0.1)),
    "negative n_iter": dict(algorithms=_entry("overiva", n_iter=-1)),
    "n_iter 2.5": dict(algorithms=_entry("auxiva", n_iter=2.5)),
    "model": dict(algorithms=_entry("overiva", model="student")),
    "W0 shape": dict(algorithms=_entry("overiva", W0=np.ones((33, 3, 3)))),
    "ogive update": dict(n_targets=1, algorithms=_entry("ogive", update="both")),
    "ogive, lengths differ": dict(n_targets=1, signals=[G["signals"][0], G["signals"][1][:, :800]], algorithms=_entry("ogive")),
    "odd frame": dict(frame=63),
    "frame 64.0": dict(frame=64.0),
    "hop above frame": dict(hop=65),
    "hop zero": dict(hop=0),
    "window length": dict(win_a=np.ones(32)),
    "filter_length zero": dict(filter_length=0),
    "filter_length 513": dict(filter_length=513),
    "filter_length 16.0": dict(filter_length=16.0),
    "ref_mic": dict(ref_mic=3),
    "sources_var": dict(sources_var=[1.0]),
    "noise shape": dict(noise=np.zeros((2, 1099))),
    "filler rank": dict(filler=np.zeros(1099)),
    "filler batch": dict(filler=np.zeros((3, 1099))),
    "filler nan": dict(filler=np.full((2, 1099), np.nan)),
    "filler complex": dict(filler=np.zeros((2, 1099), complex)),
    "too short for a frame": dict(signals=G["signals"][:, :, :5], rir_length=40, frame=64, hop=32),
    "overdet_algos a string": dict(overdet_algos="overiva"),
    "max_group": dict(max_group=-1),
    "source outside": dict(sources=G["sources"] + 10.0),
    "max_order": dict(max_order=33),
    "signals rank": dict(signals=G["signals"][0]),
}


@pytest.mark.parametrize("bad", sorted(BAD))
def test_validation_before_device(no_device, bad):
    with pytest.raises(ValueError):
        no_device.sweep_batch(**dict(_good(), **BAD[bad]))


def test_the_ilrma_refusal_names_ilrma(no_device):
    with pytest.raises(ValueError, match="ILRMA"):
        no_device.sweep_batch(**dict(_good(), algorithms={"ilrma_1": {"algo": "ilrma", "kwargs": {"n_iter": 10}}}))


def test_the_short_room_refusal_names_the_room(no_device):
    sig = [G["signals"][0], G["signals"][1][:, :5]]
    with pytest.raises(ValueError, match="room 1 is too short for one complete frame"):
        no_device.sweep_batch(**dict(_good(), signals=sig, rir_length=40))


def test_refused_under_bin_sharding(no_device, monkeypatch):
    from overiva_amd import sharded

    monkeypatch.setattr(sharded, "active_group", lambda: object())
    with pytest.raises(ValueError, match="does not run under enable_bin_sharding"):
        no_device.sweep_batch(**_good())


@pytest.mark.parametrize("extra", [dict(), dict(monitor_convergence=True), dict(n_targets=1, algorithms=_entry("ogive", n_iter=300, tol=1e-4)),
                                   dict(algorithms=_entry("auxiva_pca", n_iter=5, model="gauss")), dict(filler=np.zeros((2, 1200))),
                                   dict(noise=np.zeros((2, 1099, 3)), sources_var=[1.0, 0.5]), dict(rir_length=None, max_group=1),
                                   dict(algorithms=_entry("auxiva", W0=np.ones((33, 3, 3)) + 0j, init_eig=False, proj_back=False))])
def test_good_arguments_reach_the_library(no_device, extra):
    """the control of the refusals: arguments that are in order pass every check and go on to the library"""
    with pytest.raises(AssertionError, match="the library was touched"):
        no_device.sweep_batch(**dict(_good(), **extra))


def test_skip_rules_and_entries():
    """auxiva_pca is skipped with one target and ogive with more than one (overiva_sim.py:250-255); a pasted configuration block
    goes through; "auxiva" runs all channels and is reordered, the over-determined algorithms keep their order"""
    from overiva_amd import sweep

    block = {"auxiva_laplace": {"algo": "auxiva", "kwargs": {"n_iter": 100, "proj_back": True, "model": "laplace"}},
             "auxiva_pca_gauss": {"algo": "auxiva_pca", "kwargs": {"n_iter": 100, "proj_back": True, "model": "gauss"}},
             "overiva_laplace": {"algo": "overiva", "kwargs": {"n_iter": 100, "proj_back": True, "init_eig": False, "model": "laplace"}},
             "ogive_laplace": {"algo": "ogive", "kwargs": {"n_iter": 4000, "step_size": 0.1, "tol": 1e-3, "update": "demix",
                                                           "proj_back": True, "model": "laplace", "init_eig": False}}}
    run = lambda K: sweep._check_algorithms(block, K, [1100, 1100], 3, 64, 32, None, None, sweep.OVERDET_ALGOS)      # noqa: E731
    two = run(2)
    assert [e["name"] for e in two] == ["auxiva_laplace", "auxiva_pca_gauss", "overiva_laplace"]
    assert [e["n_src"] for e in two] == [3, 2, 2] and [e["reorder"] for e in two] == [True, False, False]
    one = run(1)
    assert [e["name"] for e in one] == ["auxiva_laplace", "overiva_laplace", "ogive_laplace"]
    assert [e["n_src"] for e in one] == [3, 1, 1] and one[2]["ogive"] == {"step_size": 0.1, "tol": 1e-3, "update": "demix"}
    default = sweep._check_algorithms(None, 2, [1100, 1100], 3, 64, 32, None, None, sweep.OVERDET_ALGOS)
    assert [(e["name"], e["algo"], e["n_iter"], e["n_src"]) for e in default] == [("overiva", "overiva", 20, 2)]
    renamed = sweep._check_algorithms({"a": {"algo": "overiva", "kwargs": {}}}, 2, [1100, 1100], 3, 64, 32, None, None, ("a",))
    assert renamed[0]["reorder"] is True          # overdet_algos holds algo values, as the issue of the reference's `name` does


@pytest.mark.parametrize("n_iter,plain,watched", [(0, [0, 0], [0]), (10, [0, 10], [0, 10]), (20, [0, 20], [0, 10, 20]),
                                                  (25, [0, 25], [0, 10, 20, 25])])
def test_checkpoint_lists(n_iter, plain, watched):
    from overiva_amd.sweep import checkpoints

    for algo in ("overiva", "auxiva"):
        assert checkpoints(algo, n_iter) == plain and checkpoints(algo, n_iter, True) == watched
    assert checkpoints("auxiva_pca", n_iter) == checkpoints("auxiva_pca", n_iter, True) == plain      # its ends only
    assert checkpoints("ogive", n_iter) == plain and checkpoints("ogive", n_iter, True) == ([0, n_iter] if n_iter else [0])
    assert checkpoints("ogive", 250, True) == [0, 100, 200, 250] and checkpoints("ogive", 200, True) == [0, 100, 200]
    with pytest.raises(ValueError):
        checkpoints("ilrma", n_iter)


# ---- the scenes: the unprocessed microphones order with a clear gap ------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "ragged"])
def test_scene_orders_its_microphones_clearly(kind):
    """The "init" evaluation orders the microphones by standard deviation.  From the NumPy restatement of the room simulation:
    the gap between neighbouring standard deviations of the mix is far above what the STFT round trip in float32 (1e-6) or the
    1e-9 of the chain's own assertion could close; the order is not the identity in every room and differs between rooms."""
    args = sc.scene(kind)
    orders = []
    for b in range(3):
        h, _ = ro.rir(args["room_dim"][b], args["sources"][b], args["mics"][b], args["absorption"][b], sc.FS, 343.0, sc.ORDER,
                      args["rir_length"])
        prem = ro.premix(np.asarray(args["signals"][b]), h)
        n_out = prem.shape[2]
        mix, _ = ro.mix_down(prem, sc.K, sc.SINR, sc.SNR, sc.REF_MIC, np.asarray(args["sources_var"]), args["_noise"][b][:n_out])
        assert sc.eval_length(n_out) >= 1
        std = mix[:n_out // sc.HOP * sc.HOP].astype(np.float32).astype(np.float64).std(axis=0)
        print(f"{kind} room {b}: n_out {n_out}, std {std}, gap {sc.gaps(std):.3e}")
        assert sc.gaps(std) > 1e-3
        orders.append(tuple(np.argsort(-std, kind="stable")))
    assert any(o != (0, 1, 2) for o in orders) and len(set(orders)) > 1, orders
