"""measure_rt60_batch() / absorption_for_rt60() without a GPU: the ABI is declared, bound and exported, the kernel uses no scratch
memory, every refusal comes before the library is touched, the NumPy restatement the GPU tests compare against
(tests/helpers/decay_oracle.py) recovers the decay time of its own input family, and the host-only pieces (the closed forms of the
fit's abscissa sums, the truncation horizon, the estimates from the device's five values) agree with brute force."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

import decay_oracle as do  # noqa: E402

HEADER = os.path.join(os.path.dirname(HERE), "include", "overiva_hip.h")
SYMBOLS = ("oiva_decay_create", "oiva_decay_destroy", "oiva_decay_set_host", "oiva_decay_set_dev", "oiva_decay_set_room",
           "oiva_decay_run", "oiva_decay_get", "oiva_decay_get_curve", "oiva_decay_ms", "oiva_decay_room_set_absorption")
FS = 8000


@pytest.fixture(scope="module")
def lib():
    from overiva_amd import _lib, build

    build.build_library()
    return _lib.load()


def test_symbols_declared_bound_and_exported(lib):
    import overiva_amd
    from overiva_amd import _lib, acoustics, build, room

    header = open(HEADER).read()
    for sym in SYMBOLS:
        assert re.search(r"oiva_status\s+%s\s*\(" % sym, header), sym
        assert sym in _lib.SIGNATURES, sym
        assert hasattr(lib, sym), sym
    assert {s for s in _lib.SIGNATURES if s.startswith("oiva_decay_")} == set(SYMBOLS)
    assert "kernels_decay.hip" in build.SOURCES and "decay.hip" in build.SOURCES
    for name in ("measure_rt60_batch", "edc_batch", "DecayBatch", "absorption_for_rt60", "truncation_horizon"):
        assert name in overiva_amd.__all__ and getattr(overiva_amd, name) is getattr(acoustics, name)
    assert issubclass(acoustics.DecayBatch, _lib.Handle)
    for method in ("measure_rt60", "set_absorption"):
        assert callable(getattr(room.RoomBatch, method))
    assert "not pinned" in " ".join(acoustics.__doc__.split()) and "not pinned" in " ".join(acoustics.measure_rt60_batch.__doc__.split())
    assert "kDecayTile = %d;" % acoustics.TILE in open(os.path.join(build.CSRC, "oiva_internal.h")).read()


def test_decay_kernel_uses_no_scratch_memory():
    from overiva_amd import build

    build.build_library()
    usage = build.kernel_usage(("kernels_decay",))
    assert len(usage) == 1 and "decay_kernel" in next(iter(usage)), sorted(usage)
    assert next(iter(usage.values()))["scratch"] == 0, usage


def test_library_checks_its_arguments_before_the_device(lib):
    from overiva_amd import _lib
    from conftest import has_gpu

    def create(lengths, out=True):
        h = C.c_void_p()
        table = (C.c_int * len(lengths))(*lengths) if lengths is not None else None
        return lib.oiva_decay_create(C.byref(h) if out else None, 0, len(lengths or [1]), table, None)

    for kw in (dict(lengths=[10], out=False), dict(lengths=None), dict(lengths=[]), dict(lengths=[10, 0]), dict(lengths=[(1 << 24) + 1])):
        assert create(**kw) == _lib.ERR_ARG, kw
    assert "response 1 must hold 1..2^24 samples" in (create([10, 0]), lib.oiva_last_error().decode())[1]
    for fn, args in (("oiva_decay_set_host", (None, None)), ("oiva_decay_set_dev", (None, None)), ("oiva_decay_set_room", (None, None)),
                     ("oiva_decay_run", (None, 8000.0, 5.0, 20.0, 0)), ("oiva_decay_get", (None,) * 6),
                     ("oiva_decay_get_curve", (None, None)), ("oiva_decay_ms", (None, None)),
                     ("oiva_decay_room_set_absorption", (None, None))):
        assert getattr(lib, fn)(*args) == _lib.ERR_ARG, fn
    assert lib.oiva_decay_destroy(None) == _lib.OK
    if not has_gpu():      # the control: a table in order reaches the device, which is not there
        assert create([10, 1 << 24]) == _lib.ERR_HIP


# ---- the restatement on its own family --------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [4097, 9000])
@pytest.mark.parametrize("rt", [0.05, 0.12, 0.3])
def test_restatement_recovers_the_decay_time(L, rt):
    """within 10 %: 8 % was measured with a restatement of the algorithm on this family, the rest is margin for another draw order"""
    r = do.measure(do.family(L, rt, FS), FS)
    print(f"L={L} rt={rt}: cross {r['rt60_cross']:.5f} fit {r['rt60_fit']:.5f} window {r['window']} margin {r['margin']:.2e}")
    assert abs(r["rt60_cross"] - rt) <= 0.1 * rt and abs(r["rt60_fit"] - rt) <= 0.1 * rt
    assert r["window"] == r["i_b"] - r["i_a"]          # E does not increase: the masked window is [i_a, i_b)
    assert r["margin"] >= 1e-9


def test_restatement_float64_against_longdouble():
    for L in (63, 257, 1025, 4097, 9000):
        for rt in (0.05, 0.12, 0.3):
            h = do.family(L, rt, FS)
            a, b = do.measure(h, FS), do.measure(h, FS, dtype=np.longdouble)
            assert (a["i_a"], a["i_b"]) == (b["i_a"], b["i_b"])
            pos = b["E"] > 0
            assert np.max(np.abs(a["E"][pos] - b["E"][pos]) / b["E"][pos]) <= 1e-12
            assert np.isnan(a["rt60_fit"]) == np.isnan(b["rt60_fit"])
            if not np.isnan(a["rt60_fit"]):
                assert abs(a["rt60_fit"] - b["rt60_fit"]) <= 1e-12 * abs(b["rt60_fit"])


def test_a_response_that_ends_before_the_lower_threshold_is_nan():
    """E[L - 1] is the last sample's square: the curve of a response stays above -25 dB only when its last sample holds more than
    10^-2.5 of the energy -- a response that grows, or a very short one"""
    for h in (np.arange(1.0, 41.0) ** 2, np.ones(40), np.ones(1), np.array([1.0, 0.5])):
        r = do.measure(h, FS)
        assert r["i_b"] == -1 and np.isnan(r["rt60_cross"]) and np.isnan(r["rt60_fit"]), h.shape
    assert do.measure(np.ones(40), FS)["i_a"] == 28          # E[n] = 40 - n <= 40 * 10^-0.5 = 12.65 from n = 28 on
    z = do.measure(np.zeros(100), FS)
    assert (z["i_a"], z["i_b"]) == (-1, -1) and np.isnan(z["rt60_cross"]) and np.isnan(z["rt60_fit"])


# ---- host-only pieces ---------------------------------------------------------------------------------------------------------
def test_closed_forms_of_the_abscissa_sums():
    from overiva_amd import acoustics

    for i_a, i_b in ((0, 1), (0, 2), (3, 10), (17, 18), (1000, 4097), (0, 1 << 24), ((1 << 24) - 5, 1 << 24)):
        N, s1, s2 = acoustics.window_sums(i_a, i_b)
        if i_b - i_a <= 5000:
            n = range(i_a, i_b)
            assert (N, s1, s2) == (len(n), sum(n), sum(k * k for k in n)), (i_a, i_b)
        assert N == i_b - i_a and 2 * s1 == N * (i_a + i_b - 1)
        assert 12 * (N * s2 - s1 * s1) == N * N * (N * N - 1)          # Sxx = N (N^2 - 1) / 12, what estimates() divides by


def test_estimates_from_the_five_values():
    from overiva_amd import acoustics

    rows = []
    for L, rt in ((4097, 0.05), (9000, 0.3), (255, 0.3), (1025, 0.12)):
        r = do.measure(do.family(L, rt, FS), FS)
        rows.append(r)
    rows += [do.measure(np.zeros(10), FS), do.measure(np.ones(40), FS)]
    cross, fit = acoustics.estimates(FS, 20.0, *[[float(r[k]) if k[0] != "i" else r[k] for r in rows]
                                                for k in ("e0", "i_a", "i_b", "sum_d", "sum_nd")])
    for r, c, f in zip(rows, cross, fit):
        assert np.isnan(c) == np.isnan(r["rt60_cross"]) and np.isnan(f) == np.isnan(r["rt60_fit"])
        if not np.isnan(f):
            assert c == r["rt60_cross"] and abs(f - r["rt60_fit"]) <= 1e-14 * f
    # a window of one sample has no slope
    c, f = acoustics.estimates(FS, 20.0, [1.0], [5], [6], [-7.0], [-35.0])
    assert c[0] == 3.0 / FS and np.isnan(f[0])


def test_truncation_horizon():
    from overiva_amd import acoustics

    want = 15 / (343 * np.sqrt(1 / 100 + 1 / 56.25 + 1 / 9))
    assert acoustics.truncation_horizon([10, 7.5, 3], 17) == pytest.approx(want, rel=1e-15)
    both = acoustics.truncation_horizon([[10, 7.5, 3], [5, 4, 3]], 17, c=340.0)
    assert both.shape == (2,) and both[0] == pytest.approx(want * 343 / 340, rel=1e-14)
    assert acoustics.truncation_horizon([10, 7.5, 3], 0) == 0 and acoustics.truncation_horizon([10, 7.5, 3], 1) == 0
    assert acoustics.truncation_horizon([10, 7.5, 3], 2) == 0
    for bad in (dict(room_dim=[10, 7.5]), dict(room_dim=[10, 7.5, 0]), dict(max_order=-1), dict(max_order=1.5), dict(c=0)):
        with pytest.raises(ValueError):
            acoustics.truncation_horizon(**dict(dict(room_dim=[10, 7.5, 3], max_order=17), **bad))


# ---- refusals, all before the library is touched -------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """any use of the library fails the test: validation must come first"""
    from overiva_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was touched before the arguments were validated")

    monkeypatch.setattr(_lib, "load", boom)
    import overiva_amd

    return overiva_amd


H = do.family(300, 0.05, FS)
BAD_MEASURE = {
    "empty list": dict(rirs=[]),
    "empty array": dict(rirs=np.zeros((3, 0))),
    "no samples": dict(rirs=np.zeros((0, 10))),
    "scalar": dict(rirs=np.float64(1.0)),
    "complex": dict(rirs=H + 0j),
    "nan": dict(rirs=np.where(np.arange(300) == 7, np.nan, H)),
    "inf in a list": dict(rirs=[H, np.where(np.arange(300) == 7, np.inf, H)]),
    "fs zero": dict(fs=0),
    "fs negative": dict(fs=-8000),
    "fs nan": dict(fs=np.nan),
    "decay_db zero": dict(decay_db=0),
    "decay_db negative": dict(decay_db=-20),
    "start_db negative": dict(start_db=-1),
    "too long": dict(rirs=np.broadcast_to(np.float32(1), ((1 << 24) + 1,))),
}


@pytest.mark.parametrize("bad", sorted(BAD_MEASURE))
def test_measure_validation_before_device(no_device, bad):
    with pytest.raises(ValueError):
        no_device.measure_rt60_batch(**dict(dict(rirs=H, fs=FS), **BAD_MEASURE[bad]))


def test_the_refusals_name_the_argument(no_device):
    for kw, name in ((dict(fs=0), "fs"), (dict(decay_db=0), "decay_db"), (dict(start_db=-1), "start_db"), (dict(rirs=H + 0j), "rirs"),
                     (dict(rirs=[H, H * np.nan]), r"rirs\[1\]")):
        with pytest.raises(ValueError, match=name):
            no_device.measure_rt60_batch(**dict(dict(rirs=H, fs=FS), **kw))
    with pytest.raises(ValueError, match="rirs"):
        no_device.edc_batch([])
    with pytest.raises(ValueError, match=r"lengths\[1\]"):
        no_device.DecayBatch([10, (1 << 24) + 1])


def _rooms(B=2):
    dim = np.array([[5.0, 4.0, 3.0], [6.0, 5.0, 2.5], [4.0, 3.5, 2.8]])[:B]
    src = np.array([[[1.0, 1.0, 1.0], [3.5, 2.0, 1.5]]] * B)
    mic = np.array([[[2.0, 3.0, 1.2], [2.2, 3.0, 1.2]]] * B)
    return dict(room_dim=dim, sources=src, mics=mic, rt60=0.2, max_order=8, fs=FS, rir_length=2000)


BAD_SEARCH = {
    "rtol zero": dict(rtol=0),
    "rtol negative": dict(rtol=-0.01),
    "bracket low": dict(bracket=(0.0, 0.9)),
    "bracket high": dict(bracket=(0.1, 1.0)),
    "bracket reversed": dict(bracket=(0.9, 0.1)),
    "bracket equal": dict(bracket=(0.5, 0.5)),
    "bracket scalar": dict(bracket=0.5),
    "rt60 zero": dict(rt60=0.0),
    "rt60 negative": dict(rt60=[0.2, -0.1]),
    "rt60 shape": dict(rt60=[0.2, 0.3, 0.4]),
    "rt60 nan": dict(rt60=np.nan),
    "estimator": dict(estimator="edt"),
    "max_steps": dict(max_steps=1),
    "decay_db": dict(decay_db=0),
    "start_db": dict(start_db=-5),
    "fs": dict(fs=0),
    "geometry": dict(room_dim=np.ones((2, 2))),
    "max_order": dict(max_order=33),
}


@pytest.mark.parametrize("bad", sorted(BAD_SEARCH))
def test_search_validation_before_device(no_device, bad):
    with pytest.raises(ValueError):
        no_device.absorption_for_rt60(**dict(_rooms(), **BAD_SEARCH[bad]))


def test_refused_under_bin_sharding(no_device, monkeypatch):
    from overiva_amd import sharded

    monkeypatch.setattr(sharded, "active_group", lambda: object())
    for call in (lambda: no_device.measure_rt60_batch(H, FS), lambda: no_device.edc_batch(H),
                 lambda: no_device.absorption_for_rt60(**_rooms())):
        with pytest.raises(ValueError, match="does not run under enable_bin_sharding"):
            call()


@pytest.mark.parametrize("call", ["measure", "measure list", "measure int", "edc", "search", "search per room", "handle"])
def test_good_arguments_reach_the_library(no_device, call):
    """the control of the refusals: arguments that are in order pass every check and go on to the library"""
    with pytest.raises(AssertionError, match="the library was touched"):
        if call == "measure":
            no_device.measure_rt60_batch(np.stack([H, H]).reshape(1, 2, 300), FS, decay_db=30, start_db=0, return_curves=True)
        elif call == "measure list":
            no_device.measure_rt60_batch([H, H[:1], np.stack([H[:17]] * 3)], 16000.0, return_indices=True)
        elif call == "measure int":
            no_device.measure_rt60_batch(np.arange(10, 0, -1), 1)
        elif call == "edc":
            no_device.edc_batch(H.astype(np.float32))
        elif call == "search":
            no_device.absorption_for_rt60(**_rooms())
        elif call == "search per room":
            no_device.absorption_for_rt60(**dict(_rooms(3), rt60=[0.2, 0.3, 0.25], estimator="cross", bracket=(0.05, 0.9), max_steps=2))
        else:
            no_device.DecayBatch([1, 1 << 24])


# ---- the inputs of the GPU tests are admissible ---------------------------------------------------------------------------------
def test_gpu_inputs_keep_their_distance_from_the_thresholds():
    """the condition under which the device's integers must equal the restatement's: no crossing within 1e-9 of its threshold;
    multi-tile responses lie on both load paths; every long input has a window of at least 32 samples"""
    import decay_cases as dc
    from overiva_amd import acoustics

    assert dc.TILE == acoustics.TILE
    items = dc.curve_inputs()
    margins = [do.measure(h, dc.FS, dtype=np.longdouble)["margin"] for h in items + dc.long_inputs()]
    print("smallest margin", min(margins))
    assert min(margins) >= 1e-9
    off = dc.offsets(items)
    assert {int(o) % 2 for o, h in zip(off, items) if len(h) > dc.TILE} == {0, 1}
    assert all(do.measure(h, dc.FS)["window"] >= 32 for h in dc.long_inputs())


def test_search_rooms_are_finite_and_bracketed_on_the_cpu():
    """with room_oracle: at the absorption that defines the targets every pair's estimate is finite, and each room's target lies
    between the values at the two ends of the bracket the GPU test passes"""
    import decay_cases as dc
    import room_oracle as ro

    g = dc.SEARCH_ROOMS
    for b in range(3):
        val = {}
        for a in (dc.SEARCH_ABSORPTION,) + dc.SEARCH_BRACKET:
            h, _ = ro.rir(g["room_dim"][b], g["sources"][b], g["mics"][b], absorption=a, fs=g["fs"], max_order=g["max_order"],
                          rir_length=g["rir_length"])
            val[a], finite = dc.room_median(h)
            assert finite, (b, a)
        lo, hi = sorted(val[a] for a in dc.SEARCH_BRACKET)
        print(f"room {b}: target {val[dc.SEARCH_ABSORPTION]:.5f} between {lo:.5f} and {hi:.5f}")
        assert lo < val[dc.SEARCH_ABSORPTION] < hi
