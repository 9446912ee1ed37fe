"""The seeded normal stream without a GPU: the NumPy restatement (tests/helpers/rng_oracle.py) gives numpy.random.Philox's raw
words, the ABI is declared, bound and exported, the kernels use no scratch memory, and every refusal comes before the library is
touched (in Python) or before a device call (in the library: without a GPU any device call gives ERR_HIP, so ERR_ARG shows the
order)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

import rng_oracle as rng_o  # noqa: E402

HEADER = os.path.join(os.path.dirname(HERE), "include", "overiva_hip.h")
SYMBOLS = ("oiva_rng_create", "oiva_rng_destroy", "oiva_rng_fill", "oiva_rng_fill_ms", "oiva_rng_get", "oiva_rng_ptr", "oiva_rng_raw",
           "oiva_rng_room_mix")
KERNELS = ("rng_normal_kernel", "rng_raw_kernel")
ALL_ONES = rng_o.ALL_ONES


@pytest.mark.parametrize("key,purpose,j", rng_o.RAW_CASES)
def test_the_restatement_gives_numpys_raw_words(key, purpose, j):
    got = rng_o.raw_blocks(key, purpose, j, 1)[0]
    want = rng_o.numpy_philox_block(key, purpose, j)
    assert got.dtype == np.uint64 and np.array_equal(got, want), (got, want)


def test_the_restatement_over_a_run_of_blocks():
    """a run of blocks that crosses 2^32, against one numpy generator advanced block by block"""
    first, n = 2 ** 32 - 3, 8
    got = rng_o.raw_blocks((123, 0), 1, first, n)
    counter = np.array([first - 1, 1, 0, 0], dtype=np.uint64)
    want = np.random.Philox(key=np.array([123, 0], dtype=np.uint64), counter=counter).random_raw(4 * n).reshape(n, 4)
    assert np.array_equal(got, want)


def test_the_restatement_maps_words_into_the_open_interval():
    u = rng_o.unit_open(np.array([0, ALL_ONES, 1 << 12], dtype=np.uint64))
    assert u[0] == 2.0 ** -53 and u[1] == 1.0 - 2.0 ** -53 and u[2] == 1.5 * 2.0 ** -52
    assert np.sqrt(-2.0 * np.log(u[0])) < 8.58
    z = rng_o.standard_normal(11, (123, 0))
    assert z.shape == (11,) and np.array_equal(z, rng_o.standard_normal(64, (123, 0))[:11])


def test_the_restatement_passes_the_statistics_the_device_is_held_to():
    """2^20 draws of the three streams of tests/test_rng_gpu.py: the stream itself, not an implementation of it, meets the bounds"""
    n = 1 << 20
    a, b, c = rng_o.standard_normal(n, (123, 0), 0), rng_o.standard_normal(n, (123, 0), 1), rng_o.standard_normal(n, (123, 1), 0)
    assert np.max(np.abs(np.concatenate([a, b, c]))) <= 8.58
    for name, z, others in (("key (123, 0) purpose 0", a, (c, b)), ("key (123, 0) purpose 1", b, (c, a)),
                            ("key (123, 1) purpose 0", c, (a, b))):
        for stat, (value, bound) in rng_o.statistics(z, *others).items():
            print(f"{name}: {stat} {value:.3e} (bound {bound:.3e})")
            assert value < bound, (name, stat, value, bound)


@pytest.fixture(scope="module")
def lib():
    from overiva_amd import _lib, build

    build.build_library()
    return _lib.load()


def test_symbols_declared_bound_and_exported(lib):
    import overiva_amd
    from overiva_amd import _lib, build, rng, room, sweep

    header = open(HEADER).read()
    for sym in SYMBOLS:
        assert re.search(r"oiva_status\s+%s\s*\(" % sym, header), sym
        assert sym in _lib.SIGNATURES, sym
        assert hasattr(lib, sym), sym
    assert {s for s in _lib.SIGNATURES if s.startswith("oiva_rng_")} == set(SYMBOLS)
    assert "kernels_rng.hip" in build.SOURCES and "rng.hip" in build.SOURCES
    for name in ("standard_normal_batch", "DeviceNormal"):
        assert name in overiva_amd.__all__ and getattr(overiva_amd, name) is getattr(rng, name)
    assert issubclass(rng.DeviceNormal, _lib.Handle) and callable(rng.raw_blocks)
    for doc in (sweep.__doc__, sweep.sweep_batch.__doc__):
        assert "What still crosses the bus" in doc and "seeds" in doc
    for doc in (room.__doc__, room.simulate_batch.__doc__, room.rir_batch.__doc__):
        assert "not pinned" in doc
    for doc in (room.simulate_batch.__doc__, sweep.sweep_batch.__doc__):
        assert "depend" in doc and "index in the batch" in doc


def test_rng_kernels_use_no_scratch_memory():
    from overiva_amd import build

    build.build_library()
    usage = build.kernel_usage(("kernels_rng",))
    for kernel in KERNELS:
        hit = [u for name, u in usage.items() if kernel in name]
        assert len(hit) == 1, (kernel, sorted(usage))
        assert hit[0]["scratch"] == 0, (kernel, hit[0])
    assert all(any(k in name for k in KERNELS) for name in usage), sorted(usage)


# ---- the library: arguments before any device call ----------------------------------------------------------------------------
def test_null_handles_and_pointers(lib):
    from overiva_amd import _lib

    x = np.zeros(4)
    k = np.zeros(4, dtype=np.uint64)
    p, kp, out = _lib.ptr(x), _lib.ptr(k), C.c_void_p()
    one = C.c_void_p(8)           # a handle that is not null: never followed, a null argument is met first
    counts = (C.c_longlong * 2)(5, 3)
    assert lib.oiva_rng_destroy(None) == _lib.OK
    assert lib.oiva_rng_create(None, 0, 2, counts, None) == _lib.ERR_ARG
    assert lib.oiva_rng_create(C.byref(out), 0, 2, None, None) == _lib.ERR_ARG
    assert lib.oiva_rng_fill(None, kp, kp, 0) == lib.oiva_rng_fill(one, None, kp, 0) == lib.oiva_rng_fill(one, kp, None, 0) == _lib.ERR_ARG
    assert lib.oiva_rng_fill_ms(None, (C.c_float * 1)()) == lib.oiva_rng_fill_ms(one, None) == _lib.ERR_ARG
    assert lib.oiva_rng_get(None, p) == lib.oiva_rng_get(one, None) == _lib.ERR_ARG
    assert lib.oiva_rng_ptr(None, C.byref(out)) == lib.oiva_rng_ptr(one, None) == _lib.ERR_ARG
    assert lib.oiva_rng_raw(0, 1, 2, 0, 0, 1, None) == _lib.ERR_ARG
    assert lib.oiva_rng_room_mix(None, 0, 1, 10.0, 60.0, 0, None, kp, kp) == _lib.ERR_ARG
    assert lib.oiva_rng_room_mix(one, 0, 1, 10.0, 60.0, 0, None, None, kp) == _lib.ERR_ARG
    assert lib.oiva_rng_room_mix(one, 0, 1, 10.0, 60.0, 0, None, kp, None) == _lib.ERR_ARG


def test_create_and_raw_check_their_arguments_before_the_device(lib):
    from overiva_amd import _lib
    from conftest import has_gpu

    h = C.c_void_p()
    for counts in ((5, 0), (5, -1), (5, (1 << 40) + 1), (1 << 40, 1)):
        assert lib.oiva_rng_create(C.byref(h), 0, 2, (C.c_longlong * 2)(*counts), None) == _lib.ERR_ARG, counts
    assert lib.oiva_rng_create(C.byref(h), 0, 0, (C.c_longlong * 2)(5, 3), None) == _lib.ERR_ARG
    assert lib.oiva_rng_create(C.byref(h), 0, 65536, (C.c_longlong * 2)(5, 3), None) == _lib.ERR_ARG
    words = np.zeros((4, 4), dtype=np.uint64)
    for n in (0, -1, (1 << 20) + 1):
        assert lib.oiva_rng_raw(0, 1, 2, 0, 0, n, _lib.ptr(words)) == _lib.ERR_ARG, n
    if not has_gpu():      # the control: arguments in order reach the device, which is not there
        assert lib.oiva_rng_create(C.byref(h), 0, 2, (C.c_longlong * 2)(5, 3), None) == _lib.ERR_HIP
        assert lib.oiva_rng_raw(0, 1, 2, 0, 0, 4, _lib.ptr(words)) == _lib.ERR_HIP


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


def _scene(B=2, S=4, M=3, n=900):
    rng = np.random.default_rng(0)
    dim = np.tile([4.0, 5.0, 3.0], (B, 1))
    return dict(signals=rng.standard_normal((B, S, n)), room_dim=dim, sources=dim[:, None, :] * rng.uniform(0.15, 0.85, (B, S, 3)),
                mics=dim[:, None, :] * rng.uniform(0.15, 0.85, (B, M, 3)), n_targets=2, fs=8000, max_order=2, rir_length=200)


def _sweep_scene():
    return dict(_scene(), frame=64, hop=32, filter_length=16)


# for a batch of two streams or rooms
BAD_SEEDS = {"bool": True, "float": 3.0, "numpy float": np.float64(3.0), "negative": -1, "2^64": 1 << 64, "too few": [1], "too many": [1, 2, 3],
             "not 1-D": [[1, 2]], "array not 1-D": np.zeros((2, 1), dtype=np.int64), "0-d array": np.array(3), "bool in sequence": [1, True],
             "float in sequence": [1, 2.0], "float array": np.array([1.0, 2.0]), "bool array": np.array([True, False]),
             "negative in sequence": [1, -2], "2^64 in sequence": [1, 1 << 64], "string": "12"}
GOOD_SEEDS = {"int": 5, "zero": 0, "largest": ALL_ONES, "numpy int": np.int64(7), "list": [3, ALL_ONES], "tuple": (0, 0),
              "array": np.array([4, 5], dtype=np.uint64)}


@pytest.mark.parametrize("bad", sorted(BAD_SEEDS))
def test_bad_seeds_are_refused_before_the_library(no_device, bad):
    seed = BAD_SEEDS[bad]
    with pytest.raises(ValueError):
        no_device.standard_normal_batch([5, 3], seed)
    with pytest.raises(ValueError):
        no_device.simulate_batch(**_scene(), seed=seed)
    with pytest.raises(ValueError):
        no_device.sweep_batch(**_sweep_scene(), seed=seed)


@pytest.mark.parametrize("good", sorted(GOOD_SEEDS))
def test_good_seeds_reach_the_library(no_device, good):
    seed = GOOD_SEEDS[good]
    for call in (lambda: no_device.standard_normal_batch([5, 3], seed), lambda: no_device.simulate_batch(**_scene(), seed=seed),
                 lambda: no_device.sweep_batch(**_sweep_scene(), seed=seed),
                 lambda: no_device.sweep_batch(**_sweep_scene(), seed=seed, filler=np.zeros((2, 1200))),
                 lambda: no_device.sweep_batch(**_sweep_scene(), seed=seed, noise=np.zeros((2, 1099, 3)))):
        with pytest.raises(AssertionError, match="the library was touched"):
            call()


def test_seed_with_the_callers_arrays(no_device):
    with pytest.raises(ValueError, match="seed and noise"):
        no_device.simulate_batch(**_scene(), seed=5, noise=np.zeros((2, 1099, 3)))
    with pytest.raises(ValueError, match="needs n_targets"):
        no_device.simulate_batch(**dict(_scene(), n_targets=None), seed=5)
    with pytest.raises(ValueError, match="nothing is left to draw"):
        no_device.sweep_batch(**_sweep_scene(), seed=5, noise=np.zeros((2, 1099, 3)), filler=np.zeros((2, 1200)))
    with pytest.raises(ValueError, match="max_group"):
        no_device.simulate_batch(**_scene(), seed=5, max_group=-1)


@pytest.mark.parametrize("sizes", [5, [], [5, 0], [5, -1], [5, 2.0], [5, True], [[5, 3]], [(1 << 40) + 1], [1 << 40, 1], "53", None],
                         ids=repr)
def test_bad_sizes_are_refused_before_the_library(no_device, sizes):
    with pytest.raises(ValueError):
        no_device.standard_normal_batch(sizes, 0)
    with pytest.raises(ValueError):
        no_device.DeviceNormal(sizes)


def test_bad_purposes_and_raw_arguments_are_refused_before_the_library(no_device):
    from overiva_amd import rng

    for purpose in (-1, 1 << 64, 1.0, True, None):
        with pytest.raises(ValueError):
            no_device.standard_normal_batch([5], 0, purpose=purpose)
    for args in (((1,), 0, 0, 1), ((1, -2), 0, 0, 1), ((1, 2), -1, 0, 1), ((1, 2), 0, 1 << 64, 1), ((1, 2), 0, 0, 0),
                 ((1, 2), 0, 0, (1 << 20) + 1), ((1, 2), 0, 0, 2.0)):
        with pytest.raises(ValueError):
            rng.raw_blocks(*args)
    with pytest.raises(AssertionError, match="the library was touched"):
        rng.raw_blocks((1, 2), 0, 0, 4)


def test_keys_of_the_two_seed_forms():
    """an int s: room b has the key (s, b); a sequence: room b has the key (seed[b], 0)"""
    from overiva_amd.rng import check_seed

    k0, k1 = check_seed(9, 3)
    assert k0.dtype == k1.dtype == np.uint64 and k0.tolist() == [9, 9, 9] and k1.tolist() == [0, 1, 2]
    k0, k1 = check_seed([ALL_ONES, 0, 4], 3)
    assert k0.dtype == k1.dtype == np.uint64 and k0.tolist() == [ALL_ONES, 0, 4] and k1.tolist() == [0, 0, 0]
