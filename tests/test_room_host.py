"""rir_batch() / simulate_batch() without a GPU: the ABI is declared, bound and exported, every refusal comes before the library is
touched, the NumPy restatement the GPU tests compare against (tests/helpers/room_oracle.py) agrees with closed forms, and every
case of tests/helpers/room_cases.py is admissible (no image delay within 1e-6 samples of a rounding tie)."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

import room_cases as cases  # noqa: E402
import room_oracle as ro  # noqa: E402

HEADER = os.path.join(os.path.dirname(HERE), "include", "overiva_hip.h")
SYMBOLS = ("oiva_room_create", "oiva_room_destroy", "oiva_room_compute_rir", "oiva_room_rir_lengths", "oiva_room_get_rir",
           "oiva_room_set_signals", "oiva_room_groups", "oiva_room_convolve", "oiva_room_get_premix", "oiva_room_mix",
           "oiva_room_get_mix", "oiva_room_time_stages")
KERNELS = ("room_kmax_kernel", "room_rir_kernel", "room_pad_kernel", "room_product_kernel", "room_unpack_kernel", "room_std_kernel",
           "room_mix_kernel")


def test_symbols_declared_bound_and_exported():
    import overiva_amd
    from overiva_amd import _lib, build, room

    header = open(HEADER).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in _lib.SIGNATURES, sym
    assert {s for s in _lib.SIGNATURES if s.startswith("oiva_room_")} == set(SYMBOLS)
    assert "kernels_room.hip" in build.SOURCES and "room.hip" in build.SOURCES
    for name in ("rir_batch", "simulate_batch", "RoomBatch"):
        assert name in overiva_amd.__all__ and getattr(overiva_amd, name) is getattr(room, name)
    assert issubclass(room.RoomBatch, _lib.Handle)
    for doc in (room.__doc__, room.rir_batch.__doc__, room.simulate_batch.__doc__):
        assert "not pinned" in " ".join(doc.split())
    for method in ("compute_rir", "get_rir", "set_signals", "convolve", "get_premix", "mix", "get_mix", "simulate", "time_stages"):
        assert callable(getattr(room.RoomBatch, method))
    build.build_library()
    lib = _lib.load()
    for sym in SYMBOLS:
        assert hasattr(lib, sym), sym


def test_room_kernels_use_no_scratch_memory():
    from overiva_amd import build

    build.build_library()
    usage = build.kernel_usage(("kernels_room",))
    for kernel in KERNELS:
        hit = [u for name, u in usage.items() if kernel in name]
        assert len(hit) == 1, (kernel, sorted(usage))
        assert hit[0]["scratch"] == 0, (kernel, hit[0])
    assert all(any(k in name for k in KERNELS) for name in usage), sorted(usage)


# ---- refusals, all before a device call ----------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """any use of the library fails the test: validation must come first"""
    from overiva_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the library was touched before the arguments were validated")

    monkeypatch.setattr(_lib, "load", boom)
    import overiva_amd

    return overiva_amd


def _good(B=2, S=3, M=2, n=50):
    rng = np.random.default_rng(0)
    dim = np.tile([4.0, 5.0, 3.0], (B, 1))
    return dict(signals=rng.standard_normal((B, S, n)), room_dim=dim, sources=dim[:, None, :] * rng.uniform(0.15, 0.85, (B, S, 3)),
                mics=dim[:, None, :] * rng.uniform(0.15, 0.85, (B, M, 3)), fs=8000, max_order=2)


def _at(a, index, value):
    a = np.array(a, dtype=float)
    a[index] = value
    return a


G = _good()
BAD = {
    "room_dim rank": dict(room_dim=G["room_dim"][0]),
    "room_dim of two": dict(room_dim=G["room_dim"][:, :2]),
    "sources rank": dict(sources=G["sources"][0]),
    "mics rank": dict(mics=G["mics"][:, :, None]),
    "batch of sources": dict(sources=G["sources"][:1]),
    "batch of mics": dict(mics=np.concatenate([G["mics"], G["mics"]])),
    "batch of signals": dict(signals=G["signals"][:1]),
    "sources of signals": dict(signals=G["signals"][:, :2]),
    "signals rank": dict(signals=G["signals"][0]),
    "a room of rank 1": dict(signals=[G["signals"][0], G["signals"][1][0]]),
    "no samples": dict(signals=G["signals"][:, :, :0]),
    "source on a wall": dict(sources=_at(G["sources"], (1, 0, 2), 0.0)),
    "source on the far wall": dict(sources=_at(G["sources"], (0, 1, 0), 4.0)),
    "source outside": dict(sources=_at(G["sources"], (0, 2, 1), 5.5)),
    "mic outside": dict(mics=_at(G["mics"], (1, 1, 0), -0.1)),
    "mic on a wall": dict(mics=_at(G["mics"], (0, 0, 2), 3.0)),
    "source on a microphone": dict(mics=_at(G["mics"], (1, 1), G["sources"][1, 2])),
    "absorption 1": dict(absorption=1.0),
    "absorption negative": dict(absorption=-0.01),
    "absorption of one wall": dict(absorption=_at(np.full((2, 6), 0.3), (1, 4), 1.2)),
    "absorption shape": dict(absorption=np.full((2, 3), 0.3)),
    "fs zero": dict(fs=0),
    "fs negative": dict(fs=-8000.0),
    "c zero": dict(c=0.0),
    "c nan": dict(c=float("nan")),
    "order negative": dict(max_order=-1),
    "order 33": dict(max_order=33),
    "order 2.0": dict(max_order=2.0),
    "17 sources": dict(signals=np.ones((2, 17, 5)), sources=np.tile(G["sources"][:, :1], (1, 17, 1)) * np.linspace(0.5, 1, 17)[None, :, None]),
    "no source": dict(signals=np.ones((2, 0, 5)), sources=G["sources"][:, :0]),
    "33 mics": dict(mics=np.tile(G["mics"][:, :1], (1, 33, 1)) * np.linspace(0.5, 1, 33)[None, :, None]),
    "no mic": dict(mics=G["mics"][:, :0]),
    "nan signal": dict(signals=_at(G["signals"], (1, 0, 7), np.nan)),
    "inf signal": dict(signals=_at(G["signals"], (0, 2, 3), np.inf)),
    "complex signals": dict(signals=G["signals"] + 0j),
    "rir_length zero": dict(rir_length=0),
    "rir_length too long": dict(rir_length=65537),
    "n_targets zero": dict(n_targets=0),
    "n_targets above S": dict(n_targets=4),
    "n_targets 1.5": dict(n_targets=1.5),
    "all targets, finite sinr": dict(n_targets=3, sinr=10.0),
    "ref_mic": dict(n_targets=1, ref_mic=2),
    "sources_var": dict(n_targets=2, sources_var=[1.0]),
    "noise rank": dict(n_targets=1, noise=np.zeros((2, 60))),
    "noise mics": dict(n_targets=1, noise=np.zeros((2, 60, 3))),
    "noise batch": dict(n_targets=1, noise=np.zeros((1, 60, 2))),
    "noise as a list": dict(n_targets=1, noise=[np.zeros((60, 2))] * 2),
}


@pytest.mark.parametrize("bad", sorted(BAD))
def test_validation_before_device(no_device, bad):
    args = dict(_good(), **BAD[bad])
    with pytest.raises(ValueError):
        no_device.simulate_batch(**args)
    if not set(BAD[bad]) & {"signals", "n_targets", "sinr", "ref_mic", "sources_var", "noise"}:
        args.pop("signals")
        with pytest.raises(ValueError):
            no_device.rir_batch(**args)


@pytest.mark.parametrize("extra", [dict(), dict(absorption=np.full(2, 0.2)), dict(absorption=np.full((2, 6), 0.2), rir_length=65536),
                                   dict(n_targets=2, noise=np.zeros((2, 60, 2))), dict(n_targets=3, sinr=np.inf, sources_var=[1, 2, 3]),
                                   dict(signals=list(_good()["signals"]), n_targets=1, noise=[np.zeros((60, 2))] * 2)])
def test_good_arguments_reach_the_library(no_device, extra):
    """the control of the refusals: arguments that are in order pass every check and go on to the library"""
    args = dict(_good(), **extra)
    with pytest.raises(AssertionError, match="the library was touched"):
        no_device.simulate_batch(**args)
    if not set(extra) & {"signals", "n_targets"}:
        args.pop("signals")
        with pytest.raises(AssertionError, match="the library was touched"):
            no_device.rir_batch(**args)


def test_refused_under_bin_sharding(no_device, monkeypatch):
    from overiva_amd import sharded

    monkeypatch.setattr(sharded, "active_group", lambda: object())
    args = _good()
    with pytest.raises(ValueError, match="does not run under enable_bin_sharding"):
        no_device.simulate_batch(**args)
    args.pop("signals")
    with pytest.raises(ValueError, match="does not run under enable_bin_sharding"):
        no_device.rir_batch(**args)


# ---- the restatement against closed forms ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [0, 1, 2, 3, 4, 5, 6, 17])
def test_image_count_and_order(N):
    from overiva_amd.room import image_count

    img = ro.images(N)
    assert len(img) == (2 * N + 1) * (2 * N * N + 2 * N + 3) // 3 == ro.image_count(N) == image_count(N)
    assert {0: 1, 1: 7, 3: 63, 4: 129, 6: 377, 17: 7175}.get(N, len(img)) == len(img)
    assert np.all(np.abs(img).sum(axis=1) <= N) and len({tuple(t) for t in img}) == len(img)
    keys = [tuple(t) for t in img]
    assert keys == sorted(keys)                                   # nx, then ny, then nz ascending
    assert keys[0] == (-N, 0, 0) and keys[-1] == (N, 0, 0)


def test_order_zero_is_one_windowed_sinc():
    L, s, m = np.array([3.0, 4.0, 2.6]), np.array([1.0, 1.5, 1.2]), np.array([2.1, 2.9, 1.4])
    fs, c = 8000, 343.0
    h, _ = ro.rir(L, s, m, 0.35, fs, c, 0)
    d = np.linalg.norm(s - m)
    tau = fs * d / c
    k = int(np.floor(tau + 0.5))
    j = np.arange(81)
    x = j - 40 - (tau - k)
    want = (0.5 - 0.5 * np.cos(2 * np.pi * j / 80)) * np.sin(np.pi * x) / (np.pi * x) / (4 * np.pi * d)
    assert h.shape == (1, 1, k + 81)
    assert np.all(h[0, 0, :k] == 0)
    assert np.max(np.abs(h[0, 0, k:] - want)) <= 1e-15 * np.max(np.abs(want))
    assert np.argmax(np.abs(h[0, 0])) == k + 40                   # the fixed lag H


def test_first_order_gains_with_hard_walls():
    L, s, m = np.array([3.0, 4.0, 2.6]), np.array([1.0, 1.5, 1.2]), np.array([2.1, 2.9, 1.4])
    k, phi, g = ro.image_terms(L, s, m, 0.0, 8000, 343.0, 1)
    img = ro.images(1)
    assert len(g) == 7
    for n, gain in zip(img, g):
        pos = np.where(n == 0, s, np.where(n > 0, 2 * L - s, -s))          # the mirror images of a box
        assert abs(gain - 1 / (4 * np.pi * np.linalg.norm(pos - m))) <= 1e-15 * gain
    # and each wall's beta reaches exactly the image reflected at that wall
    alpha = np.array([0.1, 0.25, 0.4, 0.55, 0.7, 0.85])
    _, _, g6 = ro.image_terms(L, s, m, alpha, 8000, 343.0, 1)
    wall = {(-1, 0, 0): 0, (1, 0, 0): 1, (0, -1, 0): 2, (0, 1, 0): 3, (0, 0, -1): 4, (0, 0, 1): 5}
    for n, a, b in zip(img, g, g6):
        want = 1.0 if tuple(n) == (0, 0, 0) else np.sqrt(1 - alpha[wall[tuple(n)]])
        assert abs(b / a - want) <= 1e-15


def test_reflection_counts_at_higher_order():
    """n = 3 on x: two reflections at the far wall, one at the wall at 0; n = -3: the other way round"""
    L, s, m = np.array([3.0, 4.0, 2.6]), np.array([1.0, 1.5, 1.2]), np.array([2.1, 2.9, 1.4])
    alpha = np.array([0.1, 0.5, 0.0, 0.0, 0.0, 0.0])
    img = ro.images(3)
    _, _, g0 = ro.image_terms(L, s, m, 0.0, 8000, 343.0, 3)
    _, _, g = ro.image_terms(L, s, m, alpha, 8000, 343.0, 3)
    ratio = dict(zip(map(tuple, img), g / g0))
    b0, b1 = np.sqrt(0.9), np.sqrt(0.5)
    assert abs(ratio[(3, 0, 0)] - b1 * b1 * b0) < 1e-15 and abs(ratio[(-3, 0, 0)] - b0 * b0 * b1) < 1e-15
    assert abs(ratio[(2, 1, 0)] - b1 * b0) < 1e-15 and abs(ratio[(-1, 0, 2)] - b0) < 1e-15


def test_source_and_microphone_exchange():
    case = cases.CASES[4]                                          # order 6
    g = cases.make_case(case)
    a, _ = ro.rir(g["room_dim"], g["sources"][:1], g["mics"][:1], g["absorption"], g["fs"], 343.0, g["max_order"])
    b, _ = ro.rir(g["room_dim"], g["mics"][:1], g["sources"][:1], g["absorption"], g["fs"], 343.0, g["max_order"])
    assert a.shape == b.shape
    err = np.max(np.abs(a - b)) / np.max(np.abs(a))
    print(f"reciprocity: {err:.2e} of the peak")
    assert err <= 1e-12


def test_oracle_premix_is_the_linear_convolution():
    room = cases.trio()[0]
    x, h, prem = room["signals"], room["rir"], room["premix"]
    assert prem.shape == (x.shape[0], h.shape[1], x.shape[1] + h.shape[2] - 1)
    n_out = prem.shape[2]
    for s in range(x.shape[0]):
        for m in range(h.shape[1]):
            # the same sum through the transform of the zero-padded pair: an independent route
            via_fft = np.fft.irfft(np.fft.rfft(x[s], 2 * n_out) * np.fft.rfft(h[s, m], 2 * n_out), 2 * n_out)[:n_out]
            assert np.max(np.abs(prem[s, m] - via_fft)) <= 1e-13 * np.linalg.norm(x[s]) * np.linalg.norm(h[s, m])
            assert np.array_equal(prem[s, m], np.convolve(x[s], h[s, m]))


@pytest.mark.parametrize("K,var", [(1, None), (2, (0.25, 1.0))])
def test_oracle_mix_down(K, var):
    room = cases.trio()[0]
    prem = room["premix"]
    S = prem.shape[0]
    sinr, ref_mic = 7.0, 1
    mix, ref = ro.mix_down(prem, K, sinr, 200.0, ref_mic, var, None)
    assert mix.shape == (prem.shape[2], prem.shape[1]) and ref.shape == (K + 1,) + mix.shape
    want = np.ones(K) if var is None else np.asarray(var)
    for s in range(K):
        assert abs(np.std(ref[s, :, ref_mic]) - np.sqrt(want[s])) <= 1e-12
    # powers at ref_mic, measured: the targets' from ref, the interferers' one by one (their sum in ref[K] also holds their
    # cross terms, so it is measured from ref[K] only where there is one interferer); snr = 200 makes the share the formula
    # reserves for the noise 1e-20 of the total
    p = prem / np.std(prem[:, ref_mic, :], axis=1)[:, None, None]
    sigma_i = np.sqrt(10 ** (-sinr / 10) * want.sum() / (S - K))
    target_power = sum(np.var(ref[s, :, ref_mic]) for s in range(K))
    interferer_power = sum(np.var(sigma_i * p[s, ref_mic]) for s in range(K, S))
    assert abs(target_power / interferer_power - 10 ** (sinr / 10)) <= 1e-9 * 10 ** (sinr / 10)
    if S - K == 1:
        assert abs(target_power / np.var(ref[K, :, ref_mic]) - 10 ** (sinr / 10)) <= 1e-9 * 10 ** (sinr / 10)
    assert np.max(np.abs(ref[K] - sigma_i * p[K:].sum(axis=0).T)) <= 1e-12 * np.max(np.abs(ref[K]))
    assert np.max(np.abs(mix - ref.sum(axis=0))) <= 1e-12 * np.max(np.abs(mix))
    # the clamp: an sinr the noise share alone exceeds leaves no interferer
    mix0, ref0 = ro.mix_down(prem, K, 70.0, 60.0, ref_mic, var, None)
    assert np.all(ref0[K] == 0)
    with pytest.raises(ValueError):
        ro.mix_down(prem, S, 10.0, 60.0)


# ---- admissibility ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_case_is_admissible(case):
    h, margin = cases.oracle_run(case)
    g = cases.make_case(case)
    print(f"{cases.case_id(case)}: tie margin {margin:.2e}, L = {h.shape[2]}")
    assert margin >= cases.MIN_MARGIN
    assert np.all((g["sources"] > 0) & (g["sources"] < g["room_dim"])) and np.all((g["mics"] > 0) & (g["mics"] < g["room_dim"]))
    assert np.all(np.isfinite(h)) and np.max(np.abs(h)) > 0


def test_trio_is_admissible():
    for room in cases.trio():
        assert room["margin"] >= cases.MIN_MARGIN
    assert len({r["rir"].shape[2] for r in cases.trio()}) == 3 and len({r["signals"].shape[1] for r in cases.trio()}) == 3


def test_near_case_starts_before_the_lag():
    case = [c for c in cases.CASES if cases.case_id(c).startswith("near")][0]
    g = cases.make_case(case)
    assert abs(np.linalg.norm(g["sources"][0] - g["mics"][0]) - 0.05) < 1e-12
    k, _, _ = ro.image_terms(g["room_dim"], g["sources"][0], g["mics"][0], g["absorption"], g["fs"], 343.0, 0)
    assert 0 <= k[0] < 40
