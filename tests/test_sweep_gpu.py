"""sweep_batch() on the GPU.  The contract is bit equality with the chain of existing public calls (tests/helpers/sweep_chain.py):
every step of the sweep is the same kernel on the same bits or an exact operation (the cast the host does, an exact gather,
float32 -> float64), and the one inexact new value, the standard deviation of a channel, decides only an ordering -- the chain
asserts that the values it orders lie more than 1e-9 apart.  So nothing here has a tolerance but that standard deviation, which
two float64 passes over <= 3456 samples put within a few units of 2^-53 * log2(n) of NumPy's: 1e-12 relative leaves three orders.

Shapes: three rooms of 2312..3427 output samples, 3 microphones, 2 of 4 sources targets, frame 64 / hop 32: 72..107 frames of 33
bins, an odd sample count, one chunk of the standard deviation and 9..14 workgroups of the gather per room."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

import sweep_chain as sc  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("sdr", "sir", "sar", "perm")


def _same(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(a, b, equal_nan=True)


@pytest.fixture(scope="module")
def scenes():
    """the two scenes with their noise cut to the output lengths the device gives"""
    out = {}
    for kind in ("dense", "ragged"):
        for K in (1, 2):
            args = sc.scene(kind, K)
            out[kind, K] = sc.with_noise(args, sc.out_lengths(args))
    return out


@pytest.mark.parametrize("kind", ["dense", "ragged"])
def test_analysis_from_device_audio(scenes, kind):
    """float64 audio on the device -> X, against analysis_device(x.astype(float32)); and synthesis_keep + a copy against
    synthesis_device"""
    import overiva_amd as oa
    from overiva_amd import _lib

    args = scenes[kind, 2]
    sim = {k: args[k] for k in ("signals", "room_dim", "sources", "mics", "fs", "max_order", "absorption", "rir_length", "n_targets",
                                "sinr", "snr", "ref_mic", "sources_var", "noise")}
    mix, _ = oa.simulate_batch(**sim)
    mix = list(mix)
    lens = [a.shape[0] for a in mix]
    with oa.SweepBatch(args["room_dim"], args["sources"], args["mics"], sc.FRAME, sc.HOP, n_targets=2, fs=sc.FS, max_order=sc.ORDER,
                       absorption=args["absorption"], rir_length=args["rir_length"], ref_mic=sc.REF_MIC, filter_length=sc.LF) as sb:
        sb.set_signals(list(args["signals"]))
        assert sb.out_lengths == lens
        sb.set_filler(args["filler"])
        sb.open_group(0)
        with pytest.raises(RuntimeError):                      # not mixed yet
            sb.take_mix()
        sb.convolve(0)
        sb.mix(0, args["sinr"], args["snr"], np.asarray(args["sources_var"]), list(args["noise"]))
        Xd = sb.take_mix()
        got = Xd.get_x()
        dense = kind == "dense"
        with oa.BatchSTFT(lens[0] if dense else lens, sc.M, sc.FRAME, sc.HOP, B=3 if dense else None) as st:
            x32 = [a.astype(np.float32) for a in mix]
            Xw = st.analysis_device(np.stack(x32) if dense else x32)
            want = Xw.get_x()
            assert all(_same(g, w) for g, w in zip(got, want))
            assert sb.stft.phase_ms()["upload"] > 0
            # synthesis_keep + a plain copy = synthesis_device, for all three and for two channels
            for K in (3, 2):
                Y = np.ascontiguousarray(np.concatenate(list(want), axis=0)[:, :, :K])
                import torch

                Yd = torch.from_numpy(Y.view(np.float32)).cuda()
                y_want = st.synthesis_device(Yd.data_ptr(), K)
                dev = C.c_void_p()
                _lib.check(st.lib.oiva_bstft_synthesis_keep(st.h, C.c_void_p(Yd.data_ptr()), K, C.byref(dev)))
                y_got = np.empty((int(st.out_offsets[-1]), K), np.float32)
                _lib.check(st.lib.oiva_device_to_host(_lib.ptr(y_got), dev, y_got.nbytes))
                assert _same(y_got, np.concatenate(list(y_want), axis=0))
                assert st.phase_ms()["download"] == 0 and st.phase_ms()["overlap_add"] > 0


def test_order_statistics_and_gather(scenes):
    """the unprocessed microphones of the ragged scene: the order is not the identity and differs between rooms (the CPU test of
    the scene says so beforehand); est and ref are exact gathers; the standard deviation is NumPy's to 1e-12"""
    import overiva_amd as oa

    args = scenes["ragged", 2]
    sim = {k: args[k] for k in ("signals", "room_dim", "sources", "mics", "fs", "max_order", "absorption", "rir_length", "n_targets",
                                "sinr", "snr", "ref_mic", "sources_var", "noise")}
    mix, ref = oa.simulate_batch(**sim)
    lens = [a.shape[0] for a in mix]
    with oa.SweepBatch(args["room_dim"], args["sources"], args["mics"], sc.FRAME, sc.HOP, n_targets=2, fs=sc.FS, max_order=sc.ORDER,
                       absorption=args["absorption"], rir_length=None, ref_mic=sc.REF_MIC, filter_length=sc.LF) as sb:
        sb.set_signals(list(args["signals"]))
        sb.set_filler(args["filler"])
        sb.open_group(0)
        sb.convolve(0)
        sb.mix(0, args["sinr"], args["snr"], np.asarray(args["sources_var"]), list(args["noise"]))
        Xd = sb.take_mix()
        with oa.BatchSTFT(lens, sc.M, sc.FRAME, sc.HOP) as st:
            y = st.synthesis_device(st.analysis_device([a.astype(np.float32) for a in mix]))
        for reorder in (True, False):
            sb.evaluate(Xd, reorder)
            order, std = sb.get_order()
            ref_got, est_got = sb.get_eval_signals()
            want = [sc.order_and_gather(y[b], ref[b], args["filler"][b], 2, sc.REF_MIC, reorder) for b in range(3)]
            for b, (ref_w, est_w, order_w, std_w) in enumerate(want):
                print(f"room {b} reorder {reorder}: order {order[b]}, std error {np.max(np.abs(std[b] - std_w) / std_w):.2e}")
                assert np.array_equal(order[b], order_w)
                assert np.max(np.abs(std[b] - std_w) / std_w) <= 1e-12
                assert _same(ref_got[b], ref_w) and _same(est_got[b], est_w)
            if reorder:
                assert any(tuple(o) != (0, 1, 2) for o in order) and len({tuple(o) for o in order}) > 1, order
            else:
                assert all(tuple(o) == (0, 1, 2) for o in order)


CASES = [
    ("dense", 2, "overiva", dict(n_iter=12), False),            # 2 of 3 channels, no reorder
    ("ragged", 2, "overiva", dict(n_iter=25, model="gauss"), True),
    ("ragged", 2, "auxiva", dict(n_iter=12), False),            # 3 of 3 channels, reordered
    ("dense", 2, "auxiva", dict(n_iter=25), True),
    ("ragged", 2, "auxiva_pca", dict(n_iter=12), False),
    ("dense", 2, "auxiva_pca", dict(n_iter=25), True),
    ("dense", 1, "ogive", dict(n_iter=230, step_size=0.1, tol=1e-3), False),
    ("dense", 1, "ogive", dict(n_iter=230, step_size=0.1, tol=1e-3), True),
]


@pytest.mark.parametrize("kind,K,algo,kwargs,monitor", CASES, ids=[f"{c[0]}-{c[2]}-{'monitor' if c[4] else 'ends'}" for c in CASES])
def test_sweep_equals_the_chain(scenes, kind, K, algo, kwargs, monitor):
    import overiva_amd as oa

    args = scenes[kind, K]
    got = oa.sweep_batch(algorithms={"entry": {"algo": algo, "kwargs": kwargs}}, monitor_convergence=monitor, **sc.sweep_args(args))
    assert len(got) == 1 and got[0]["algorithm"] == "entry" and got[0]["n_targets"] == K and got[0]["n_mics"] == sc.M
    info = oa.last_batch_info()
    assert info["algorithm"] == "sweep" and info["groups"] == [3]
    want = sc.chain(args, algo, kwargs, monitor)
    assert got[0]["checkpoints"] == want["checkpoints"]
    if algo != "ogive":
        assert got[0]["checkpoints"] == oa.sweep.checkpoints(algo, kwargs["n_iter"], monitor)
    for key in KEYS:
        assert got[0][key].shape == (3, len(want["checkpoints"]), K + (key == "perm")), key
        assert _same(got[0][key], want[key]), (key, got[0][key], want[key])
    assert np.all(np.isfinite(got[0]["sdr"])) and got[0]["runtime"] > 0
    if algo == "ogive":
        assert len(got[0]["epochs"]) == len(got[0]["converged"]) == 3


def test_several_entries_share_one_stft(scenes):
    """two entries in one call = the two calls; the skip rules hold on the device path"""
    import overiva_amd as oa

    args = sc.sweep_args(scenes["ragged", 2])
    block = {"a": {"algo": "auxiva", "kwargs": {"n_iter": 5}}, "o": {"algo": "overiva", "kwargs": {"n_iter": 5}},
             "g": {"algo": "ogive", "kwargs": {"n_iter": 5}}}
    both = oa.sweep_batch(algorithms=block, **args)
    assert [r["algorithm"] for r in both] == ["a", "o"]
    for r in both:
        alone = oa.sweep_batch(algorithms={r["algorithm"]: block[r["algorithm"]]}, **args)[0]
        assert all(_same(r[k], alone[k]) for k in KEYS)
    assert all(_same(both[0][k][:, 0], both[1][k][:, 0]) for k in KEYS)       # the shared initial evaluation


def test_room_alone_and_groups(scenes):
    """room b of the batch of three = the call on that room alone; max_group=1 = one group"""
    import overiva_amd as oa

    full = scenes["ragged", 2]
    block = {"auxiva": {"algo": "auxiva", "kwargs": {"n_iter": 7}}}
    whole = oa.sweep_batch(algorithms=block, **sc.sweep_args(full))[0]
    grouped = oa.sweep_batch(algorithms=block, max_group=1, **sc.sweep_args(full))[0]
    assert oa.last_batch_info()["groups"] == [1, 1, 1]
    assert all(_same(whole[k], grouped[k]) for k in KEYS)
    for b in range(3):
        one = dict(sc.pick(sc.scene("ragged", 2), [b]))
        one["noise"] = [full["noise"][b]]
        alone = oa.sweep_batch(algorithms=block, **sc.sweep_args(one))[0]
        assert all(_same(alone[k][0], whole[k][b]) for k in KEYS), b


def test_a_room_too_short_for_a_frame_is_refused(scenes):
    import overiva_amd as oa

    args = sc.sweep_args(sc.pick(sc.scene("ragged", 2), [0, 1]))
    args["signals"] = [args["signals"][0], args["signals"][1][:, :3]]      # the impulse response alone is longer than a frame ...
    args["frame"], args["hop"] = 1024, 512                                  # ... of 64 samples, not of 1024; room 0 holds four
    with pytest.raises(ValueError, match="room 1 is too short for one complete frame"):
        oa.sweep_batch(**args)
