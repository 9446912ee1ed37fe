"""rir_batch() / simulate_batch() on the GPU against the NumPy restatement of DESIGN.md 3.11 (tests/helpers/room_oracle.py).

Bounds, derived and not measured:
  * impulse responses: 1e-9 * max|rir| of the pair.  A delay tau <= 2e4 samples carries a few units of 2^-53 relative error, which
    is <= 1e-11 samples; |sinc'| < 1.4, so a term is off by <= 1e-11 g, and the gains of the windows that overlap a sample sum to
    less than the direct one.  1e-9 leaves two orders of margin.
  * premix: 1e-12 * ||signal||_2 ||rir||_2 per output sample: the bound eps log2(n) of a convolution through the transform times
    a small constant is about 1e-14; two orders of margin.
  * mix-down: 1e-11 * max|mix|: the convolution bound plus a float64 reduction of length n.
Achieved on an MI355X: see DESIGN.md 3.11.

Shapes: orders 0, 1, 3, 4, 6 give 1, 7, 63, 129 and 377 images against the kernel's tables of 256 and ballots of 64; the lengths
come out between 129 and 1682 samples against a workgroup's slab of 1024 and a wave's 256; S x M of 1 x 1, 3 x 2 and 2 x 5."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

import room_cases as cases  # noqa: E402
import room_oracle as ro  # noqa: E402

pytestmark = pytest.mark.gpu

RIR_TOL = 1e-9
PREMIX_TOL = 1e-12
MIX_TOL = 1e-11


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _rir_error(got, want):
    """largest error of a pair relative to that pair's peak"""
    peak = np.max(np.abs(want), axis=2)
    return float(np.max(np.max(np.abs(got - want), axis=2) / peak))


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_rir_against_the_restatement(case):
    import overiva_amd as oa

    g = cases.make_case(case)
    want, margin = cases.oracle_run(case)
    got = oa.rir_batch(g["room_dim"][None], g["sources"][None], g["mics"][None], fs=g["fs"], max_order=g["max_order"],
                       absorption=g["absorption"][None], rir_length=g["rir_length"])
    info = oa.last_batch_info()
    if g["rir_length"] is None:
        assert isinstance(got, list) and len(got) == 1
    else:
        assert isinstance(got, np.ndarray) and got.shape[0] == 1 and got.shape[3] == g["rir_length"]
    h = got[0]
    assert h.shape == want.shape, (h.shape, want.shape)              # L_b from the device = the oracle's k_max + 81
    assert info["algorithm"] == "simulate" and info["max_order"] == g["max_order"] and info["rir_lengths"] == [want.shape[2]]
    assert info["images"] == ro.image_count(g["max_order"])
    err = _rir_error(h, want)
    print(f"{cases.case_id(case)}: rir error {err:.2e} of the peak (tie margin {margin:.1e})")
    assert err <= RIR_TOL


def test_scalar_and_per_room_absorption_agree():
    import overiva_amd as oa

    rooms = cases.trio()[:1]
    args = cases.trio_args(rooms)
    a = oa.rir_batch(**dict(args, absorption=0.3))
    b = oa.rir_batch(**dict(args, absorption=np.array([0.3])))
    c = oa.rir_batch(**args)                                          # (B, 6) of 0.3
    assert _same_bits(a[0], b[0]) and _same_bits(a[0], c[0])


@pytest.fixture(scope="module")
def trio_runs():
    """the trio as one batch (lists in, lists out), each room alone, and the batch once more: rir, premix, mix and ref"""
    import overiva_amd as oa

    rooms = cases.trio()
    noise = [np.random.default_rng(r["seed"] + 200).standard_normal((r["premix"].shape[2], cases.TRIO_M)) for r in rooms]
    mix_args = dict(n_targets=2, sinr=10.0, snr=60.0, ref_mic=1, sources_var=[0.5, 1.0])

    def run(idx):
        sel = [rooms[i] for i in idx]
        args = cases.trio_args(sel)
        sig = [r["signals"] for r in sel]
        rir = oa.rir_batch(**args)
        prem = oa.simulate_batch(sig, **args)
        mix, ref = oa.simulate_batch(sig, noise=[noise[i] for i in idx], **args, **mix_args)
        return dict(rir=rir, premix=prem, mix=mix, ref=ref, info=oa.last_batch_info())

    out = {"batch": run([0, 1, 2]), "again": run([0, 1, 2]), "noise": noise, "mix_args": mix_args}
    for i in range(3):
        out[("alone", i)] = run([i])
    for place, order in (("first", [1, 0, 2]), ("last", [0, 2, 1])):   # room 1 first, room 1 last (it is the middle of "batch")
        out[place] = run(order)
    return out


def test_bits_do_not_depend_on_the_batch(trio_runs):
    batch = trio_runs["batch"]
    assert batch["info"]["batched"] == 3 and batch["info"]["ragged"] and batch["info"]["lengths"] == [700, 1, 3001]
    for key in ("rir", "premix", "mix", "ref"):
        for i in range(3):
            assert _same_bits(batch[key][i], trio_runs[("alone", i)][key][0]), (key, i)
            assert _same_bits(batch[key][i], trio_runs["again"][key][i]), (key, i)                 # two runs of one call
        # room 1 alone, in the middle, first and last of three
        assert _same_bits(batch[key][1], trio_runs["first"][key][0]), key
        assert _same_bits(batch[key][1], trio_runs["last"][key][2]), key
        assert _same_bits(batch[key][0], trio_runs["first"][key][1]) and _same_bits(batch[key][2], trio_runs["last"][key][1]), key


def test_trio_rir_and_premix_against_the_restatement(trio_runs):
    """signals of 700, 1 and 3 001 samples in one list; every room of its own rir length"""
    batch = trio_runs["batch"]
    for i, room in enumerate(cases.trio()):
        assert batch["rir"][i].shape == room["rir"].shape
        assert _rir_error(batch["rir"][i], room["rir"]) <= RIR_TOL
        got, want = batch["premix"][i], room["premix"]
        assert got.shape == want.shape == (cases.TRIO_S, cases.TRIO_M, room["signals"].shape[1] + room["rir"].shape[2] - 1)
        scale = np.linalg.norm(room["signals"], axis=1)[:, None] * np.linalg.norm(room["rir"], axis=2)      # (S, M)
        err = float(np.max(np.max(np.abs(got - want), axis=2) / scale))
        print(f"room {i}: n = {room['signals'].shape[1]}, premix error {err:.2e} of ||x|| ||h||")
        assert err <= PREMIX_TOL


def test_dense_premix_is_stacked():
    """array in, array out when the rooms come out equally long (a fixed rir_length)"""
    import overiva_amd as oa

    rooms = cases.trio()[::2]
    args = dict(cases.trio_args(rooms), rir_length=400)
    sig = np.stack([r["signals"][:, :500] for r in rooms])
    prem = oa.simulate_batch(sig, **args)
    assert isinstance(prem, np.ndarray) and prem.shape == (2, cases.TRIO_S, cases.TRIO_M, 899)
    for b, r in enumerate(rooms):
        h, _ = ro.rir(r["room_dim"], r["sources"], r["mics"], r["absorption"], cases.TRIO_FS, 343.0, cases.TRIO_ORDER, 400)
        want = ro.premix(sig[b], h)
        scale = np.linalg.norm(sig[b], axis=1)[:, None] * np.linalg.norm(h, axis=2)
        assert np.max(np.max(np.abs(prem[b] - want), axis=2) / scale) <= PREMIX_TOL


@pytest.mark.parametrize("K,sinr,snr,with_noise", [(1, 10.0, 60.0, True), (2, 10.0, 60.0, True), (1, 10.0, 60.0, False),
                                                    (2, 10.0, 60.0, False), (2, 70.0, 60.0, True), (1, 70.0, 60.0, False)])
def test_mix_down_against_the_restatement(trio_runs, K, sinr, snr, with_noise):
    import overiva_amd as oa

    rooms = cases.trio()
    noise = trio_runs["noise"] if with_noise else None
    var = [0.5, 1.0][:K]
    mix, ref = oa.simulate_batch([r["signals"] for r in rooms], **cases.trio_args(rooms), n_targets=K, sinr=sinr, snr=snr, ref_mic=1,
                                 sources_var=var, noise=noise)
    for i, room in enumerate(rooms):
        want_mix, want_ref = ro.mix_down(room["premix"], K, sinr, snr, 1, var, None if noise is None else noise[i])
        assert mix[i].shape == want_mix.shape and ref[i].shape == want_ref.shape == (K + 1,) + want_mix.shape
        peak = np.max(np.abs(want_mix))
        e_mix, e_ref = np.max(np.abs(mix[i] - want_mix)) / peak, np.max(np.abs(ref[i] - want_ref)) / peak
        print(f"room {i} K={K} sinr={sinr}: mix error {e_mix:.2e}, ref error {e_ref:.2e} of max|mix|")
        assert e_mix <= MIX_TOL and e_ref <= MIX_TOL
        if sinr == 70.0 and noise is None:
            assert np.all(ref[i][K] == 0)                            # the clamp max(0, .): no interferer, no noise


def test_room_groups_do_not_change_the_bits(trio_runs):
    """the premix of the trio one room per group against all three at once"""
    from overiva_amd.room import RoomBatch

    rooms = cases.trio()
    args = cases.trio_args(rooms)
    with RoomBatch(args["room_dim"], args["sources"], args["mics"], fs=args["fs"], max_order=args["max_order"],
                   absorption=args["absorption"]) as rb:
        rb.compute_rir()
        assert rb.set_signals([r["signals"] for r in rooms], max_group=1) == 1
        prem = rb.simulate()
        mix, ref = rb.simulate(dict(trio_runs["mix_args"]), trio_runs["noise"])
        assert rb.info()["rooms_per_group"] == 1
    for i in range(3):
        assert _same_bits(prem[i], trio_runs["batch"]["premix"][i])
        assert _same_bits(mix[i], trio_runs["batch"]["mix"][i]) and _same_bits(ref[i], trio_runs["batch"]["ref"][i])


def test_noise_of_the_wrong_length_is_refused():
    import overiva_amd as oa

    rooms = cases.trio()[:1]
    with pytest.raises(ValueError, match="noise: room 0"):
        oa.simulate_batch([rooms[0]["signals"]], **cases.trio_args(rooms), n_targets=1, noise=[np.zeros((5, cases.TRIO_M))])


def test_end_to_end_pipeline_runs():
    """simulate_batch -> separate_batch -> bss_eval_batch completes with finite criteria: the pipeline runs; no claim on quality"""
    import overiva_amd as oa

    B, S, M, K, n = 2, 3, 3, 2, 4096
    rng = np.random.default_rng(5)
    dim = np.array([[5.0, 4.0, 2.7], [4.0, 6.0, 3.1]])
    sources = dim[:, None, :] * rng.uniform(0.15, 0.85, (B, S, 3))
    mics = dim[:, None, :] * rng.uniform(0.15, 0.85, (B, M, 3))
    envelope = 0.2 + np.abs(np.sin(np.arange(n)[None, None, :] / 400.0 + rng.uniform(0, 6, (B, S, 1))))
    signals = rng.standard_normal((B, S, n)) * envelope
    mix, ref = oa.simulate_batch(signals, dim, sources, mics, fs=8000, max_order=2, rir_length=512, n_targets=K, sinr=10.0, snr=30.0,
                                 noise=rng.standard_normal((B, n + 511, M)))
    assert mix.shape == (B, n + 511, M) and ref.shape == (B, K + 1, n + 511, M)
    y = oa.separate_batch(mix.astype(np.float32), 256, n_src=K, n_iter=5)
    assert y.shape[0] == B and y.shape[2] == K
    n_y = y.shape[1]
    sdr, sir, sar, perm = oa.bss_eval_batch(ref[:, :K, :n_y, 0], y.transpose(0, 2, 1).astype(np.float64), filter_length=64)
    assert sdr.shape == (B, K) and np.all(np.isfinite(sdr)) and np.all(np.isfinite(sir)) and np.all(np.isfinite(sar))
