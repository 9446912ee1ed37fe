"""The seeded normal stream on the GPU and the calls that draw from it.

  * raw words: numpy.random.Philox's, bit for bit.
  * normals: within 1e-13 absolute of the NumPy restatement (tests/helpers/rng_oracle.py).  |r| <= 8.58; the restatement's angle
    2 pi u carries a rounding of a few 2 pi 2^-53 which the device's sinpi / cospi of the exact 2 u do not, and sqrt, log, sin and
    cos add a few units of 2^-53 each on either side: below 2e-14 in all, times five.  Largest difference measured on an MI355X:
    see DESIGN.md 3.13.
  * everything else is bit equality: a stream against its longer draw, a packed batch against its streams alone,
    simulate_batch(seed=) against simulate_batch(noise=) and sweep_batch(seed=) against sweep_batch(noise=, filler=) with the
    host arrays of standard_normal_batch.

Shapes: stream lengths 1..7 (every cut of the last block), 1023 (a cut block in the fourth workgroup) and 4097 (seventeen
workgroups, one value in the last block); the packed sizes (5, 3, 1, 10, 4, 7) put streams at odd offsets, where a stream's base
is 8-byte aligned only, and let a block's unused values fall onto the next stream; the rooms are those of the room and sweep
tests."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

import rng_oracle as rng_o  # noqa: E402
import room_cases as cases  # noqa: E402
import sweep_chain as sc  # noqa: E402

pytestmark = pytest.mark.gpu

NORMAL_TOL = 1e-13
SIZES = (1, 2, 3, 4, 5, 7, 1023, 4097)
PACKED = (5, 3, 1, 10, 4, 7)
KEYS = ("sdr", "sir", "sar", "perm")


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _same(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(a, b, equal_nan=True)


# ---- the stream -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,purpose,j", rng_o.RAW_CASES)
def test_raw_words_are_numpys(key, purpose, j):
    from overiva_amd import rng

    got = rng.raw_blocks(key, purpose, j, 1)
    assert got.shape == (1, 4) and got.dtype == np.uint64
    assert np.array_equal(got[0], rng_o.numpy_philox_block(key, purpose, j)), got


def test_a_run_of_raw_blocks_across_workgroups():
    """600 blocks from just below 2^32: three workgroups, the last one cut; numpy advances one generator through them"""
    from overiva_amd import rng

    first, n = 2 ** 32 - 300, 600
    got = rng.raw_blocks((123, rng_o.ALL_ONES), 1, first, n)
    counter = np.array([first - 1, 1, 0, 0], dtype=np.uint64)
    want = np.random.Philox(key=np.array([123, rng_o.ALL_ONES], dtype=np.uint64), counter=counter).random_raw(4 * n).reshape(n, 4)
    assert np.array_equal(got, want)


@pytest.fixture(scope="module")
def long_draws():
    """one draw of 4200 values per (key, purpose) of the normal tests"""
    import overiva_amd as oa

    seeds = [123, (1 << 64) - 1]
    return {(s, p): z for p in (0, 1) for s, z in zip(seeds, oa.standard_normal_batch([4200, 4200], seeds, purpose=p))}


@pytest.mark.parametrize("n", SIZES)
def test_normals_against_the_restatement(long_draws, n):
    import overiva_amd as oa

    worst = 0.0
    for (seed, purpose), longer in long_draws.items():
        got = oa.standard_normal_batch([n], [seed], purpose=purpose)[0]
        assert got.shape == (n,) and got.dtype == np.float64
        want = rng_o.standard_normal(n, (seed, 0), purpose)
        worst = max(worst, float(np.max(np.abs(got - want))))
        assert _same_bits(got, longer[:n]), (seed, purpose)          # a stream is a prefix of every longer draw
    print(f"n = {n}: largest difference to the restatement {worst:.2e}")
    assert worst <= NORMAL_TOL


def test_a_packed_batch_equals_its_streams_alone():
    """streams at odd offsets next to each other: no block writes past its stream's end, no store assumes 16-byte alignment"""
    import overiva_amd as oa

    seeds = [31, 32, 33, 34, 35, 36]
    for purpose in (0, 1):
        batch = oa.standard_normal_batch(PACKED, seeds, purpose=purpose)
        assert [len(z) for z in batch] == list(PACKED)
        for i, (n, s) in enumerate(zip(PACKED, seeds)):
            alone = oa.standard_normal_batch([n], [s], purpose=purpose)[0]
            assert _same_bits(batch[i], alone), (purpose, i)
            assert np.max(np.abs(alone - rng_o.standard_normal(n, (s, 0), purpose))) <= NORMAL_TOL
        # the same streams in another order and as the tail of a batch whose first stream ends on an odd element
        turned = oa.standard_normal_batch(PACKED[::-1], seeds[::-1], purpose=purpose)
        assert all(_same_bits(a, b) for a, b in zip(turned[::-1], batch))
        shifted = oa.standard_normal_batch((1023,) + PACKED, [7] + seeds, purpose=purpose)
        assert all(_same_bits(a, b) for a, b in zip(shifted[1:], batch))


def test_the_int_seed_names_the_keys_s_b():
    """seed = s is the key (s, b) for stream b, checked through the staged handle; the handle draws again on a second fill"""
    import overiva_amd as oa

    s = 2 ** 63 + 5
    got = oa.standard_normal_batch(PACKED, s)
    with oa.DeviceNormal(PACKED) as gen:
        with pytest.raises(RuntimeError):
            gen.get()                                               # nothing drawn yet
        want = gen.fill([s] * len(PACKED), list(range(len(PACKED)))).get()
        assert gen.ptr and gen.fill_ms() > 0
        assert all(_same_bits(a, b) for a, b in zip(got, want))
        for b, n in enumerate(PACKED):
            assert np.max(np.abs(want[b] - rng_o.standard_normal(n, (s, b), 0))) <= NORMAL_TOL
        again = gen.fill([s] * len(PACKED), [0] * len(PACKED), purpose=1).get()
        assert all(_same_bits(again[b], again[0][:n]) for b, n in enumerate(PACKED) if n <= PACKED[0])
    seq = oa.standard_normal_batch(PACKED, [s] * len(PACKED))      # the sequence form: every key (s, 0)
    assert _same_bits(seq[0], got[0]) and not _same_bits(seq[1], got[1])


def test_statistics_of_a_million_draws():
    """2^20 draws of key (123, 0), purposes 0 and 1, and of key (123, 1): every statistic inside five standard deviations, the
    Kolmogorov-Smirnov distance below its 0.1 % point (tests/test_rng_host.py holds the restatement to the same bounds)"""
    import overiva_amd as oa

    n = 1 << 20
    with oa.DeviceNormal([n, n]) as gen:
        a, c = gen.fill([123, 123], [0, 1], purpose=0).get()
        b = gen.fill([123, 123], [0, 1], purpose=1).get()[0]
    assert np.all(np.isfinite(a)) and np.max(np.abs(np.concatenate([a, b, c]))) <= 8.58
    for name, z, others in (("key (123, 0) purpose 0", a, (c, b)), ("key (123, 0) purpose 1", b, (c, a)),
                            ("key (123, 1) purpose 0", c, (a, b))):
        for stat, (value, bound) in rng_o.statistics(z, *others).items():
            print(f"{name}: {stat} {value:.3e} (bound {bound:.3e})")
            assert value < bound, (name, stat, value, bound)


# ---- simulate_batch(seed=) ------------------------------------------------------------------------------------------------------
MIX_ARGS = dict(n_targets=2, sinr=10.0, snr=20.0, ref_mic=1, sources_var=[0.5, 1.0])


def _trio(kind):
    """(signals, geometry arguments) of the ragged trio (700, 1 and 3001 samples, every room its own impulse response length) or of
    a dense pair (an array of signals, one rir_length)"""
    rooms = cases.trio()
    if kind == "ragged":
        return [r["signals"] for r in rooms], cases.trio_args(rooms)
    rooms = rooms[::2]
    return np.stack([r["signals"][:, :500] for r in rooms]), dict(cases.trio_args(rooms), rir_length=400)


@pytest.mark.parametrize("seed_form", ["sequence", "int"])
@pytest.mark.parametrize("max_group", [0, 1])
@pytest.mark.parametrize("kind", ["dense", "ragged"])
def test_simulate_with_a_seed_equals_simulate_with_that_noise(kind, max_group, seed_form):
    import overiva_amd as oa

    sig, args = _trio(kind)
    B = len(sig)
    seed = [911, 912, 913][:B] if seed_form == "sequence" else 77
    mix, ref = oa.simulate_batch(sig, **args, **MIX_ARGS, seed=seed, max_group=max_group)
    info = oa.last_batch_info()
    assert info["noise"] == "device" and info["rooms_per_group"] == (1 if max_group else B)
    n_out = [a.shape[0] for a in mix]
    assert len(set(n_out)) == (1 if kind == "dense" else 3)
    flat = oa.standard_normal_batch([n * cases.TRIO_M for n in n_out], seed, purpose=0)
    noise = [z.reshape(n, cases.TRIO_M) for z, n in zip(flat, n_out)]
    want_mix, want_ref = oa.simulate_batch(sig, **args, **MIX_ARGS, noise=noise if kind == "ragged" else np.stack(noise))
    assert oa.last_batch_info()["noise"] == "host"
    assert isinstance(mix, np.ndarray) == isinstance(want_mix, np.ndarray) == (kind == "dense")
    for b in range(B):
        assert _same_bits(mix[b], want_mix[b]) and _same_bits(ref[b], want_ref[b]), b
    quiet, _ = oa.simulate_batch(sig, **args, **MIX_ARGS)
    assert oa.last_batch_info()["noise"] is None and not _same_bits(quiet[0], mix[0])


def test_a_room_alone_with_its_own_seed():
    """with one seed per room a room's mix does not depend on the batch: room 1 of three = that room alone under seed[1]"""
    import overiva_amd as oa

    rooms = cases.trio()
    seeds = [911, 912, 913]
    mix, ref = oa.simulate_batch([r["signals"] for r in rooms], **cases.trio_args(rooms), **MIX_ARGS, seed=seeds)
    for b in (1, 2):
        one_mix, one_ref = oa.simulate_batch([rooms[b]["signals"]], **cases.trio_args([rooms[b]]), **MIX_ARGS, seed=[seeds[b]])
        assert _same_bits(one_mix[0], mix[b]) and _same_bits(one_ref[0], ref[b]), b
    # the int form names the room's index: room 1 alone is index 0 and draws another stream
    by_index, _ = oa.simulate_batch([r["signals"] for r in rooms], **cases.trio_args(rooms), **MIX_ARGS, seed=912)
    alone, _ = oa.simulate_batch([rooms[0]["signals"]], **cases.trio_args([rooms[0]]), **MIX_ARGS, seed=912)
    assert _same_bits(alone[0], by_index[0])
    moved, _ = oa.simulate_batch([rooms[1]["signals"]], **cases.trio_args([rooms[1]]), **MIX_ARGS, seed=912)
    assert not _same_bits(moved[0], by_index[1])


# ---- sweep_batch(seed=) ---------------------------------------------------------------------------------------------------------
BLOCK = {"overiva": {"algo": "overiva", "kwargs": {"n_iter": 6}}}


def _sweep_scene(kind):
    """the scene without its noise and filler, and its output and evaluation lengths"""
    args = sc.scene(kind)
    lens = sc.out_lengths(args)
    plain = {k: v for k, v in args.items() if not k.startswith("_") and k != "filler"}
    return plain, lens, [sc.eval_length(n) for n in lens]


@pytest.mark.parametrize("kind,max_group,own_filler", [("dense", 0, False), ("ragged", 0, False), ("ragged", 1, False),
                                                        ("dense", 0, True)],
                         ids=["dense", "ragged", "ragged-groups-of-1", "dense-own-filler"])
def test_sweep_with_a_seed_equals_sweep_with_those_arrays(kind, max_group, own_filler):
    import overiva_amd as oa

    plain, lens, m = _sweep_scene(kind)
    seeds = [501, 502, 503]
    filler = list(sc.scene(kind)["filler"]) if own_filler else None
    got = oa.sweep_batch(algorithms=BLOCK, seed=seeds, filler=filler, max_group=max_group, **plain)[0]
    info = oa.last_batch_info()
    assert info["noise"] == "device" and info["groups"] == ([1, 1, 1] if max_group else [3])
    assert got["n_samples"] == lens
    flat = oa.standard_normal_batch([n * sc.M for n in lens], seeds, purpose=0)
    noise = [z.reshape(n, sc.M) for z, n in zip(flat, lens)]
    rows = filler if own_filler else oa.standard_normal_batch(m, seeds, purpose=1)
    want = oa.sweep_batch(algorithms=BLOCK, noise=noise if kind == "ragged" else np.stack(noise), filler=rows, max_group=max_group,
                          **plain)[0]
    assert oa.last_batch_info()["noise"] == "host"
    assert got["checkpoints"] == want["checkpoints"] == [0, 6]
    for key in KEYS:
        assert _same(got[key], want[key]), (key, got[key], want[key])
    assert np.all(np.isfinite(got["sdr"]))


def test_sweep_with_a_seed_and_the_callers_noise():
    """seed with noise given: only the filler is drawn; the default of both, seed=None, draws nothing"""
    import overiva_amd as oa

    plain, lens, m = _sweep_scene("dense")
    noise = np.stack([a[:n] for a, n in zip(sc.scene("dense")["_noise"], lens)])
    got = oa.sweep_batch(algorithms=BLOCK, seed=9, noise=noise, **plain)[0]
    assert oa.last_batch_info()["noise"] == "host"
    rows = oa.standard_normal_batch(m, 9, purpose=1)
    want = oa.sweep_batch(algorithms=BLOCK, noise=noise, filler=rows, **plain)[0]
    assert all(_same(got[k], want[k]) for k in KEYS)
    oa.sweep_batch(algorithms=BLOCK, **plain)
    assert oa.last_batch_info()["noise"] is None


def test_the_staged_sweep_draws_the_filler_where_it_is_read():
    """set_filler(seed=): the row K of est that evaluate leaves is the purpose-1 stream, bit for bit, group after group"""
    import overiva_amd as oa

    plain, lens, m = _sweep_scene("ragged")
    rows = oa.standard_normal_batch(m, 31, purpose=1)
    with oa.SweepBatch(plain["room_dim"], plain["sources"], plain["mics"], sc.FRAME, sc.HOP, n_targets=sc.K, fs=sc.FS,
                       max_order=sc.ORDER, absorption=plain["absorption"], rir_length=None, ref_mic=sc.REF_MIC,
                       filter_length=sc.LF) as sb:
        assert sb.set_signals(list(plain["signals"]), max_group=2) == 2
        sb.set_filler(seed=31)
        for g0 in (0, 2):
            sb.open_group(g0)
            sb.convolve(g0)
            keys = ([31] * len(sb.rooms), list(sb.rooms))
            sb.mix(g0, sc.SINR, sc.SNR, np.asarray(plain["sources_var"]), seed_keys=keys)
            sb.evaluate(sb.take_mix(), True)
            _, est = sb.get_eval_signals()
            for i, b in enumerate(sb.rooms):
                assert _same_bits(est[i][sc.K], rows[b]), b
        with pytest.raises(ValueError):
            sb.set_filler(filler=rows, seed=31)
        sb.set_filler([np.zeros(n) for n in m])                    # back to a caller's rows, on the open group
        sb.evaluate(sb.take_mix(), True)
        assert np.all(sb.get_eval_signals()[1][0][sc.K] == 0)
