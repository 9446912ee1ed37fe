"""The decay measurement on the GPU: measure_rt60_batch(), edc_batch(), RoomBatch.measure_rt60 / set_absorption and
absorption_for_rt60() against the NumPy restatement (tests/helpers/decay_oracle.py).

  * curves: every E[n] > 0 within 1e-12 relative of the longdouble restatement -- the bound this project holds float64 stages to
    (TOL of tests/test_ilrma_gpu.py) -- and exact zeros equal.
  * i_a, i_b and rt60_cross: equal to the restatement's.  The condition is on the inputs: no crossing within 1e-9 relative of its
    threshold (tests/test_decay_host.py holds the inputs to it; the family keeps 3.3e-4).
  * rt60_fit: within max(1e-12, 10 delta) relative, delta = the float64-against-longdouble distance of the restatement on that
    input, on inputs whose window holds at least 32 samples; on shorter windows the NaN / finite status agrees.
  * everything else is bit equality: a response alone against the same response in any batch at any place, RoomBatch.measure_rt60
    against measure_rt60_batch of the downloaded responses, a handle after set_absorption against a fresh handle, a room's search
    alone against the same room's search in a batch.

Shapes (tests/helpers/decay_cases.py): lengths 1, 2, 63..65, 255..257 (lane, wave and workgroup edges of a cut tile), T - 1, T,
T + 1, 2 T + 1 for the kernel's tile T = 1024 (a whole tile, a tile and a cut one, two carries), at even and odd offsets of the
packed batch (16-byte and 8-byte loads), 4097 and 9000 (windows of 134..829 samples); rooms of 2 x 3 pairs at order 6 and of
2 x 2 pairs at order 8, fs = 8000.

The search test uses max_order = 8, absorption 0.3 for the targets and bracket = (0.12, 0.4): at that order the responses are
cut long before -25 dB and the measured time GROWS with the absorption inside the bracket (decay_cases.py tells the figures); every
pair's estimate is finite on the CPU (tests/test_decay_host.py).

Measured on an MI355X (each test prints its figures): curves 3.8e-16 from the longdouble restatement; rt60_fit 2.6e-15 on 30
windows of 134..829 samples; smallest crossing margin of the inputs 3.3e-4; the search converges in 5 steps per room, absorption
0.295 for all three rooms, measured 0.1206 / 0.1745 / 0.0979 s against targets 0.1215 / 0.1751 / 0.0983 s.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

import decay_cases as dc  # noqa: E402
import decay_oracle as do  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-12
FS = dc.FS


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def measured():
    """ONE call on the whole list: (inputs, cross, fit, curves, i_a, i_b) and the restatements in float64 and longdouble"""
    import overiva_amd as oa

    items = dc.curve_inputs() + dc.long_inputs()
    cross, fit, curves, (ia, ib) = oa.measure_rt60_batch(items, FS, return_curves=True, return_indices=True)
    info = oa.last_batch_info()
    assert info["algorithm"] == "decay" and info["precision"] == "float64" and info["batched"] == len(items)
    ref = [do.measure(h, FS, dtype=np.longdouble) for h in items]
    ref64 = [do.measure(h, FS) for h in items]
    return items, cross, fit, curves, ia, ib, ref, ref64


def test_curve(measured):
    items, _, _, curves, _, _, ref, _ = measured
    n_curve = len(dc.curve_inputs())
    worst = 0.0
    for h, E, r in zip(items[:n_curve], curves[:n_curve], ref[:n_curve]):
        assert E.shape == h.shape and E.dtype == np.float64
        want = r["E"]
        pos = want > 0
        assert np.array_equal(E[~pos], np.zeros(np.count_nonzero(~pos)))
        worst = max(worst, float(np.max(np.abs(E[pos] - want[pos]) / want[pos])))
    print(f"curves: largest relative distance from the longdouble restatement {worst:.3e} (bound {TOL:.0e})")
    assert worst <= TOL
    tail = curves[n_curve - 1]
    assert np.all(tail[-300:] == 0.0) and tail[-301] > 0          # the plateau of the trailing zeros is exact
    import overiva_amd as oa

    alone = oa.edc_batch(items[n_curve - 2])
    assert _same_bits(alone, curves[n_curve - 2])


def test_indices_and_estimates(measured):
    items, cross, fit, _, ia, ib, ref, ref64 = measured
    assert min(r["margin"] for r in ref) >= 1e-9          # the condition on the inputs
    worst, held = 0.0, 0
    for k, (r, r64) in enumerate(zip(ref, ref64)):
        assert (int(ia[k]), int(ib[k])) == (r["i_a"], r["i_b"]), (k, len(items[k]))
        assert np.isnan(cross[k]) == np.isnan(r["rt60_cross"]) and (np.isnan(cross[k]) or cross[k] == r64["rt60_cross"]), k
        assert np.isnan(fit[k]) == np.isnan(r["rt60_fit"]), (k, len(items[k]), fit[k], r["rt60_fit"])
        if r["i_b"] >= 0 and r["i_b"] - r["i_a"] >= 32:
            delta = abs(r64["rt60_fit"] - r["rt60_fit"]) / abs(r["rt60_fit"])
            dist = abs(fit[k] - r["rt60_fit"]) / abs(r["rt60_fit"])
            worst, held = max(worst, dist), held + 1
            assert dist <= max(TOL, 10 * delta), (k, len(items[k]), dist, delta)
    print(f"rt60_fit: largest relative distance from the longdouble restatement {worst:.3e} on {held} windows of >= 32 samples")
    assert held >= len(dc.long_inputs())


def test_degenerate_responses_do_not_disturb_the_others():
    import overiva_amd as oa

    a, b = do.family(4097, 0.05, FS), do.family(1025, 0.12, FS)
    batch = [a, np.zeros(500), np.array([0.7]), np.ones(40), b]
    cross, fit, curves, (ia, ib) = oa.measure_rt60_batch(batch, FS, return_curves=True, return_indices=True)
    assert (int(ia[1]), int(ib[1])) == (-1, -1) and np.isnan(cross[1]) and np.isnan(fit[1]) and np.all(curves[1] == 0.0)
    assert (int(ia[2]), int(ib[2])) == (-1, -1) and np.isnan(cross[2]) and np.isnan(fit[2]) and curves[2][0] == 0.7 * 0.7
    assert (int(ia[3]), int(ib[3])) == (28, -1) and np.isnan(cross[3]) and np.isnan(fit[3])          # never below -25 dB
    assert np.array_equal(curves[3], np.arange(40.0, 0.0, -1.0))
    c2, f2, e2, (ia2, ib2) = oa.measure_rt60_batch([a, b], FS, return_curves=True, return_indices=True)
    for i, j in ((0, 0), (4, 1)):
        assert _same_bits(curves[i], e2[j]) and _same_bits(cross[i], c2[j]) and _same_bits(fit[i], f2[j])
        assert ia[i] == ia2[j] and ib[i] == ib2[j] and np.isfinite(fit[i])
    # an array (..., L): shaped like the leading axes
    stack = np.stack([a[:1025], b]).reshape(2, 1, 1025)
    c3, f3 = oa.measure_rt60_batch(stack, FS)
    assert c3.shape == f3.shape == (2, 1) and _same_bits(f3[1, 0], fit[4])


def test_bits_do_not_depend_on_the_batch():
    from overiva_amd import acoustics

    items = [do.family(L, rt, FS) for L, rt in ((1, 0.05), (65, 0.05), (257, 0.12), (1023, 0.05), (1025, 0.3), (2049, 0.05), (4097, 0.12))]

    def run(order):
        with acoustics.DecayBatch([len(items[i]) for i in order]) as d:
            d.set(np.concatenate([items[i] for i in order])).run(FS, keep_curve=True)
            r, curves = d.get(), d.get_curves()
            assert d.ms() > 0
        return {i: (curves[k], {key: v[k] for key, v in r.items()}) for k, i in enumerate(order)}

    together = run(list(range(7)))
    permuted = run([6, 2, 5, 0, 3, 1, 4])
    for i in range(7):
        alone = run([i])
        for other in (together, permuted):
            assert _same_bits(alone[i][0], other[i][0]), i
            for key in ("e0", "sum_d", "sum_nd"):
                assert _same_bits(alone[i][1][key], other[i][1][key]), (i, key)
            assert alone[i][1]["i_a"] == other[i][1]["i_a"] and alone[i][1]["i_b"] == other[i][1]["i_b"], i
    assert together[6][1]["sum_d"] < 0 and together[6][1]["i_b"] > together[6][1]["i_a"] >= 0


def test_on_the_room_handle():
    import overiva_amd as oa
    from overiva_amd import room

    g = dc.HANDLE_ROOMS
    rng = np.random.default_rng(3)
    signals = [rng.standard_normal((2, 700)), rng.standard_normal((2, 900))]
    with room.RoomBatch(absorption=0.25, **g) as rb:
        with pytest.raises(RuntimeError):
            rb.measure_rt60()
        rb.compute_rir()
        cross, fit = rb.measure_rt60()
        assert oa.last_batch_info()["algorithm"] == "decay" and oa.last_batch_info()["batched"] == 2 * 2 * 3
        c2, f2 = oa.measure_rt60_batch(rb.get_rir(), FS)
        for b in range(2):
            assert cross[b].shape == (2, 3) and _same_bits(cross[b], c2[b]) and _same_bits(fit[b], f2[b])
            assert np.all(np.isfinite(fit[b]))
        c3, f3 = rb.measure_rt60(decay_db=10.0, start_db=0.0)
        c4, f4 = oa.measure_rt60_batch(rb.get_rir(), FS, decay_db=10.0, start_db=0.0)
        assert all(_same_bits(f3[b], f4[b]) and _same_bits(c3[b], c4[b]) for b in range(2))
        rb.set_signals(signals)
        rb.convolve(0)
        rb.get_premix(0)
        new = np.array([[0.4, 0.3, 0.2, 0.5, 0.1, 0.6], [0.15] * 6])
        rb.set_absorption(new)
        with pytest.raises(RuntimeError):          # the responses are stale
            rb.convolve(0)
        with pytest.raises(RuntimeError):
            rb.measure_rt60()
        rb.compute_rir()
        with pytest.raises(RuntimeError):          # the premix of the old responses is gone until the signals are convolved again
            rb.get_premix(0)
        rb.convolve(0)
        again, premix = rb.get_rir(), rb.get_premix(0)
        cross5, fit5 = rb.measure_rt60()
    with room.RoomBatch(absorption=new, **g) as fresh:
        fresh.compute_rir()
        fresh.set_signals(signals)
        fresh.convolve(0)
        want, want_premix = fresh.get_rir(), fresh.get_premix(0)
        cross6, fit6 = fresh.measure_rt60()
    for b in range(2):
        assert _same_bits(again[b], want[b]) and _same_bits(premix[b], want_premix[b])
        assert _same_bits(fit5[b], fit6[b]) and _same_bits(cross5[b], cross6[b])
        assert not _same_bits(fit5[b], fit[b])


def test_absorption_for_rt60():
    import overiva_amd as oa

    g = dc.SEARCH_ROOMS
    rirs = oa.rir_batch(absorption=dc.SEARCH_ABSORPTION, **g)
    target = np.array([dc.room_median(rirs[b])[0] for b in range(3)])
    kw = dict(max_order=g["max_order"], fs=FS, rir_length=g["rir_length"], bracket=dc.SEARCH_BRACKET)
    absorption, rt60, converged, steps = oa.absorption_for_rt60(g["room_dim"], g["sources"], g["mics"], target, **kw)
    print(f"targets {target}, absorption {absorption}, measured {rt60}, steps {steps}")
    assert converged.dtype == bool and converged.all()
    assert np.all(np.abs(rt60 - target) <= 0.01 * target)
    check = oa.rir_batch(g["room_dim"], g["sources"], g["mics"], fs=FS, max_order=g["max_order"], absorption=absorption,
                         rir_length=g["rir_length"])
    for b in range(3):
        value = dc.room_median(check[b])[0]
        assert abs(value - target[b]) <= 0.01 * target[b], (b, value, target[b])
    # a room alone returns the bits it returns in the batch
    b = 1
    alone = oa.absorption_for_rt60(g["room_dim"][b:b + 1], g["sources"][b:b + 1], g["mics"][b:b + 1], target[b], **kw)
    assert _same_bits(alone[0], absorption[b:b + 1]) and _same_bits(alone[1], rt60[b:b + 1])
    assert alone[2][0] == converged[b] and alone[3][0] == steps[b]
    # out of reach: no exception, not converged, the nearer end
    a10, r10, conv10, steps10 = oa.absorption_for_rt60(g["room_dim"], g["sources"], g["mics"], 10.0, **kw)
    assert not conv10.any() and np.all(steps10 == 2) and np.all(np.isin(a10, dc.SEARCH_BRACKET)) and np.all(np.isfinite(r10))
    # mixed: one reachable target, two not; the reachable room takes the steps it took before
    mixed = np.array([10.0, target[1], 1e-3])
    am, rm, cm, sm = oa.absorption_for_rt60(g["room_dim"], g["sources"], g["mics"], mixed, **kw)
    assert cm.tolist() == [False, True, False] and _same_bits(am[1], absorption[1]) and sm[1] == steps[1]


def test_c_entry_points():
    from overiva_amd import _lib, acoustics, room

    lib = _lib.load()
    g = dc.HANDLE_ROOMS
    h = do.family(300, 0.05, FS)
    with acoustics.DecayBatch([300]) as d:
        assert lib.oiva_decay_run(d.h, float(FS), 5.0, 20.0, 0) == _lib.ERR_STATE          # nothing set
        d.set(h)
        for bad in ((0.0, 5.0, 20.0), (float(FS), -1.0, 20.0), (float(FS), 5.0, 0.0), (float("nan"), 5.0, 20.0)):
            assert lib.oiva_decay_run(d.h, *bad, 0) == _lib.ERR_ARG, bad
        buf = np.empty(300)
        assert lib.oiva_decay_get(d.h, None, None, None, None, None) == _lib.ERR_STATE
        d.run(FS, keep_curve=False)
        assert lib.oiva_decay_get_curve(d.h, _lib.ptr(buf)) == _lib.ERR_STATE
        assert lib.oiva_decay_get(d.h, None, None, None, None, None) == _lib.OK
        ib = np.empty(1, dtype=np.int32)
        assert lib.oiva_decay_get(d.h, None, None, _lib.ptr(ib), None, None) == _lib.OK and ib[0] == do.measure(h, FS)["i_b"]
        d.run(FS, keep_curve=True)
        assert lib.oiva_decay_get_curve(d.h, _lib.ptr(buf)) == _lib.OK and buf[0] == d.get()["e0"][0]
        d.run(FS, keep_curve=False)
        assert lib.oiva_decay_get_curve(d.h, _lib.ptr(buf)) == _lib.ERR_STATE
    with room.RoomBatch(absorption=0.25, **g) as rb:
        L = g["rir_length"]
        with acoustics.DecayBatch([L] * 12) as d:
            assert lib.oiva_decay_set_room(d.h, rb.h) == _lib.ERR_STATE          # before compute_rir
            rb.compute_rir()
            assert lib.oiva_decay_set_room(d.h, rb.h) == _lib.OK
        for table in ([L] * 11, [L] * 11 + [L - 1], [L * 12]):
            with acoustics.DecayBatch(table) as d:
                assert lib.oiva_decay_set_room(d.h, rb.h) == _lib.ERR_ARG, table
        bad = np.full((2, 6), 1.0)
        assert lib.oiva_decay_room_set_absorption(rb.h, _lib.ptr(bad)) == _lib.ERR_ARG
        with pytest.raises(RuntimeError):          # without set_absorption the handle computes its responses once, as before
            rb.compute_rir()
