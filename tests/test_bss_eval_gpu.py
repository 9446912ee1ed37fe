"""bss_eval_batch() / bss_eval_sources() on the GPU against the NumPy restatement of DESIGN.md 3.10 (tests/helpers/bss_eval_oracle.py).

Bounds: the float64 stages (G, D, E) to 1e-12 relative to the largest entry, the bound test_ilrma_gpu.py holds float64 stages to;
a solved system's defining property (G C = D, G_jj c = D[j]) to 1e-10 of ||D||; the three dB matrices within 10 x the
restatement's own spread on the room (bss_eval_cases.py: the larger of its reaction to a 1e-13 relative perturbation of the
inputs and the distance between its two forms), the factor test_ilrma_gpu.py uses for the same construction.

Measured on the CPU for the restatement (delta / distance between forms, dB; cond(G)):
    white N=1 n=300  Lf=8   : <= 3.4e-12 / <= 2.1e-12 ; 2
    white N=2 n=700  Lf=33  : <= 2.3e-12 / <= 4.8e-12 ; 3
    ar    N=3 n=1500 Lf=70  : <= 4.0e-12 / <= 6.6e-11 ; 1e3
    ar    N=5 n=1200 Lf=20  : 5.7e-12 / 3.7e-12       ; 5e2
    ar    N=2 n=4000 Lf=512 : 1.4e-12 / 5.1e-11       ; 3e3
    ar    N=4 n=2048 Lf=16  : 2.3e-12 / 3.9e-11       ; 3e2
    white N=6 n=2049 Lf=11  : <= 1.8e-12 / <= 4.8e-12 ; 2
    ar    N=7 n=1000 Lf=10  : 1.3e-12 / 2.1e-12       ; 3e2
    ar    N=8 n=900  Lf=9   : 1.1e-12 / 4.9e-12       ; 3e2
    white N=8 n=1100 Lf=64  : 1.8e-12 / 8.3e-12       ; 2e1
    white N=2 n=1500 Lf=257 : 1.3e-12 / 1.8e-12       ; 1e1
    ar    N=3 n=700  Lf=64  : 3.5e-12 / 9.8e-12       ; 1e3
    ar    N=4 n=640  Lf=128 : 4.6e-12 / 7.6e-12       ; 2e4
    white N=1 n=128  Lf=64  : 6.7e-13 / 2.9e-12       ; 3e1
Measured on an MI355X: see DESIGN.md 3.10.

The lag pass works in segments of 2048 samples: the 4000-sample case runs two segments with a partial last one, the 2048-sample
case exactly one, the 2049-sample case a second one of a single sample.

``test_stages_against_numpy[white-B1-N2-n1500-Lf257]`` is the case that made the lag pass add each 128-sample step from zero
and then the steps, not up to 2048 products in one chain.  The SAR of this room is 30-32 dB with ``E_k / art`` = 1e3 .. 1.7e3 in
``art = E_k - 2 D_k^T C_k + tot``, and the Gram form reacts to the last bits of G, D and E there: on the restatement's own G, D, E a
relative perturbation of 3e-16 per entry moves its SAR by up to 1.1e-11 dB, 1e-15 by 1.9e-11 dB.  With one chain per segment the
device's G and D were 4.5e-16 and 1.2e-15 from NumPy's and the SAR 2.04e-11 dB from the time-domain form against 10 x yardstick =
1.84e-11 dB (the NumPy Gram form on the DEVICE's G, D, E landed on the same 2.04e-11); with the steps added separately they are
1.5e-16 and 1.7e-16, and the distance is 2.27e-12 dB.  Over all cases G, D, E went from <= 2.9e-15 to <= 5.4e-16 and the worst
ratio of distance to bound from 1.11 to 0.59 (ar N=4 n=640 Lf=128: 4.45e-11 against 7.56e-11).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))

import bss_eval_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_stages_against_numpy(case):
    from overiva_amd.metrics import BssEval

    kind, B, N, n, Lf = case
    run = cases.oracle_run(case)
    with BssEval([n] * B, N, Lf) as ev:
        ev.set_signals(list(run["ref"]), list(run["est"]))
        ev.correlate()
        ev.factor()
        G, D, E = ev.get_gram()
        ev.solve()
        Cb, cs = ev.get_filters()
        ev.criteria()
        mats = ev.get_criteria()
        assert not ev.status().any()
    for b, room in enumerate(run["rooms"]):
        for name, got, want in (("G", G[b], room["G"]), ("D", D[b], room["D"]), ("E", E[b], room["E"])):
            err = np.max(np.abs(got - want)) / np.max(np.abs(want))
            print(f"{cases.case_id(case)} room {b} {name}: {err:.2e}")
            assert err <= 1e-12, (name, b, err)
        assert _same_bits(G[b], G[b].T.copy()), "G is not symmetric to the bit"
        res = np.linalg.norm(G[b] @ Cb[b].T - D[b].T) / np.linalg.norm(D[b])
        print(f"{cases.case_id(case)} room {b} |G C - D| / |D|: {res:.2e}")
        assert res <= 1e-10
        for j in range(N):
            sl = slice(j * Lf, (j + 1) * Lf)
            res = np.linalg.norm(G[b][sl, sl] @ cs[b, :, j].T - D[b][:, sl].T) / np.linalg.norm(D[b])
            assert res <= 1e-10, (b, j, res)
        got = tuple(m[b] for m in mats)
        dist = cases.db_distance(got, room["td"])
        print(f"{cases.case_id(case)} room {b} dB distance {dist:.2e} against 10 x yardstick {cases.FACTOR * room['yardstick']:.2e}")
        assert dist <= cases.FACTOR * room["yardstick"]
        if N == 1:
            assert np.isposinf(got[1]).all()


def test_ragged_rooms_have_the_bits_of_their_own_call():
    """the second trio: a room of exactly one 2048-sample segment, one of a segment and one sample, and a shorter one"""
    _ragged_rooms(2, 33, [700, 655, 1001])
    _ragged_rooms(4, 16, [2048, 2049, 1000])


def _ragged_rooms(N, Lf, lens):
    from overiva_amd import bss_eval_batch, last_batch_info

    rooms = [cases.make_room("white", N, n, 300 + b) for b, n in enumerate(lens)]
    out = bss_eval_batch([r for r, _ in rooms], [e for _, e in rooms], filter_length=Lf, return_matrices=True)
    info = last_batch_info()
    assert info["ragged"] is True and info["lengths"] == lens and info["batched"] == 3
    for b, (r, e) in enumerate(rooms):
        one = bss_eval_batch(r[None], e[None], filter_length=Lf, return_matrices=True)
        for a, o in zip(out, one):
            assert _same_bits(np.asarray(a[b], dtype=np.float64), np.asarray(o[0], dtype=np.float64)), b


def test_bits_do_not_depend_on_the_batch():
    """five rooms of three sources, then three rooms of eight: 72 vectors in the quadratic forms, 8 right-hand sides"""
    _batch_bits(5, 3, 20, 900, [3, 0, 4, 2, 1])
    _batch_bits(3, 8, 9, 900, [2, 0, 1])


def _batch_bits(B, N, Lf, n, order):
    from overiva_amd import bss_eval_batch
    from overiva_amd.metrics import BssEval

    rooms = [cases.make_room("ar", N, n, 400 + b) for b in range(B)]
    ref, est = np.stack([r for r, _ in rooms]), np.stack([e for _, e in rooms])
    together = bss_eval_batch(ref, est, filter_length=Lf, return_matrices=True)
    permuted = bss_eval_batch(ref[order], est[order], filter_length=Lf, return_matrices=True)
    for b in range(B):
        alone = bss_eval_batch(ref[b:b + 1], est[b:b + 1], filter_length=Lf, return_matrices=True)
        for t, a, p in zip(together[4:], alone[4:], permuted[4:]):
            assert _same_bits(t[b], a[0]), b
            assert _same_bits(t[b], p[order.index(b)]), b
    # ... nor on how the rooms are grouped for memory: groups of two rooms
    with BssEval([n] * B, N, Lf, max_group=2) as ev:
        assert ev.group == 2
        ev.set_signals(list(ref), list(est))
        ev.run()
        grouped = ev.get_criteria()
    for t, g in zip(together[4:], grouped):
        assert _same_bits(t, g)


def test_permutation_and_diagonal():
    from overiva_amd import bss_eval_batch

    N, Lf, n = 3, 20, 900
    ref, est = cases.make_room("ar", N, n, 500)
    shuffle = [2, 0, 1]                                   # est_shuffled[m] = est[shuffle[m]]: reference j is best served by
    want_perm = [shuffle.index(j) for j in range(N)]      # the estimate at position shuffle.index(j)
    sdr, sir, sar, perm, msdr, msir, msar = bss_eval_batch(ref[None], est[shuffle][None], filter_length=Lf, return_matrices=True)
    assert perm.shape == (1, N) and list(perm[0]) == want_perm
    assert _same_bits(sdr[0], msdr[0][want_perm, np.arange(N)])
    straight = bss_eval_batch(ref[None], est[None], filter_length=Lf)
    assert list(straight[3][0]) == [0, 1, 2]
    for a, b in zip((sdr, sir, sar), straight[:3]):
        assert _same_bits(a, b)
    d_sdr, d_sir, d_sar, d_perm, m_sdr, _, _ = bss_eval_batch(ref[None], est[None], compute_permutation=False, filter_length=Lf,
                                                              return_matrices=True)
    assert list(d_perm[0]) == [0, 1, 2]
    for a, b in zip((d_sdr, d_sir, d_sar), straight[:3]):
        assert _same_bits(a, b)
    assert np.isnan(m_sdr[0][~np.eye(N, dtype=bool)]).all()


def test_flagged_room():
    from overiva_amd import bss_eval_batch
    from overiva_amd.metrics import BssEval

    N, Lf, n = 2, 33, 700
    rooms = [cases.make_room("white", N, n, 600 + b) for b in range(3)]
    ref, est = np.stack([r for r, _ in rooms]), np.stack([e for _, e in rooms])
    ref[1, 1] = ref[1, 0]                                 # room 1: two identical references
    with pytest.raises(np.linalg.LinAlgError, match=r"problem\(s\) 1$"):
        bss_eval_batch(ref, est, filter_length=Lf)
    with BssEval([n] * 3, N, Lf) as ev:
        ev.set_signals(list(ref), list(est))
        ev.run()
        assert list(ev.status()) == [False, True, False]
        mats = ev.get_criteria(check=False)
    without = bss_eval_batch(ref[[0, 2]], est[[0, 2]], filter_length=Lf, return_matrices=True)
    for m, w in zip(mats, without[4:]):
        assert _same_bits(m[[0, 2]], w)


def test_one_room_call_dtypes_and_info():
    from overiva_amd import bss_eval_batch, bss_eval_sources, last_batch_info

    N, Lf, n = 2, 33, 700
    ref, est = cases.make_room("white", N, n, 700)
    one = bss_eval_sources(ref, est, filter_length=Lf)
    info = last_batch_info()
    assert info["algorithm"] == "bss_eval" and info["batched"] == 1 and info["n_sources"] == N and info["filter_length"] == Lf
    assert "lengths" not in info
    batch = bss_eval_batch(ref[None], est[None], filter_length=Lf)
    assert one[0].shape == (N,) and one[3].shape == (N,)
    for o, b in zip(one, batch):
        assert np.array_equal(o, b[0])
    r32, e32 = ref.astype(np.float32), est.astype(np.float32)
    f32 = bss_eval_sources(r32, e32, filter_length=Lf)
    f64 = bss_eval_sources(r32.astype(np.float64), e32.astype(np.float64), filter_length=Lf)
    for a, b in zip(f32[:3], f64[:3]):
        assert _same_bits(a, b)
    mono = bss_eval_sources(ref[0], est[0], filter_length=Lf)
    assert np.isposinf(mono[1]).all() and mono[0].shape == (1,)


def test_example_runs_and_separation_beats_the_mixture():
    out = subprocess.run([sys.executable, os.path.join(REPO, "examples", "sweep_batch_example.py"), "--rooms", "2", "--seconds", "4.0",
                          "--filter-length", "64", "--n-iter", "30"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [l for l in out.stdout.splitlines() if l.startswith("mean SIR")]
    assert lines, out.stdout
    mix, sep = (float(t) for t in lines[-1].replace("mean SIR: mixture", "").replace("dB", "").split("separated"))
    print(lines[-1])
    assert sep >= mix + 10.0
