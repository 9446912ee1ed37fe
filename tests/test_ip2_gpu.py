"""overiva_ip2_batch() on the GPU against the NumPy restatement (tests/helpers/ip2_oracle.py; DESIGN.md 3.17 is the contract).

Every figure is printed before it is asserted.  The bounds are the project's own: 1e-12 of the largest entry for a float64 stage,
1e-10 for the defining properties, max(1e-12, 10 delta) for iterated results, delta being how far a 1e-13 relative perturbation
of X moves the restatement's own W (test_ip2_host.py::test_cases_are_reproducible)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

import ip2_cases as cases  # noqa: E402
import ip2_oracle as ipo  # noqa: E402

pytestmark = pytest.mark.gpu


def make_plan(X, K, model="laplace"):
    """an open plan for an array of rooms or a list of rooms of different lengths, X and the covariance set"""
    import overiva_amd as oa

    if isinstance(X, list):
        plan = oa.RaggedBatchPlan([x.shape[0] for x in X], X[0].shape[1], X[0].shape[2], K, model)
    else:
        plan = oa.BatchPlan(X.shape[0], X.shape[1], X.shape[2], X.shape[3], K, model)
    plan.set_x(X)
    plan.covariance()
    return plan


def run_device(X, K, n, model="laplace", W0=None, chunks=None):
    """W (B, F, M, K) complex128 after n iterations, cut into ``chunks`` calls"""
    with make_plan(X, K, model) as plan:
        plan.set_w(W0)
        first = 0
        for c in chunks or [n]:
            plan.ip2_iterate(first, c)
            first += c
        assert first == n
        return plan.get_w(np.complex128)


# ---- 1. the UPDATE stage alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.UPDATE_CASES, ids=cases.update_id)
def test_update_stage_against_the_oracle(case):
    """stages 0 to 2 on the device, then UPDATE against the restatement fed the device's own V, Cx and W, at both parities"""
    (B, T, F, M, K), model = case
    X, W0 = cases.update_inputs(case)
    with make_plan(X, K, model) as plan:
        Cx = plan.get_cx()
        for parity in (0, 1):
            plan.set_w(W0)
            for stage in ("power", "activation", "cov"):
                plan.ip2_stage(stage, parity)
            V = plan.get_weighted_cov()                       # (B, F, K, M, M)
            W = plan.get_w(np.complex128)                     # scaled by the activation
            plan.ip2_stage("update", parity)
            got = plan.get_w(np.complex128)
            assert np.all(np.isfinite(got))
            dist = prop = jorth = rise = 0.0
            for b in range(B):
                # J is a function of W and Cx alone, and does not change when W's columns are scaled
                W_hat = ipo.init_w_hat(Cx[b], K, W[b])
                want = ipo.update(W_hat, V[b], Cx[b], K, parity)
                dist = max(dist, float(np.max(np.abs(got[b] - want[:, :, :K])) / np.max(np.abs(want[:, :, :K]))))
                dev = ipo.init_w_hat(Cx[b], K, got[b])
                jorth = max(jorth, ipo.j_orthogonality(dev, Cx[b], K))
                done = []
                for step in ipo.schedule(K, parity):          # the other columns: those of the steps before, which no longer move
                    if len(step) == 2:
                        prop = max(prop, ipo.pair_properties(dev, V[b][:, step[0]], V[b][:, step[1]], *step, others=done))
                    else:
                        prop = max(prop, ipo.single_properties(dev, V[b][:, step[0]], step[0], others=done))
                    done += list(step)
                if K == M:
                    s0, s1 = ipo.surrogate(W_hat, V[b], K), ipo.surrogate(dev, V[b], K)
                    rise = max(rise, float(np.max((s1 - s0) / np.abs(s0))))
                    ip1 = ipo.surrogate(ipo.update_ip1(W_hat, V[b], Cx[b], K), V[b], K)
                    if K == 2:                                # one pair step against IP1 on 0 then 1 from the same start
                        assert np.all(s1 <= ip1 + 1e-12 * np.abs(ip1))
            print(f"ip2 update {cases.update_id(case)} parity {parity}: W {dist:.2e}, properties {prop:.2e}, J {jorth:.2e}, "
                  f"surrogate rise {rise:.2e}")
            assert dist <= 1e-12
            assert prop <= 1e-10 and jorth <= 1e-10
            assert rise <= 1e-12


def test_the_update_needs_its_iteration_index():
    """odd K: the two parities run different schedules from the same state"""
    case = ((1, 70, 17, 6, 5), "laplace")
    X, W0 = cases.update_inputs(case)
    out = []
    with make_plan(X, 5) as plan:
        for parity in (0, 1, 2):
            plan.set_w(W0)
            plan.ip2_iterate(parity, 1)
            out.append(plan.get_w(np.complex128))
    assert np.array_equal(out[0], out[2]) and not np.array_equal(out[0], out[1])


# ---- 2. iterated results -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.ITERATED, ids=cases.case_id)
def test_iterated_against_the_oracle(case):
    kind, (T, F, M, K), model = case
    run = cases.oracle_run(case)
    for n in cases.counts(case):
        W = run_device(run["X"][None], K, n, model)[0]
        d, bound = cases.rel(W, run[n]["W"]), max(1e-12, 10 * run[n]["delta"])
        print(f"ip2 iterated {cases.case_id(case)} n={n}: device W {d:.2e}, bound {bound:.2e} (delta {run[n]['delta']:.2e})")
        assert d <= bound


def test_overiva_ip2_is_overiva_ip2_batch_of_one_room():
    import overiva_amd as oa

    T, F, M, K = 70, 17, 4, 2
    X = cases.make_x("mix", T, F, M, K)
    one = oa.overiva_ip2(X, n_src=K, n_iter=4, return_filters=True)
    bat = oa.overiva_ip2_batch(X[None], n_src=K, n_iter=4, return_filters=True)
    assert one[0].shape == (T, F, K) and one[0].dtype == np.complex64 and one[1].shape == (F, M, K)
    assert np.array_equal(one[0], bat[0][0]) and np.array_equal(one[1], bat[1][0])
    assert np.array_equal(oa.overiva_ip2(X, n_src=K, n_iter=4), one[0])                  # Y alone
    info = oa.last_batch_info()
    assert info["algorithm"] == "overiva_ip2" and info["batched"] == 1 and info["shape"] == (T, F, M, K)
    # the filters are the plan's, and Y is their output
    assert np.array_equal(run_device(X[None], K, 4).astype(np.complex64), bat[1])
    with make_plan(X[None], K) as plan:
        plan.set_w(bat[1][0].astype(np.complex128))
        assert cases.rel(plan.demix(True), bat[0]) <= 1e-5
    # W0: the identity is the default; another start gives another result; the eigenvector start is the plan's
    eye = np.zeros((F, M, K))
    eye[:, :K, :] = np.eye(K)
    assert np.array_equal(oa.overiva_ip2(X, n_src=K, n_iter=4, W0=eye), one[0])
    W0 = cases.random_w0(1, F, M, K)
    Yw, Ww = oa.overiva_ip2_batch(X[None], n_src=K, n_iter=4, W0=W0, return_filters=True)
    assert np.array_equal(Ww, run_device(X[None], K, 4, W0=W0).astype(np.complex64)) and not np.array_equal(Ww, bat[1])
    Ye, We = oa.overiva_ip2(X, n_src=K, n_iter=2, init_eig=True, return_filters=True)
    with make_plan(X[None], K) as plan:
        plan.set_w_eig()
        plan.ip2_iterate(0, 2)
        assert np.array_equal(plan.get_w(np.complex64)[0], We) and np.array_equal(plan.demix(True)[0], Ye)
    assert not np.array_equal(We, oa.overiva_ip2(X, n_src=K, n_iter=2, return_filters=True)[1])
    # determined by default
    Yd = oa.overiva_ip2(X, n_iter=2)
    assert Yd.shape == (T, F, M)


def test_callback_cadence():
    import overiva_amd as oa

    B, T, F, M, K = 2, 70, 17, 3, 3
    X = np.stack([cases.make_x("mix", T, F, M, K, seed=cases.SEED + b) for b in range(B)])
    got = []
    Y = oa.overiva_ip2_batch(X, n_iter=22, callback=lambda Y: got.append(Y.copy()))
    assert len(got) == 3 and all(g.shape == (B, T, F, K) for g in got)          # iterations 0, 10 and 20
    assert np.array_equal(got[0], oa.overiva_ip2_batch(X, n_iter=0))
    assert np.array_equal(got[1], oa.overiva_ip2_batch(X, n_iter=10))
    assert np.array_equal(got[2], oa.overiva_ip2_batch(X, n_iter=20))
    assert np.array_equal(Y, oa.overiva_ip2_batch(X, n_iter=22))                # the callback does not change the result


# ---- 3. bit rules ----------------------------------------------------------------------------------------------------------------------
BITS = [(4, 2), (3, 3)]


@pytest.mark.parametrize("M,K", BITS, ids=lambda v: str(v))
def test_chunks_do_not_change_the_bits(M, K):
    X = cases.make_rooms(2, 70, 17, M, K)
    whole = run_device(X, K, 5)
    assert np.all(np.isfinite(whole))
    assert np.array_equal(whole, run_device(X, K, 5, chunks=[2, 3]))
    assert np.array_equal(whole, run_device(X, K, 5, chunks=[1, 1, 1, 1, 1]))


@pytest.mark.parametrize("M,K", BITS, ids=lambda v: str(v))
def test_bits_do_not_depend_on_the_batch(M, K):
    B = 5
    X = cases.make_rooms(B, 70, 17, M, K)
    full = run_device(X, K, 5)
    perm = [3, 0, 4, 2, 1]
    shuffled = run_device(X[perm], K, 5)
    for b in range(B):
        alone = run_device(X[b:b + 1], K, 5)
        assert np.all(np.isfinite(alone))
        assert np.array_equal(alone[0], full[b]) and np.array_equal(alone[0], shuffled[perm.index(b)]), b


@pytest.mark.parametrize("M,K", BITS, ids=lambda v: str(v))
def test_rooms_of_different_lengths_have_the_bits_of_their_dense_batch(M, K):
    import overiva_amd as oa

    Xs = [cases.make_x("mix", T, 17, M, K, seed=cases.SEED + b) for b, T in enumerate((70, 257, 64))]
    W = run_device(Xs, K, 5)
    Ys = oa.overiva_ip2_batch(Xs, n_src=K, n_iter=5)
    assert isinstance(Ys, list) and [y.shape for y in Ys] == [x.shape[:2] + (K,) for x in Xs]
    assert oa.last_batch_info()["ragged"] and oa.last_batch_info()["frames"] == [70, 257, 64]
    for b, x in enumerate(Xs):
        assert np.all(np.isfinite(W[b]))
        assert np.array_equal(run_device(x[None], K, 5)[0], W[b]), b
        assert np.array_equal(oa.overiva_ip2_batch(x[None], n_src=K, n_iter=5)[0], Ys[b]), b


# ---- 4. an all-zero room ---------------------------------------------------------------------------------------------------------------
def test_an_all_zero_room_is_named_and_leaves_the_others_alone():
    import overiva_amd as oa

    X = cases.make_rooms(3, 70, 17, 4, 2)
    clean = run_device(X, 2, 3)
    X[1] = 0
    with make_plan(X, 2) as plan:
        plan.set_w(None)
        plan.ip2_iterate(0, 3)
        assert list(plan.status()) == [False, True, False]
        with pytest.raises(np.linalg.LinAlgError, match=r"problem\(s\) 1\b"):
            plan.get_w()
        W = plan.get_w(check=False)
    assert np.array_equal(W[0], clean[0]) and np.array_equal(W[2], clean[2])
    assert not np.all(np.isfinite(W[1]))
    with pytest.raises(np.linalg.LinAlgError):
        oa.overiva_ip2_batch(X, n_src=2, n_iter=3)


# ---- 5. audio in, audio out ------------------------------------------------------------------------------------------------------------
def _audio(seed, n, M):
    rng = np.random.default_rng(seed)
    env = np.repeat(rng.gamma(0.3, 1.0, (n // 512 + 1, M)), 512, axis=0)[:n]
    A = rng.standard_normal((M, M)) + 2 * np.eye(M)
    return ((env * rng.standard_normal((n, M))) @ A.T).astype(np.float32)


def test_separate_batch_is_the_composed_path():
    """separate_batch(algorithm="overiva_ip2") against stft.analysis -> overiva_ip2_batch -> stft.synthesis per room, bit for bit,
    for an array and for a list of rooms"""
    import overiva_amd as oa
    from overiva_amd import stft

    L, HOP, M, K = 64, 32, 3, 2
    wa = stft.hann(L)
    ws = stft.compute_synthesis_window(wa, HOP)
    for xs in (np.stack([_audio(s, 3200, M) for s in (1, 2, 3)]), [_audio(s, n, M) for s, n in ((4, 3200), (5, 2217), (6, 4800))]):
        Xc = [stft.analysis(x, L, HOP, win=wa) for x in xs]
        Yc, Wc = oa.overiva_ip2_batch(Xc if isinstance(xs, list) else np.stack(Xc), n_src=K, n_iter=6, return_filters=True)
        yc = [stft.synthesis(Y, L, HOP, win=ws) for Y in Yc]
        yb, Wb = oa.separate_batch(xs, L, HOP, n_src=K, n_iter=6, algorithm="overiva_ip2", return_filters=True)
        assert oa.last_batch_info()["algorithm"] == "overiva_ip2"
        assert np.array_equal(Wb.astype(np.complex64), Wc)
        assert len(yb) == len(yc) == 3
        for a, b in zip(yb, yc):
            assert a.shape == b.shape and np.array_equal(a, b)


def test_sweep_puts_ip1_and_ip2_side_by_side():
    """one "overiva" and one "overiva_ip2" entry on one X with monitoring: both rows, the same checkpoints, and the ip2 row's
    final criteria equal to simulate_batch -> separate_batch(algorithm="overiva_ip2") -> bss_eval_batch bit for bit"""
    import overiva_amd as oa

    import sweep_chain as sc

    args = sc.scene("dense", 2)
    args = sc.with_noise(args, sc.out_lengths(args))
    block = {"ip1": {"algo": "overiva", "kwargs": {"n_iter": 12}}, "ip2": {"algo": "overiva_ip2", "kwargs": {"n_iter": 12}}}
    rows = oa.sweep_batch(algorithms=block, monitor_convergence=True, **sc.sweep_args(args))
    assert [r["algorithm"] for r in rows] == ["ip1", "ip2"]
    assert rows[0]["checkpoints"] == rows[1]["checkpoints"] == [0, 10, 12]
    for key in ("sdr", "sir", "sar"):
        assert rows[0][key].shape == rows[1][key].shape == (3, 3, 2) and np.all(np.isfinite(rows[1][key]))
        assert np.array_equal(rows[0][key][:, 0], rows[1][key][:, 0])           # iteration 0: the same start
        assert not np.array_equal(rows[0][key][:, -1], rows[1][key][:, -1])
    print("sweep SDR at", rows[0]["checkpoints"], "IP1", rows[0]["sdr"].mean(axis=(0, 2)), "IP2", rows[1]["sdr"].mean(axis=(0, 2)))
    # the chain of public calls
    sim = {k: args[k] for k in ("signals", "room_dim", "sources", "mics", "fs", "max_order", "absorption", "rir_length", "n_targets",
                                "sinr", "snr", "ref_mic", "sources_var", "noise")}
    mix, ref = oa.simulate_batch(**sim)
    y = oa.separate_batch(np.stack([m.astype(np.float32) for m in mix]), sc.FRAME, sc.HOP, n_src=2, n_iter=12, algorithm="overiva_ip2")
    gathered = [sc.order_and_gather(y[b], ref[b], args["filler"][b], 2, args["ref_mic"], False) for b in range(3)]
    sdr, sir, sar, perm = oa.bss_eval_batch([g[0] for g in gathered], [g[1] for g in gathered], filter_length=sc.LF)
    for key, want in (("sdr", sdr), ("sir", sir), ("sar", sar)):
        assert np.array_equal(rows[1][key][:, -1], want[:, :2]), key
    assert np.array_equal(rows[1]["perm"][:, -1], perm)
    # the determined form runs on all the channels and is reordered
    det = oa.sweep_batch(algorithms={"d": {"algo": "auxiva_ip2", "kwargs": {"n_iter": 3}}}, **sc.sweep_args(args))
    assert det[0]["checkpoints"] == [0, 3] and np.all(np.isfinite(det[0]["sdr"]))


# ---- 6. the C entries --------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_c_entries():
    import ctypes

    import overiva_amd as oa
    from overiva_amd import _lib

    lib = _lib.load()
    X = cases.make_x("iid", 20, 5, 3, 3)[None]
    ms = (ctypes.c_float * 4)()
    with oa.BatchPlan(1, 20, 5, 3, 2, data="complex128") as plan:
        for call in (lambda: lib.oiva_batch_ip2_iterate(plan.h, 0, 1), lambda: lib.oiva_batch_ip2_stage(plan.h, 3, 0),
                     lambda: lib.oiva_batch_ip2_time_stages(plan.h, 1, ms)):
            assert call() == _lib.ERR_ARG and b"complex128" in lib.oiva_last_error()
        with pytest.raises(ValueError, match="complex128"):
            plan.ip2_iterate(0, 1)
    with oa.BatchPlan(1, 20, 5, 3, 2) as plan:
        assert lib.oiva_batch_ip2_stage(plan.h, 0, 0) == _lib.ERR_STATE            # X not set
        plan.set_x(X)
        assert lib.oiva_batch_ip2_stage(plan.h, 0, 0) == _lib.ERR_STATE            # no covariance
        plan.covariance()
        assert lib.oiva_batch_ip2_stage(plan.h, 3, 0) == _lib.ERR_STATE            # no W
        assert lib.oiva_batch_ip2_iterate(plan.h, 0, 1) == _lib.ERR_STATE
        with pytest.raises(RuntimeError):
            plan.ip2_iterate(0, 1)
        plan.set_w(None)
        assert lib.oiva_batch_ip2_stage(plan.h, 4, 0) == _lib.ERR_ARG
        assert lib.oiva_batch_ip2_stage(plan.h, -1, 0) == _lib.ERR_ARG
        assert lib.oiva_batch_ip2_stage(plan.h, 0, -1) == _lib.ERR_ARG
        assert lib.oiva_batch_ip2_iterate(plan.h, -1, 1) == _lib.ERR_ARG
        assert lib.oiva_batch_ip2_iterate(plan.h, 0, -1) == _lib.ERR_ARG
        assert lib.oiva_batch_ip2_time_stages(plan.h, 0, ms) == _lib.ERR_ARG
        plan.ip2_iterate(0, 1)
        t = plan.ip2_time_stages(1)
        assert set(t) == {"power", "activation", "cov", "update"} and all(v > 0 for v in t.values())
        assert np.all(np.isfinite(plan.get_w()))
        # a new X of the same plan: the next iteration streams it
        X2 = cases.make_x("iid", 20, 5, 3, 3, seed=3)[None]
        plan.set_x(X2)
        plan.covariance()
        plan.set_w(None)
        plan.ip2_iterate(0, 2)
        assert np.array_equal(plan.get_w(np.complex128), run_device(X2, 2, 2))
