"""ilrma_batch() / ilrma() on the GPU: every stage against the NumPy restatement (tests/helpers/ilrma_oracle.py)
from a known state, the floors, iterated results where the restatement is itself reproducible, a degenerate room, the cost along
the device path, bits that do not depend on the batch, and the public call.

Figures measured on an MI355X (printed by the tests before they assert):
  stages: P, R, Tn, Vn, C, lambda and the normalised state within 3.1e-15 of NumPy at the first four shapes, within 3.6e-15 at the
  seven with L = 4, 5, 8, 9, 16 and M = 1, 6, 7 (worst: R normalised at (1, 100, 33, 7, 8)) (bound 1e-12);
  |w_s^H C_s w_s - 1| <= 2.2e-13 and |w_j^H C_s w_s| <= 3.7e-14 after the per-bin step, 3.0e-14 and 2.3e-14 at the seven (bound 1e-10);
  floors: Tn, Vn and R within 3.8e-16 at L = 2 and within 2.5e-16 at L = 9 with both floored entries in component 8;
  iterated: device W within 5.6e-16 .. 6.5e-14 of the oracle's against 10 delta = 1.6e-13 .. 2.8e-12; at the shapes with L = 4 .. 16
  6.8e-17 .. 8.0e-14 against 10 delta = 1.1e-13 .. 3.4e-12, Tn @ Vn 1.1e-16 .. 1.4e-14 against 10 delta_R = 2.1e-13 .. 1.7e-12
  (DESIGN.md 3.9 has the table);
  cost over 20 epochs stage by stage: largest relative rise 1.1e-15, largest move in step 4 1.3e-15 (bound 1e-12).
"""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

import ilrma_cases as cases  # noqa: E402
import ilrma_oracle as ilo  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-12        # the bound test_weighted_covariance holds `precise` to
TOL_W = 1e-10      # defining properties of the per-bin step


def dist(a, b):
    """maximum absolute difference over the maximum magnitude"""
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def rooms(kind, B, T, F, M, seed=cases.SEED):
    return np.stack([cases.make_x(kind, T, F, M, seed=seed + b) for b in range(B)])


def random_w0(B, F, M, seed):
    """well conditioned: the identity plus a small complex perturbation"""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((B, F, M, M)) + 1j * rng.standard_normal((B, F, M, M))
    return np.eye(M)[None, None] + 0.3 / np.sqrt(M) * g


def open_plan(X, W0, T0, V0):
    """a BatchPlan with ILRMA begun on X (B, T, F, M)"""
    from overiva_amd import BatchPlan

    B, T, F, M = X.shape
    plan = BatchPlan(B, T, F, M, M)
    plan.set_x(X)
    plan.covariance()
    plan.set_w(W0)
    plan.ilrma_begin(T0, V0)
    return plan


def unpack_herm(Cp, M):
    """(..., M*M) packed Hermitian (M real diagonals, then (re, im) of every c < d, row-major) -> (..., M, M) complex"""
    C = np.zeros(Cp.shape[:-1] + (M, M), np.complex128)
    a = M
    for c in range(M):
        C[..., c, c] = Cp[..., c]
        for d in range(c + 1, M):
            C[..., c, d] = Cp[..., a] + 1j * Cp[..., a + 1]
            C[..., d, c] = Cp[..., a] - 1j * Cp[..., a + 1]
            a += 2
    return C


def run_device(X, n, T0, V0, W0=None):
    """n epochs through the plan: (W complex128, Tn, Vn, Y complex64 without projection back)"""
    with open_plan(X, W0, T0, V0) as plan:
        plan.ilrma_iterate(n)
        Tn, Vn = plan.get_nmf()
        return plan.get_w(np.complex128), Tn, Vn, plan.demix(False)


# ---- 1. stages against NumPy -------------------------------------------------------------------------------------------------
# (B, T, F, M, L).  The kernels of the T, V and R updates are instantiated for L rounded up to LP = 1, 2, 4, 8, 16, the power and
# covariance kernels per channel count: the second row of shapes runs LP = 8 and 16 with L below and at LP, L = LP = 4, and M = 1, 6, 7
STAGE_SHAPES = [(3, 70, 17, 2, 2), (2, 33, 65, 3, 3), (2, 257, 20, 8, 2), (1, 70, 17, 5, 1),
                (2, 70, 17, 6, 5), (1, 100, 33, 7, 8), (1, 130, 17, 3, 9), (2, 64, 16, 2, 16), (1, 128, 64, 2, 16), (1, 70, 17, 4, 4),
                (1, 70, 5, 1, 4)]


@pytest.mark.parametrize("shape", STAGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stages_against_numpy(shape):
    """a ragged 16-bin group and a ragged 64-bin chunk, a chunk of frames plus a tail, two covariance splits at T = 257, odd and
    full channel counts, L = 1 and 3; then L = 5 and 8 (LP = 8) at 6 and 7 channels, 33 bins being two 16-bin groups and one bin;
    L = 9 and 16 (LP = 16) with T two lane strides plus 2, exactly one and exactly two, F exactly one 16-bin group and exactly
    one 64-bin chunk; L = LP = 4; one channel"""
    B, T, F, M, L = shape
    X = rooms("mix", B, T, F, M)
    W0 = random_w0(B, F, M, seed=3)
    T0, V0 = cases.make_nmf(T, F, M, L, B=B)
    seen = {}

    def check(name, dev, ref):
        seen[name] = max(seen.get(name, 0.0), dist(dev, ref))

    with open_plan(X, W0, T0, V0) as plan:
        st = [ilo.start(X[b], T0[b], V0[b], W0[b]) for b in range(B)]      # (X128, W, Tn, Vn, R, P) per room
        Xs, W, Tn, Vn, R, P = (np.stack([s[i] for s in st]) for i in range(6))
        dP, dR = plan.get_pr()
        check("P begin", dP, P)
        check("R begin", dR, R)

        plan.ilrma_stage("t_update")
        for b in range(B):
            for s in range(M):
                ilo.update_t(P[b], R[b], Tn[b], Vn[b], s)
        check("Tn", plan.get_nmf()[0], Tn)
        check("R after T", plan.get_pr()[1], R)

        plan.ilrma_stage("v_update")
        for b in range(B):
            for s in range(M):
                ilo.update_v(P[b], R[b], Tn[b], Vn[b], s)
        check("Vn", plan.get_nmf()[1], Vn)
        check("R untouched by V", plan.get_pr()[1], R)

        plan.ilrma_stage("r_rewrite")
        for b in range(B):
            for s in range(M):
                ilo.rewrite_r(R[b], Tn[b], Vn[b], s)
        check("R rewrite", plan.get_pr()[1], R)

        plan.ilrma_stage("weighted_cov")
        C = np.stack([np.stack([ilo.weighted_cov(Xs[b], R[b], s) for s in range(M)]) for b in range(B)])      # (B, K, F, M, M)
        Cp, _ = plan.get_ilrma_cov()
        dC = np.transpose(unpack_herm(Cp, M), (0, 2, 1, 3, 4)) / T
        check("C", dC, C)

        plan.ilrma_stage("ip_update")
        Wn = plan.get_w(np.complex128)
        assert np.all(np.isfinite(Wn))
        assert np.array_equal(plan.get_pr()[0], dP)           # P is not refreshed inside an epoch
        worst_unit = worst_orth = 0.0
        for s in range(M):
            ws = Wn[..., s]                                                           # (B, F, M)
            Cw = np.einsum("bfcd,bfd->bfc", C[:, s], ws)
            worst_unit = max(worst_unit, float(np.max(np.abs(np.einsum("bfc,bfc->bf", np.conj(ws), Cw) - 1.0))))
            for j in range(M):
                if j != s:
                    wj = Wn[..., j] if j < s else W[..., j]                           # later columns as they were before the step
                    worst_orth = max(worst_orth, float(np.max(np.abs(np.einsum("bfc,bfc->bf", np.conj(wj), Cw)))))
        seen["|w^H C w - 1|"], seen["|w_j^H C w|"] = worst_unit, worst_orth

        plan.ilrma_stage("power")
        Pn = np.stack([ilo.power(Xs[b], Wn[b]) for b in range(B)])
        check("P", plan.get_pr()[0], Pn)

        plan.ilrma_stage("normalise")
        Wref = Wn.copy()
        lam = np.empty((B, M))
        for b in range(B):
            Pn[b], lam[b] = ilo.normalise(Xs[b], Wref[b], Tn[b], R[b])
        dP, dR = plan.get_pr()
        check("lambda", plan.get_ilrma_cov()[1], lam)
        check("W normalised", plan.get_w(np.complex128), Wref)
        check("P normalised", dP, Pn)
        check("R normalised", dR, R)
        check("Tn normalised", plan.get_nmf()[0], Tn)
        check("Vn kept", plan.get_nmf()[1], Vn)
    print(f"ilrma stages {shape}: " + ", ".join(f"{k} {v:.2e}" for k, v in seen.items()))
    for name, v in seen.items():
        assert v <= (TOL_W if name.startswith("|w") else TOL), (name, v)


# ---- 2. floors -----------------------------------------------------------------------------------------------------------------
def test_floors():
    """one entry of T0 and one of V0 small enough to fall below eps in the first update: both come back as exactly eps, and R
    follows.  At L = 9 both sit in component 8, the upper half of the 16 the kernels are instantiated for."""
    _floors(2, 0, 1)
    _floors(9, 8, 8)


def _floors(L, lt, lv):
    B, T, F, M = 1, 70, 17, 2
    X = rooms("iid", B, T, F, M)
    T0, V0 = cases.make_nmf(T, F, M, L, B=B)
    T0[0, 1, 5, lt] = 1e-20
    V0[0, 0, lv, 33] = 1e-20
    with open_plan(X, None, T0, V0) as plan:
        _, W, Tn, Vn, R, P = ilo.start(X[0], T0[0], V0[0])
        plan.ilrma_stage("t_update")
        plan.ilrma_stage("v_update")
        plan.ilrma_stage("r_rewrite")
        for s in range(M):
            ilo.update_t(P, R, Tn, Vn, s)
            ilo.update_v(P, R, Tn, Vn, s)
            ilo.rewrite_r(R, Tn, Vn, s)
        dT, dV = plan.get_nmf()
        dR = plan.get_pr()[1]
    assert Tn[1, 5, lt] == ilo.EPS and Vn[0, lv, 33] == ilo.EPS          # the oracle floors them
    assert dT[0, 1, 5, lt] == ilo.EPS and dV[0, 0, lv, 33] == ilo.EPS
    assert (dT[0] == ilo.EPS).sum() == 1 and (dV[0] == ilo.EPS).sum() == 1 and dT.min() == ilo.EPS and dV.min() == ilo.EPS
    print(f"ilrma floors L={L}: Tn {dist(dT[0], Tn):.2e}, Vn {dist(dV[0], Vn):.2e}, R {dist(dR[0], R):.2e}, "
          f"R row {dist(dR[0, 1, 5], R[1, 5]):.2e}, R column {dist(dR[0, 0, :, 33], R[0, :, 33]):.2e}")
    assert dist(dT[0], Tn) <= TOL and dist(dV[0], Vn) <= TOL and dist(dR[0], R) <= TOL
    assert dist(dR[0, 1, 5], R[1, 5]) <= TOL and dist(dR[0, 0, :, 33], R[0, :, 33]) <= TOL


# ---- 3. iterated parity, where the oracle is reproducible ----------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.ITERATED, ids=cases.case_id)
def test_iterated_parity(case):
    """delta: how far a 1e-13 relative perturbation of X moves the oracle's own W (delta_R: its Tn @ Vn).  The device, whose sums
    round in another order, must stay within 10 delta and 10 delta_R."""
    o = cases.oracle_run(case)
    assert 10 * o["delta"] <= 1e-8, o["delta"]           # the case is one where the oracle itself is reproducible
    W, Tn, Vn, _ = run_device(o["X"][None], case[2], o["T0"], o["V0"])
    dW, dR = cases.rel(W[0], o["W"]), cases.rel(Tn[0] @ Vn[0], o["Tn"] @ o["Vn"])
    print(f"ilrma iterated {cases.case_id(case)}: delta {o['delta']:.2e} device W {dW:.2e}; delta_R {o['delta_R']:.2e} device R {dR:.2e}")
    assert dW <= 10 * o["delta"] and dR <= 10 * o["delta_R"]


# ---- 4. a degenerate room ------------------------------------------------------------------------------------------------------
def test_degenerate_room_is_named_and_leaves_the_others_alone():
    """an all-zero room: P = 0 sends Tn and Vn to the floor and C_s is singular (no small seed of a 33-frame mixture drove the
    oracle non-finite on the CPU, so the room is zeros).  The call names it, status() flags it alone, and the other rooms have the
    bits of a batch without it."""
    import overiva_amd as oa

    B, T, F, M, L = 3, 70, 17, 2, 2
    X = rooms("mix", B, T, F, M)
    X[1] = 0
    T0, V0 = cases.make_nmf(T, F, M, L, B=B)
    with pytest.raises(np.linalg.LinAlgError, match=r"problem\(s\) 1$"):
        oa.ilrma_batch(X, n_iter=3, T0=T0, V0=V0)
    with open_plan(X, None, T0, V0) as plan:
        plan.ilrma_iterate(3)
        assert plan.status().tolist() == [False, True, False]
        W = plan.get_w(np.complex128, check=False)
    keep = [0, 2]
    Wk, _, _, _ = run_device(X[keep], 3, T0[keep], V0[keep])
    assert np.all(np.isfinite(Wk)) and np.array_equal(W[keep], Wk)


# ---- 5. the cost along the device path ---------------------------------------------------------------------------------------
def test_cost_is_monotone_on_the_device_path():
    """20 epochs stage by stage; Q in NumPy from get_w and get_nmf after every step 1, 3 and 4: no step raises it by more than
    1e-12 relative and step 4 moves it by at most that either way"""
    B, T, F, M, L = 2, 70, 17, 4, 2
    X = rooms("mix", B, T, F, M)
    X128 = X.astype(np.complex128)
    T0, V0 = cases.make_nmf(T, F, M, L, B=B)

    def cost(plan):
        W = plan.get_w(np.complex128)
        Tn, Vn = plan.get_nmf()
        return np.array([ilo.cost(ilo.power(X128[b], W[b]), Tn[b] @ Vn[b], W[b]) for b in range(B)])

    rise = move4 = -np.inf
    with open_plan(X, None, T0, V0) as plan:
        q = first = cost(plan)
        for _ in range(20):
            for step, stages in ((1, ("t_update", "v_update", "r_rewrite")), (3, ("weighted_cov", "ip_update")),
                                 (4, ("power", "normalise"))):
                for s in stages:
                    plan.ilrma_stage(s)
                q, before = cost(plan), q
                change = (q - before) / np.abs(before)
                rise = max(rise, float(change.max()))
                if step == 4:
                    move4 = max(move4, float(np.abs(change).max()))
    print(f"ilrma cost: largest relative rise {rise:.2e}, largest move in step 4 {move4:.2e}, Q {first} -> {q}")
    assert np.all(np.isfinite(q)) and np.all(q < first)
    assert rise <= 1e-12 and move4 <= 1e-12


# ---- 6. bits do not depend on the batch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F, M, L", [(17, 3, 2), (65, 3, 2), (17, 3, 9)], ids=["17", "65", "17-L9"])
def test_bits_do_not_depend_on_the_batch(F, M, L):
    B, T = 5, 70
    X = rooms("mix", B, T, F, M)
    T0, V0 = cases.make_nmf(T, F, M, L, B=B)
    full = run_device(X, 5, T0, V0)
    perm = [3, 0, 4, 2, 1]
    shuffled = run_device(X[perm], 5, T0[perm], V0[perm])
    for b in range(B):
        alone = run_device(X[b:b + 1], 5, T0[b:b + 1], V0[b:b + 1])
        for name, a, f, p in zip(("W", "Tn", "Vn", "Y"), alone, full, shuffled):
            assert np.all(np.isfinite(a)), name
            assert np.array_equal(a[0], f[b]), (name, b)
            assert np.array_equal(a[0], p[perm.index(b)]), (name, b)


# ---- 7. the public call --------------------------------------------------------------------------------------------------------
def test_ilrma_is_ilrma_batch_of_one_room():
    import overiva_amd as oa

    T, F, M, L = 70, 17, 3, 2
    X = cases.make_x("mix", T, F, M)
    one = oa.ilrma(X, n_iter=4, n_components=L, seed=5, return_filters=True, return_nmf=True)
    bat = oa.ilrma_batch(X[None], n_iter=4, n_components=L, seed=5, return_filters=True, return_nmf=True)
    assert one[0].shape == (T, F, M) and one[0].dtype == np.complex64 and one[1].shape == (F, M, M)
    assert one[2][0].shape == (M, F, L) and one[2][1].shape == (M, L, T)
    assert np.array_equal(one[0], bat[0][0]) and np.array_equal(one[1], bat[1][0])
    assert np.array_equal(one[2][0], bat[2][0][0]) and np.array_equal(one[2][1], bat[2][1][0])
    assert np.array_equal(oa.ilrma(X, n_iter=4, n_components=L, seed=5), one[0])          # Y alone
    # the default start is the documented recipe
    T0, V0 = cases.make_nmf(T, F, M, L, seed=5)
    assert np.array_equal(oa.ilrma(X, n_iter=4, n_components=L, T0=T0[0], V0=V0[0]), one[0])
    info = oa.last_batch_info()
    assert info["algorithm"] == "ilrma" and info["n_components"] == L and info["batched"] == 1
    assert info["precision"] == "precise" and info["shape"] == (T, F, M, M)


def test_callback_epochs():
    import overiva_amd as oa

    B, T, F, M = 2, 70, 17, 2
    X = rooms("iid", B, T, F, M)
    got = []
    Y = oa.ilrma_batch(X, n_iter=12, seed=1, callback=lambda Y: got.append(Y.copy()))
    assert len(got) == 2 and all(g.shape == (B, T, F, M) for g in got)          # epochs 0 and 10
    assert np.array_equal(got[0], oa.ilrma_batch(X, n_iter=0, seed=1))
    assert np.array_equal(got[1], oa.ilrma_batch(X, n_iter=10, seed=1))
    assert np.array_equal(Y, oa.ilrma_batch(X, n_iter=12, seed=1))              # the callback does not change the result


def test_projection_back_is_the_batch_s_own():
    import overiva_amd as oa

    B, T, F, M = 2, 70, 17, 3
    X = rooms("mix", B, T, F, M).astype(np.complex128)          # complex128 in: W comes back in complex128
    Y0, W = oa.ilrma_batch(X, n_iter=3, seed=2, proj_back=False, return_filters=True)
    Y1 = oa.ilrma_batch(X, n_iter=3, seed=2, proj_back=True)
    assert Y0.dtype == Y1.dtype == W.dtype == np.complex128
    with oa.BatchPlan(B, T, F, M, M) as plan:
        plan.set_x(X)
        plan.covariance()
        plan.set_w(W)
        assert np.array_equal(plan.demix(False, np.complex128), Y0)
        assert np.array_equal(plan.demix(True, np.complex128), Y1)
    assert not np.array_equal(Y0, Y1)
    # complex128 input is converted on the device: the same bits as its complex64 rounding gives
    assert np.array_equal(oa.ilrma_batch(X.astype(np.complex64), n_iter=3, seed=2), Y1.astype(np.complex64))


def test_ragged_plan_refuses():
    import overiva_amd as oa
    from overiva_amd import _lib

    with oa.RaggedBatchPlan([20, 16], 5, 2, 2) as plan:
        with pytest.raises(ValueError, match="ragged"):
            plan.ilrma_begin(np.ones((2, 2, 5, 2)), np.ones((2, 2, 2, 20)))
        with pytest.raises(ValueError, match="ragged"):
            plan.ilrma_iterate(1)
        T0, V0 = np.ones((2, 2, 5, 2)), np.ones((2, 2, 2, 20))
        lib = _lib.load()
        assert lib.oiva_batch_ilrma_begin(plan.h, 2, _lib.ptr(T0), _lib.ptr(V0)) == _lib.ERR_ARG
        assert b"ragged" in lib.oiva_last_error()
        assert lib.oiva_batch_ilrma_iterate(plan.h, 1) == _lib.ERR_ARG and b"ragged" in lib.oiva_last_error()
        assert lib.oiva_batch_ilrma_stage(plan.h, 0) == _lib.ERR_ARG and b"ragged" in lib.oiva_last_error()
        out = (ctypes.c_double * 400)()
        assert lib.oiva_batch_ilrma_get_nmf(plan.h, out, None) == _lib.ERR_ARG and b"ragged" in lib.oiva_last_error()


def test_begin_refusals_of_the_c_entry():
    """what oiva_batch_ilrma_begin itself refuses on a dense batch: K != M, a component count outside 1..16, a T0 that is not
    strictly positive, and the stages before begin"""
    import overiva_amd as oa
    from overiva_amd import _lib

    lib = _lib.load()
    X = rooms("iid", 1, 20, 5, 3)
    with oa.BatchPlan(1, 20, 5, 3, 2) as plan:
        plan.set_x(X)
        plan.covariance()
        plan.set_w(None)
        with pytest.raises(ValueError, match="K = M"):
            plan.ilrma_begin(np.ones((1, 2, 5, 2)), np.ones((1, 2, 2, 20)))
    with oa.BatchPlan(1, 20, 5, 3, 3) as plan:
        plan.set_x(X)
        plan.covariance()
        plan.set_w(None)
        with pytest.raises(RuntimeError, match="ilrma_begin"):
            plan.ilrma_iterate(1)
        with pytest.raises(ValueError, match="1..16"):
            plan.ilrma_begin(np.ones((1, 3, 5, 17)), np.ones((1, 3, 17, 20)))
        bad = np.ones((1, 3, 5, 2))
        bad[0, 2, 4, 1] = 0.0
        with pytest.raises(ValueError, match="positive"):
            plan.ilrma_begin(bad, np.ones((1, 3, 2, 20)))
        assert lib.oiva_batch_ilrma_stage(plan.h, 0) == _lib.ERR_STATE
        plan.ilrma_begin(np.ones((1, 3, 5, 2)), np.ones((1, 3, 2, 20)))
        assert lib.oiva_batch_ilrma_stage(plan.h, 7) == _lib.ERR_ARG
        plan.ilrma_iterate(1)
        assert np.all(np.isfinite(plan.get_w()))
