"""Parity of the HIP path (through the C ABI, ctypes) against the oracle and the committed golden
vectors of the real reference.  Needs an MI355X: run with ``-m gpu``.

Tolerances.  BASELINE.json's north_star asks for 1e-5 relative (fp32) on demixed Y and final W for identical
STFT input; the distance is ||a-b||_F / ||b||_F.

* Default arithmetic (``auto``).  The reference computes in the dtype of X (overiva.py:89,126,131), and so does the default:
  - complex128 input (``precise``: float64 covariance accumulation and per-bin algebra on complex64-rounded data), against
    the reference's complex128 result: ``1e-5``, scaled by ``amp / 10`` only where the reference itself amplifies rounding
    by more than 10 (fixture key ``amp_*`` = measured amplification of a relative input perturbation in the reference,
    tests/golden/make_golden.py); where it is chaotic (amp > 1e3, conftest.chaotic) no value is compared, the run must give
    the same bits twice (_same_twice);
  - complex64 input: on frame axes up to 256 long with up to 8 channels ``auto`` runs ``precise`` too (round 6: the reference
    forms those covariances in complex128 as well, overiva.py:179), except where the X-resident kernel keeps ``mixed`` (2, 6, 8
    channels with 1-2 sources); elsewhere ``mixed`` (float32 products and lane chains, float64 sums and per-bin algebra) --
    against the reference's OWN complex64 result (``W_c64_*``): ``max(1e-5, 1.5 * floor)`` with floor = distance between
    the reference's complex64 and complex128 results -- the parity claim -- and against the complex128 result
    ``max(that bound, floor)``: never less accurate than the reference's own complex64 arithmetic (achieved: 0.1-0.9
    floors).  On the four rows where the reference's own complex64 run is not reproducible to 1e-3 under a last-bit change
    of X (conftest.c64_diverged, measured on the real reference: tests/golden/c64_jitter.npz) "floor" is replaced by that
    jitter where it is larger -- see test_overiva_matches_reference.  (Round 5's one exception -- fixture z, i.i.d., gauss, 20
    iterations, 1.7 floors in ``mixed`` -- runs the float64 covariance now and needs none.)
* ``fast`` arithmetic (float32 per-bin algebra too): 1e-5 on well-conditioned (i.i.d.) input; on mixture-like input a
  documented envelope of FAST_FLOORS reference floors -- an accuracy statement of that mode, not the parity claim.

Every end-to-end comparison appends a row to $OIVA_PARITY_LOG (JSON lines) when that variable is set;
profiles/rNN_parity_errors.md is made from it (tools/parity_table.py).
"""
import json
import os

import numpy as np
import pytest

from conftest import c64_diverged, c64_jitter, chaotic, golden_files, golden_ids, need
from oracle import overiva_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-5          # the north_star bound
TOL_KERNEL = 3e-6   # single-kernel bound (one fp32 pass, no iteration feedback)
# rows of pure amplified rounding noise where `mixed` lands MORE than one floor from the reference's complex128 result (see
# test_overiva_matches_reference): each entry is a measured, documented exception, not a class
TOL_KERNEL_F64 = 1e-12   # float64 accumulation of exact float32 products
FAST_FLOORS = 6.0   # envelope of the float32 mode on ill-conditioned input, in reference-complex64 floors


def _amp(g, model, n_iter):
    return max(1.0, float(g.get(f"amp_{model}_{n_iter}", 1.0)))


def _bound128(g, model, n_iter):
    """bound against the reference's complex128 result: the north-star 1e-5, scaled only for amp > 10"""
    return TOL * max(1.0, _amp(g, model, n_iter) / 10.0)


def _log(**row):
    path = os.environ.get("OIVA_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(row) + "\n")


def _same_twice(run):
    """where the reference itself is chaotic (conftest.chaotic) or its own complex64 arithmetic is, no value can be pinned on
    the result.  What still holds there: the GPU path is deterministic -- the same call twice returns the same bits, all
    finite (or raises the same LinAlgError twice: a singular solve, as numpy.linalg.solve raises in the reference).
    Returns the arrays of the first call, or None when it raised."""
    outs = []
    for _ in range(2):
        try:
            outs.append(tuple(np.array(a) for a in run()))
        except np.linalg.LinAlgError:
            outs.append(None)
    a, b = outs
    assert (a is None) == (b is None), "one call raised LinAlgError and the other did not"
    if a is not None:
        assert all(np.all(np.isfinite(x)) for x in a)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    return a


def _c64_floor(fn_ref64, ref128):
    """distance of the reference algorithm's OWN complex64 arithmetic (oracle, reference-faithful
    mode) from its complex128 result on the same input"""
    try:
        with np.errstate(all="ignore"):
            e = orc.rel_err(fn_ref64(), ref128)
    except np.linalg.LinAlgError:
        return np.inf
    return e if np.isfinite(e) else np.inf


@pytest.fixture
def fast_mode(oa):
    oa.set_precision("fast")
    yield
    oa.set_precision("auto")


@pytest.fixture(scope="module")
def oa():
    import overiva_amd
    from overiva_amd import _lib

    _lib.load()
    return overiva_amd


def _plan(oa, X, K, model="laplace", mode="fast"):
    T, F, M = X.shape
    p = oa.Plan(T, F, M, K, model)
    p.set_precision(mode)
    p.set_x(X)
    p.covariance()
    return p


# --------------------------------------------------------------------------------------------
# per-kernel parity
# --------------------------------------------------------------------------------------------
def test_input_covariance(oa, golden):
    X, K = golden["X"], int(golden["K"])
    with _plan(oa, X, K) as p:
        Cx = p.get_cx()
    ref = orc.input_covariance(X.astype(np.complex128))
    assert orc.rel_err(Cx, ref) < TOL_KERNEL


@pytest.mark.parametrize("mode", ["fast", "precise"])
@pytest.mark.parametrize("splits", [0, 1, 3])
def test_weighted_covariance(oa, golden, splits, mode):
    X, K = golden["X"], int(golden["K"])
    T = X.shape[0]
    rng = np.random.default_rng(5)
    rinv = rng.gamma(2.0, 1.0, (T, K)).astype(np.float32)
    with _plan(oa, X, K, mode=mode) as p:
        if splits:
            p.set_cov_splits(splits)
        p.t_set_rinv(rinv)
        p.t_run_weighted_cov()
        V = p.t_get_v(np.complex128)
    # the device divides 1 by the float32 reciprocal it is handed: compare with exactly those weights
    w = 1.0 / (np.float32(1) / rinv).astype(np.float64) if mode == "precise" else rinv.astype(np.float64)
    ref = orc.weighted_cov_all(X, w)
    assert V.shape == ref.shape
    e = orc.rel_err(V, ref)
    print(f"\n[parity] {golden['_id']} weighted covariance {mode} splits={splits}: {e:.2e}")
    # (more than 8 channels: the planar kernel takes its weights from a float32 table, 6e-8 each)
    tol64 = TOL_KERNEL_F64 if X.shape[2] <= 8 else 2e-7
    assert e < (tol64 if mode == "precise" else TOL_KERNEL)
    # Hermitian by construction
    assert np.array_equal(V, np.conj(np.swapaxes(V, -1, -2)))


@pytest.mark.parametrize("shape", [(1024, 6, 8, 2), (1024, 5, 5, 5), (1024, 4, 7, 3), (1024, 3, 8, 4), (1024, 3, 4, 2), (1024, 2, 12, 3)],
                         ids=lambda s: "x".join(str(v) for v in s))
def test_update_adds_any_number_of_frame_splits(oa, shape):
    """the per-bin update kernels add the frame splits' partial covariances in batches of 2, 4, 8 or 16 loads that follow the number
    of splits (csrc/oiva_internal.h::sum_vpart, round 5; more than 16: several rounds): every batch size and the multi-round case,
    two iterations from the identity against the oracle (overiva.py:176-190) -- update_bg (8 / 2, 4 / 2), update_det (5 / 5),
    update_gram (7 / 3, 8 / 4), one wavefront per bin (12 / 3)"""
    T, F, M, K = shape
    X = orc.synth_iid(T, F, M, seed=41)
    _, Wref = orc.overiva_faithful(X.astype(np.complex128), n_src=K, n_iter=2, proj_back=False, model="laplace", return_filters=True)
    seen = set()
    for splits in (1, 2, 3, 4, 6, 8, 12, 16, 22, 32):
        with oa.Plan(T, F, M, K, "laplace") as p:
            p.set_precision("mixed")
            p.set_resident(False)
            p.set_cov_splits(splits)
            p.set_x(X)
            p.covariance()
            p.set_w(None)
            p.iterate(2)
            W = p.get_w()
            got = p.cov_splits()
        seen.add(0 if got <= 2 else 1 if got <= 4 else 2 if got <= 8 else 3 if got <= 16 else 4)
        assert orc.rel_err(W, Wref) < 3e-6, (splits, got)
    assert seen == {0, 1, 2, 3, 4} or M > 8, seen      # (every batch size and more than one round of 16; 9..16 channels: own loader)


def test_demix_power(oa, golden):
    X, K = golden["X"], int(golden["K"])
    T, F, M = X.shape
    rng = np.random.default_rng(6)
    What = (rng.standard_normal((F, M, M)) + 1j * rng.standard_normal((F, M, M))).astype(np.complex64)
    with _plan(oa, X, K) as p:
        p.t_set_what(What)
        pw = p.t_run_power()
    ref = orc.demix_power(X, What[:, :, :K])
    assert orc.rel_err(pw, ref) < TOL_KERNEL


@pytest.mark.parametrize("before_covariance", [False, True], ids=["padded-copy", "caller-X"])
@pytest.mark.parametrize("shape", [(70, 5, 10, 10), (33, 3, 14, 9), (50, 70, 9, 9), (64, 65, 13, 6), (40, 2, 15, 15), (40, 7, 11, 11),
                                   (100, 9, 12, 5), (17, 1, 16, 16), (65, 64, 10, 5)], ids=lambda s: "x".join(str(v) for v in s))
def test_power_pass_of_many_sources_at_every_channel_count(oa, shape, before_covariance):
    """the matrix-core power pass (9..16 channels, more than 4 sources; overiva.py:140 + :153): 16-byte loads at every even
    channel pitch (10 and 14 channels: the last channel quarter holds two), odd channel counts on the plan's zero-padded copy
    of X once oiva_plan_covariance has filled it and on the caller's X before; ragged bins, frames and sources"""
    T, F, M, K = shape
    X = orc.synth_iid(T, F, M, seed=3)
    rng = np.random.default_rng(6)
    What = (rng.standard_normal((F, M, M)) + 1j * rng.standard_normal((F, M, M))).astype(np.complex64)
    with oa.Plan(T, F, M, K, "laplace") as p:
        p.set_x(X)
        if not before_covariance:
            p.covariance()
        p.t_set_what(What)
        pw = p.t_run_power()
    assert orc.rel_err(pw, orc.demix_power(X, What[:, :, :K])) < TOL_KERNEL


@pytest.mark.parametrize("shape", [(100, 64, 16, 16), (64, 128, 16, 9), (37, 64, 16, 5), (16, 64, 16, 16), (1000, 192, 16, 13), (129, 64, 16, 8)],
                         ids=lambda s: "x".join(str(v) for v in s))
def test_power_pass_through_lds_at_16_channels(oa, shape):
    """power_lds_kernel (16 channels, more than 4 sources, at least 64 bins; overiva.py:140 + :153): X in 2 KB runs through
    LDS to the matrix cores -- frame counts that are no multiple of the 64 frames of a workgroup or the 16 of a tile, every
    source count, several batches, whole batches (F bins) and a ragged last batch of ONE bin (F + 1 bins: its one sub-batch
    starts at bin F - 15 and the bins it then holds twice meet a zero in W); against the oracle, and the two against each
    other through the last bin's own contribution"""
    T, F, M, K = shape
    X = orc.synth_iid(T, F + 1, M, seed=3)
    rng = np.random.default_rng(6)
    What = (rng.standard_normal((F + 1, M, M)) + 1j * rng.standard_normal((F + 1, M, M))).astype(np.complex64)
    with oa.Plan(T, F, M, K, "laplace") as p:
        p.set_x(np.ascontiguousarray(X[:, :F]))
        p.covariance()
        p.t_set_what(What[:F])
        pw = p.t_run_power()
    assert orc.rel_err(pw, orc.demix_power(X[:, :F], What[:F, :, :K])) < TOL_KERNEL
    with oa.Plan(T, F + 1, M, K, "laplace") as p:
        p.set_x(X)
        p.covariance()
        p.t_set_what(What)
        pw1 = p.t_run_power()
    ref1 = orc.demix_power(X, What[:, :, :K])
    assert orc.rel_err(pw1, ref1) < TOL_KERNEL
    # the last bin's own contribution, from the oracle, takes one result to the other
    last = orc.demix_power(X[:, F:], What[F:, :, :K])
    assert orc.rel_err(pw1 - last, pw) < 2 * TOL_KERNEL


@pytest.mark.parametrize("shape", [(70, 65, 16, 16), (33, 79, 16, 7), (50, 80, 16, 16), (40, 111, 16, 9), (64, 127, 16, 16), (20, 190, 16, 12), (48, 63, 16, 16), (48, 17, 16, 6)],
                         ids=lambda s: "x".join(str(v) for v in s))
def test_power_pass_ragged_last_batch_at_16_channels(oa, shape):
    """a last batch of 1, 15, 16, 47, 63 bins (and two batches + 62) through power_lds_kernel -- sub-batches that are whole,
    cut, or past the last bin; fewer than 64 bins: the frame-major kernel (power_mfma_kernel) -- each bin's power with the
    other bins' W set to zero must be that bin's alone: a bin counted twice or not at all shows as a factor, not as rounding
    (overiva.py:140 + :153)"""
    T, F, M, K = shape
    X = orc.synth_iid(T, F, M, seed=5)
    rng = np.random.default_rng(8)
    What = (rng.standard_normal((F, M, M)) + 1j * rng.standard_normal((F, M, M))).astype(np.complex64)
    with oa.Plan(T, F, M, K, "laplace") as p:
        p.set_x(X)
        p.covariance()
        p.t_set_what(What)
        pw = p.t_run_power()
        assert orc.rel_err(pw, orc.demix_power(X, What[:, :, :K])) < TOL_KERNEL
        for f in sorted({0, 15, 16, F - 17, F - 16, F - 15, F - 2, F - 1, (F // 64) * 64, (F // 64) * 64 - 1} & set(range(F))):
            W1 = np.zeros_like(What)
            W1[f] = What[f]
            p.t_set_what(W1)
            one = p.t_run_power()
            assert orc.rel_err(one, orc.demix_power(X[:, f:f + 1], What[f:f + 1, :, :K])) < TOL_KERNEL, f


@pytest.mark.needs("im_{model}_e0_s0_V")
@pytest.mark.parametrize("rows", [False, True], ids=["lane-per-element", "lane-per-row"])
@pytest.mark.parametrize("fp64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("model", ["laplace", "gauss"])
def test_ip_update(oa, golden, model, fp64, rows):
    """weighted covariance + per-bin chain (IP1 solve, normalisation, J) from the reference's own
    traced state at overiva.py:181 (W_hat after gamma scaling, r_inv) -> W_hat after the epoch."""
    X, K = golden["X"], int(golden["K"])
    T, F, M = X.shape
    for e in (0, 1):
        rinv = golden[f"im_{model}_e{e}_s0_rinv"]
        W_in = golden[f"im_{model}_e{e}_s0_What"]
        with _plan(oa, X, K, model) as p:
            p.set_precision(1 if fp64 else 0, row_layout=rows)
            p.set_w(None)                  # marks the plan ready; state is overwritten next
            p.t_set_what(W_in)
            p.t_set_rinv(rinv)
            p.t_run_weighted_cov()
            p.t_run_update()
            W_out = p.t_get_what()
        V = orc.weighted_cov_all(X, rinv)
        ref = orc.ip_update_bin(W_in, V, orc.input_covariance(X.astype(np.complex128)), K)
        err = orc.rel_err(W_out, ref)
        _log(test="ip_update", fixture=golden["_id"], model=model, epoch=e, fp64=fp64, rows=rows, What_err=err)
        assert err < 2e-5, (e, err)


@pytest.mark.parametrize("cond", [1e8, 1e10, 1e12])
@pytest.mark.parametrize("M", [3, 4, 6, 8, 12, 16])
def test_determined_update_on_ill_conditioned_covariances(oa, M, cond):
    """the float64 update of the determined case (update_det_kernel up to 8 channels; above: update_det16r_kernel --
    one matrix row per lane, three waves per four bins, round 6 --, with $OIVA_DET16_ROWS=0 update_det16_kernel;
    overiva.py:181-186) on covariances of condition number 1e8 .. 1e12 and a W_hat that is not adapted to them, against the
    oracle's chain (a pivoted solve with W_hat^H V_s per source) from the covariances the device itself formed: within 4 of
    the reference's OWN sensitivities to a change of V in its last bits.  (Round 4's form was up to 1e3 sensitivities off:
    tests/test_update_forms.py.)"""
    from test_update_forms import ill_conditioned_case, reference_sensitivity

    F = 5
    X, W_in, _, _ = ill_conditioned_case(F, M, cond, seed=M)
    X = X.astype(np.complex64)
    T = X.shape[0]
    rinv = np.random.default_rng(3).gamma(2.0, 1.0, (T, M)).astype(np.float32)
    with _plan(oa, X, M, mode="precise") as p:
        Cx = p.get_cx(np.complex128)
        p.set_w(None)                  # marks the plan ready; state is overwritten next
        p.t_set_what(W_in)
        p.t_set_rinv(rinv)
        p.t_run_weighted_cov()
        V = p.t_get_v(np.complex128)
        p.t_run_update()
        W_out = p.t_get_what(np.complex128)
    sens, ref = reference_sensitivity(W_in, V, Cx, M)
    e = orc.rel_err(W_out, ref)
    print(f"\n[parity] determined update, {M} channels, cond(Cx) {np.max(np.linalg.cond(Cx)):.1e}: {e:.2e} (reference sensitivity {sens:.1e})")
    assert e < 4 * sens + 1e-12


@pytest.mark.parametrize("mode", ["fast", "mixed"])
def test_j_initialisation(oa, golden, mode):
    """overiva.py:96-98,120-123.  `mixed` (the default arithmetic, float64 solve): 1e-5; `fast` (float32 solve): 1e-5 up to 8
    channels, 2e-5 -- the bound of test_ip_update -- above (13 channels / 3 sources of a mixture: 1.3e-5)"""
    X, K = golden["X"], int(golden["K"])
    T, F, M = X.shape
    with _plan(oa, X, K, mode=mode) as p:
        p.set_w(None)
        What = p.t_get_what()
        Wg = p.get_w()
    ref = orc.init_demixing(orc.input_covariance(X.astype(np.complex128)), K)
    assert orc.rel_err(What, ref) < (2e-5 if mode == "fast" and M > 8 else 1e-5)
    assert orc.rel_err(Wg, ref[:, :, :K]) == 0.0


def test_activation(oa, golden):
    """one iteration, then r_inv and wscale against the oracle computed from the same start"""
    X, K = golden["X"], int(golden["K"])
    T, F, M = X.shape
    for model in ("laplace", "gauss"):
        with _plan(oa, X, K, model) as p:
            p.set_w(None)
            W0 = p.t_get_what()
            p.iterate(1)
            rinv, wscale = p.t_get_rinv()
        pw = orc.demix_power(X, W0[:, :, :K])
        ref_rinv, ref_ws = orc.finalize_activation(pw, F, model)
        assert orc.rel_err(rinv, ref_rinv) < TOL_KERNEL
        assert orc.rel_err(wscale, ref_ws) < TOL_KERNEL
        assert abs(np.mean(1.0 / rinv.astype(np.float64), axis=0) - 1.0).max() < 1e-5


# --------------------------------------------------------------------------------------------
# end to end: overiva() against the reference's golden outputs
# --------------------------------------------------------------------------------------------
def _demix(X, W):
    return np.einsum("tfm,fmk->tfk", X.astype(np.complex128), np.conj(W.astype(np.complex128)))


@pytest.mark.needs('W_c128_{model}_{n_iter}')
@pytest.mark.parametrize("model", ["laplace", "gauss"])
@pytest.mark.parametrize("n_iter", [0, 1, 2, 5, 20])
@pytest.mark.parametrize("dt", ["c64", "c128"])
def test_overiva_matches_reference(oa, golden, model, n_iter, dt):
    """default arithmetic against the real reference's stored results (where the reference is chaotic: the same bits twice)"""
    X, K = golden["X"], int(golden["K"])
    Xin = X if dt == "c64" else X.astype(np.complex128)
    if chaotic(golden, model, n_iter):
        out = _same_twice(lambda: oa.overiva(Xin, n_src=K, n_iter=n_iter, proj_back=False, model=model, return_filters=True))
        assert out is None or (out[0].dtype == Xin.dtype and out[1].shape == (X.shape[1], X.shape[2], K))
        return
    Y, W = oa.overiva(Xin, n_src=K, n_iter=n_iter, proj_back=False, model=model, return_filters=True)
    assert Y.dtype == Xin.dtype and W.dtype == Xin.dtype
    assert Y.shape == (X.shape[0], X.shape[1], K) and W.shape == (X.shape[1], X.shape[2], K)
    assert W.flags["C_CONTIGUOUS"]
    ref128 = golden[f"W_c128_{model}_{n_iter}"]
    e128 = orc.rel_err(W, ref128)
    b128 = _bound128(golden, model, n_iter)
    eY = orc.rel_err(Y, _demix(X, ref128))
    k64 = f"W_c64_{model}_{n_iter}"
    floor = orc.rel_err(golden[k64], ref128) if k64 in golden else None
    e64 = orc.rel_err(W, golden[k64]) if k64 in golden else None
    mode = oa.last_solver_info()["precision"]      # (what `auto` ran: overiva.resolve_precision + the X-resident rule)
    # One floor against the complex128 result, 1.5 against the complex64 one -- everywhere but on the four rows where the
    # reference's OWN complex64 run is not reproducible to 1e-3 (conftest.c64_diverged: its W moves by `jitter` when X changes
    # in the last bit; e_mix laplace 20: jitter 7.1e-3 = 4 floors).  There the yardstick is that jitter: nothing can be pinned
    # on a result tighter than the result pins itself.
    yard = floor
    if floor is not None and c64_diverged(golden, model, n_iter):
        yard = max(floor, c64_jitter(golden, model, n_iter))
    if mode == "mixed" and floor is not None:
        b128 = max(b128, yard)   # never less accurate than the reference's own complex64 arithmetic ...
    # (Round 5 carried ONE exception here -- fixture z, 160 frames x 40 bins x 8 channels / 3 sources, i.i.d., gauss, 20
    #  iterations: W 1.7 floors from complex128 in `mixed`, because the reference forms the covariances in complex128 and rounds
    #  once (overiva.py:179) where `mixed` adds float32 chains.  Round 6: `auto` runs the float64 covariance on short frame axes
    #  with up to 8 channels -- the row is 1e-7 from complex128 now and the exception list is gone.)
    _log(test="e2e", fixture=golden["_id"], model=model, n_iter=n_iter, input=dt, mode=mode, W_vs_c128=e128,
         Y_vs_c128=eY, W_vs_ref_c64=e64, ref_c64_floor=floor, amp=_amp(golden, model, n_iter), bound_c128=b128,
         ref_c64_jitter=c64_jitter(golden, model, n_iter))
    print(f"\n[parity] {golden['_id']} {model} n_iter={n_iter} {dt} ({mode}): W vs c128 {e128:.2e} (bound {b128:.1e}), Y {eY:.2e}"
          + (f", W vs reference-c64 {e64:.2e} (floor {floor:.1e})" if floor is not None else ""))
    assert e128 < b128 and eY < b128
    if dt == "c64" and floor is not None:
        assert e64 < max(TOL, 1.5 * yard)      # as close to the reference's complex64 run as its own noise allows


@pytest.mark.needs('W_c128_{model}_{n_iter}', 'W_c64_{model}_{n_iter}')
@pytest.mark.parametrize("model", ["laplace", "gauss"])
@pytest.mark.parametrize("n_iter", [1, 5, 20])
def test_fast_mode_accuracy(oa, golden, fast_mode, model, n_iter):
    """the float32 mode: 1e-5 where the reference is well conditioned, a documented envelope elsewhere (where the reference is
    chaotic: the same bits twice)"""
    X, K = golden["X"], int(golden["K"])
    if chaotic(golden, model, n_iter):
        _same_twice(lambda: oa.overiva(X, n_src=K, n_iter=n_iter, proj_back=False, model=model, return_filters=True))
        return
    _, W = oa.overiva(X, n_src=K, n_iter=n_iter, proj_back=False, model=model, return_filters=True)
    ref128 = golden[f"W_c128_{model}_{n_iter}"]
    floor = orc.rel_err(golden[f"W_c64_{model}_{n_iter}"], ref128)
    e128 = orc.rel_err(W, ref128)
    _log(test="e2e", fixture=golden["_id"], model=model, n_iter=n_iter, input="c64", mode="fast", W_vs_c128=e128,
         Y_vs_c128=None, W_vs_ref_c64=orc.rel_err(W, golden[f"W_c64_{model}_{n_iter}"]), ref_c64_floor=floor,
         amp=_amp(golden, model, n_iter), bound_c128=max(TOL, FAST_FLOORS * floor))
    print(f"\n[parity] {golden['_id']} {model} n_iter={n_iter} fast: W vs c128 {e128:.2e} = {e128 / floor:.1f} reference floors")
    assert e128 < max(TOL, FAST_FLOORS * floor)


@pytest.mark.needs('Ypb_c128_{model}_12')
@pytest.mark.parametrize("model", ["laplace", "gauss"])
def test_proj_back_and_callback(oa, golden, model):
    X, K = golden["X"], int(golden["K"])
    if chaotic(golden, model, 12):        # (the reference is chaotic here: the same bits twice, callbacks included)
        def run():
            seen = []
            Y = oa.overiva(X.astype(np.complex128), n_src=K, n_iter=12, proj_back=True, model=model, callback=lambda y: seen.append(np.array(y)))
            assert len(seen) == 2
            return (Y, *seen)
        _same_twice(run)
        return
    got = []
    Y = oa.overiva(X.astype(np.complex128), n_src=K, n_iter=12, proj_back=True, model=model,
                   callback=lambda y: got.append(np.array(y)))
    bound = _bound128(golden, model, 12)
    e = orc.rel_err(Y, golden[f"Ypb_c128_{model}_12"])
    _log(test="proj_back", fixture=golden["_id"], model=model, n_iter=12, input="c128", mode="precise", Y_vs_c128=e,
         amp=_amp(golden, model, 12), bound_c128=bound)
    print(f"\n[parity] {golden['_id']} {model} proj_back 12 its: Y err {e:.2e} (bound {bound:.1e})")
    assert e < bound
    assert len(got) == 2 and got[0].shape == Y.shape and got[0].dtype == np.complex128
    if model == "laplace":
        assert orc.rel_err(got[0], golden["cb0_c128_laplace"]) < bound
        assert orc.rel_err(got[1], golden["cb10_c128_laplace"]) < bound


@pytest.mark.needs('Ypb_frame0_c128_laplace_12')
def test_frame0_of_large_fixtures(oa, golden):
    """the F >= 64 fixtures keep frame 0 of the projected-back outputs (pins z of every bin and source)"""
    X, K = golden["X"].astype(np.complex128), int(golden["K"])
    Y = oa.overiva(X, n_src=K, n_iter=12, proj_back=True, model="laplace")
    e = orc.rel_err(Y[0], golden["Ypb_frame0_c128_laplace_12"])
    Yp = oa.auxiva_pca(X, n_src=K, n_iter=5, proj_back=True, model="laplace")
    ep = orc.rel_err(Yp[0], golden["Ypca_frame0_c128_laplace_5"])
    _log(test="frame0", fixture=golden["_id"], model="laplace", n_iter=12, input="c128", mode="precise", Y_vs_c128=e,
         pca_Y_vs_c128=ep)
    print(f"\n[parity] {golden['_id']} proj_back frame 0: overiva {e:.2e}, auxiva_pca {ep:.2e}")
    assert e < _bound128(golden, "laplace", 20) and ep < 2 * _bound128(golden, "laplace", 20)


@pytest.mark.needs('W0')
def test_warm_start_default_nsrc_eig(oa, golden):
    X, K = golden["X"], int(golden["K"])
    X128 = X.astype(np.complex128)
    _, W = oa.overiva(X128, n_src=K, n_iter=3, proj_back=False, W0=golden["W0"], return_filters=True)
    e0 = orc.rel_err(W, golden["W_w0_c128_laplace_3"])
    _, W = oa.overiva(X128, n_iter=2, proj_back=False, return_filters=True)
    assert W.shape == golden["W_det_c128_laplace_2"].shape
    e1 = orc.rel_err(W, golden["W_det_c128_laplace_2"])
    Y, W = oa.overiva(X128, n_src=K, n_iter=3, proj_back=False, init_eig=True, return_filters=True)
    # the device eigensolver applies LAPACK's phase convention (largest component real), so Y itself is comparable
    e2 = orc.rel_err(Y, golden["Y_eig_c128_laplace_3"])
    _log(test="warm/det/eig", fixture=golden["_id"], model="laplace", n_iter=3, input="c128", mode="precise", W_w0=e0,
         W_det=e1, absY_eig=e2)
    print(f"\n[parity] {golden['_id']} W0 3 its {e0:.2e}, determined 2 its {e1:.2e}, init_eig |Y| {e2:.2e}")
    b = _bound128(golden, "laplace", 5)
    assert e0 < b and e1 < b and e2 < b


@pytest.mark.needs('Ypca_c128_laplace_5')
def test_auxiva_pca(oa, golden):
    X, K = golden["X"], int(golden["K"])
    Y = oa.auxiva_pca(X.astype(np.complex128), n_src=K, n_iter=5, proj_back=True, model="laplace")
    assert Y.shape == golden["Ypca_c128_laplace_5"].shape and Y.dtype == np.complex128
    e = orc.rel_err(Y, golden["Ypca_c128_laplace_5"])
    _log(test="auxiva_pca", fixture=golden["_id"], model="laplace", n_iter=5, input="c128", mode="precise", Y_vs_c128=e)
    print(f"\n[parity] {golden['_id']} auxiva_pca 5 its: Y err {e:.2e}")
    assert e < 2 * _bound128(golden, "laplace", 5)      # (the PCA projection of X is a float32 pass of its own)
    with pytest.raises(KeyError):
        oa.auxiva_pca(X.astype(np.complex128), n_src=K, n_iter=1)


@pytest.mark.parametrize("shape", [(200, 9, 4, 2), (150, 6, 5, 2), (300, 7, 8, 3), (120, 3, 3, 1), (400, 5, 16, 4), (260, 4, 13, 6),
                                   (90, 3, 2, 1), (250, 5, 8, 7)])
def test_init_eig_on_device_matches_numpy_eig(oa, shape):
    """init_eig (overiva.py:106-109) from the device eigensolver against numpy.linalg.eig of the same covariance:
    W0 = conj of the K principal eigenvectors, each with LAPACK's phase (largest component real)"""
    from overiva_amd.overiva import eig_init

    T, F, M, K = shape
    X = orc.synth_mixture(T, F, M, K, seed=sum(shape) + 1)
    with oa.Plan(T, F, M, K, "laplace") as p:
        p.set_precision("precise")
        p.set_x(X)
        p.covariance()
        Cx = p.get_cx(np.complex128)
        p.set_w_eig()
        W = p.get_w(np.complex128)
    lam = np.linalg.eigvalsh(Cx)
    gap = np.min(np.diff(lam, axis=1)) / np.max(lam)
    assert orc.rel_err(W, eig_init(Cx, K)) < 1e-11 / max(gap, 1e-6)


@pytest.mark.parametrize("shape", [(200, 9, 4, 2), (150, 6, 5, 2), (300, 7, 8, 3), (120, 3, 3, 1), (400, 5, 16, 4), (260, 4, 13, 6),
                                   (90, 3, 2, 1), (250, 5, 8, 7)])
def test_pca_subspace_on_device(oa, shape):
    """the Jacobi eigensolver behind auxiva_pca (auxiva_pca.py:75-81) against numpy.linalg.eigh of the same covariance:
    all eigenvalues, the projector onto the K principal eigenvectors, their order, orthonormality; then the projection
    new_X = X conj(w[:, :, -K:]) up to the phase of each component, and that the device-resident new_X feeds a solve"""
    T, F, M, K = shape
    X = orc.synth_mixture(T, F, M, K, seed=sum(shape))
    with oa.Plan(T, F, M, K, "laplace") as p:
        p.set_precision("precise")
        p.set_x(X)
        p.covariance()
        Cx = p.get_cx(np.complex128)
        ev = p.set_w_pca(return_eigenvalues=True)
        P = p.get_w(np.complex128)
        new_X = p.demix(proj_back=False)
        dev = p.demix_device(proj_back=False)
        assert dev.shape == (T, F, K)
        Yd = oa.overiva(dev, n_iter=2, proj_back=False)
        Yh = oa.overiva(new_X, n_iter=2, proj_back=False)
    lam, vec = np.linalg.eigh(Cx)
    assert np.max(np.abs(ev - lam)) <= 1e-12 * np.max(np.abs(lam))
    Pr = vec[:, :, -K:]
    eye = np.broadcast_to(np.eye(K), (F, K, K))
    assert np.max(np.abs(np.conj(P.swapaxes(1, 2)) @ P - eye)) < 1e-12
    gap = np.min(np.diff(lam, axis=1)) / np.max(lam)
    tol = 1e-11 / max(gap, 1e-6)
    # column by column: the same eigenvector up to a phase, in the same (ascending) order
    c = np.abs(np.einsum("fmk,fmk->fk", np.conj(Pr), P))
    assert np.max(np.abs(c - 1.0)) < tol, (np.max(np.abs(c - 1.0)), gap)
    ref = np.einsum("tfm,fmk->tfk", X, np.conj(Pr)).astype(np.complex64)
    phase = np.einsum("fmk,fmk->fk", np.conj(Pr), P)          # P = Pr * phase, so new_X = ref * conj(phase)
    assert orc.rel_err(new_X, ref * np.conj(phase)[None]) < 1e-6
    assert Yd.dtype == np.complex64 and np.array_equal(Yd, Yh)   # device hand-over == host round trip, bit for bit


@pytest.mark.parametrize("shape", [(96, 5, 11, 3), (80, 3, 9, 9), (72, 6, 13, 1), (64, 4, 16, 5), (50, 7, 7, 7), (90, 19, 5, 2),
                                   (90, 21, 8, 3), (64, 9, 8, 4), (70, 5, 8, 5), (100, 12, 8, 8), (60, 7, 7, 4), (64, 5, 12, 12),
                                   (70, 4, 16, 16), (60, 3, 10, 10), (66, 2, 15, 15), (80, 6, 6, 4), (75, 5, 8, 6), (90, 4, 5, 3),
                                   (85, 5, 6, 3), (77, 6, 7, 5)])
@pytest.mark.parametrize("model", ["laplace", "gauss"])
def test_odd_shapes_against_oracle(oa, shape, model):
    """channel counts without a golden fixture (incl. the 9..16-channel covariance kernels) and every form of the per-bin update
    -- structured chain (1-2 sources + background), Gram form (3 and more sources + background), maintained inverse (determined, up
    to 8 and 9..16 channels) -- in the default arithmetic"""
    T, F, M, K = shape
    X = orc.synth_iid(T, F, M, seed=sum(shape))
    Yr, Wr = orc.overiva_staged(X, n_src=K, n_iter=4, proj_back=True, model=model, return_filters=True)
    mode = "mixed"
    try:
        Y, W = oa.overiva(X, n_src=K, n_iter=4, proj_back=True, model=model, return_filters=True)
        mode = oa.last_solver_info()["precision"]
        eW, eY = orc.rel_err(W, Wr), orc.rel_err(Y, Yr)
    except np.linalg.LinAlgError:
        # a W_hat^H V that is singular in complex64 arithmetic (gauss, 2 bins x 15 channels: the weights 1 / r leave V to a
        # few frames): the error the reference raises there too (numpy.linalg.solve) -- accepted only where the
        # reference's own complex64 arithmetic is chaotic (below)
        assert mode == "mixed"
        eW = eY = np.inf
    bound = TOL
    if mode == "mixed" and max(eW, eY) >= TOL:
        # complex64 arithmetic on an ill-conditioned case (gauss with 3-5 bins and 10-16 channels): as far from the
        # complex128 result as the reference's OWN complex64 arithmetic (oracle, reference-faithful form) is -- and
        # nothing to pin where that arithmetic is itself chaotic
        floor = _c64_floor(lambda: orc.overiva_faithful(X, n_src=K, n_iter=4, proj_back=True, model=model, return_filters=True)[1], Wr)
        if not floor < 1e-2:
            # nothing to pin on the complex64 result: the call gives the same bits (or the same error) twice, and complex128
            # input, which runs `precise`, still reaches the complex128 result
            print(f"\n[parity] T{T} F{F} M{M} K{K} {model}: reference complex64 arithmetic chaotic (floor {floor:.1e}), ours {eW:.1e}")
            _same_twice(lambda: oa.overiva(X, n_src=K, n_iter=4, proj_back=True, model=model, return_filters=True))
            Y, W = oa.overiva(X.astype(np.complex128), n_src=K, n_iter=4, proj_back=True, model=model, return_filters=True)
            assert orc.rel_err(W, Wr) < TOL and orc.rel_err(Y, Yr) < 2 * TOL
            return
        bound = max(TOL, 1.5 * floor)       # the same 1.5 floors test_overiva_matches_reference allows complex64 input
    _log(test="odd_shape", fixture=f"T{T}F{F}M{M}K{K}", model=model, n_iter=4, input="c64", mode=mode, W_vs_c128=eW,
         Y_vs_c128=eY)
    print(f"\n[parity] T{T} F{F} M{M} K{K} {model} 4 its ({mode}): W err {eW:.2e} Y err {eY:.2e} (bound {bound:.1e})")
    assert eW < bound and eY < 2 * bound


# (T, F, M, K), the covariance and the power kernel `mixed` runs on it (csrc/kernel_choice.h)
MANY_SOURCES_64_BINS = [((256, 64, 16, 16), "Hmfma", "Lds"),      # one whole batch
                        ((200, 130, 16, 16), "Hmfma", "Lds"),     # two batches + a ragged one of 2 bins
                        ((160, 65, 16, 9), "Hmfma", "Lds"),       # background channels, one-bin ragged batch
                        ((192, 128, 16, 5), "Half16", "Lds"),
                        ((160, 79, 15, 15), "Hmfma", "Mfma"),     # padded copy of X, ragged batch
                        ((144, 70, 12, 12), "Hmfma", "Mfma"),
                        ((150, 66, 10, 6), "Half16", "Mfma")]


@pytest.mark.parametrize("model", ["laplace", "gauss"])
@pytest.mark.parametrize("shape,cov_kind,pow_kind", MANY_SOURCES_64_BINS, ids=["x".join(str(v) for v in c[0]) for c in MANY_SOURCES_64_BINS])
def test_many_sources_from_64_bins_against_oracle(oa, shape, cov_kind, pow_kind, model):
    """more than 8 channels and more than 4 sources at 64 bins and more, ITERATED: the chain matrix-core power pass (power_lds_kernel /
    power_mfma_kernel over several 64-bin batches with a ragged last one) -> activation -> cov_hmfma / cov_half16 -> per-bin
    update (update_det16r_kernel where determined) of BASELINE.json configs[4], five iterations against the oracle's
    complex128 result (overiva.py:138-190).  Every part of that chain is held against the oracle alone elsewhere, at these
    sizes; the hand-over between the parts at several batches only here.  Bounds from the reference's own arithmetic (oracle,
    reference-faithful complex64 form against the complex128 one, 5 iterations): i.i.d. input floors 1.2e-7 .. 4.5e-7 -> the north
    star's 1e-5 on W and Y; complex128 input (runs `precise`) 1e-6 on W as test_rows_kernel_against_the_oracle; mixture-like
    input floors 1.8e-5 .. 4.9e-4 -> max(1e-5, 1.5 floors) on W with the floor computed here.  (192 x 128 x 16 / 5 gauss on the
    mixture: the reference's complex64 floor is 1.3 -- chaotic, nothing to pin -- and that one leg is left out.)"""
    from overiva_amd import plan

    T, F, M, K = shape
    kw = dict(n_src=K, n_iter=5, proj_back=False, model=model, return_filters=True)
    fixture = f"T{T}F{F}M{M}K{K}"
    X = orc.synth_iid(T, F, M, seed=sum(shape))
    Yr, Wr = orc.overiva_staged(X, **kw)
    # complex64 input: `mixed`, the kernels the row is named for
    Y, W = oa.overiva(X, **kw)
    info = oa.last_solver_info()
    assert info["precision"] == "mixed" and not info["sharded"] and info["resident_launches"] == 0
    choice = plan.kernel_choice(T, F, M, K, info["precision"])
    assert (choice["cov_kind"], choice["pow_kind"]) == (cov_kind, pow_kind)
    eW, eY = orc.rel_err(W, Wr), orc.rel_err(Y, Yr)
    _log(test="many_sources_64", fixture=fixture + " iid", model=model, n_iter=5, input="c64", mode="mixed", W_vs_c128=eW, Y_vs_c128=eY)
    print(f"\n[parity] {fixture} iid {model} 5 its (mixed, {cov_kind} + {pow_kind}): W err {eW:.2e} Y err {eY:.2e} (bound {TOL:.0e})")
    assert eW < TOL and eY < TOL
    # complex128 input: `precise` -- the same power pass, float64 covariances
    _, W128 = oa.overiva(X.astype(np.complex128), **kw)
    info = oa.last_solver_info()
    assert info["precision"] == "precise" and plan.kernel_choice(T, F, M, K, "precise")["pow_kind"] == pow_kind
    e128 = orc.rel_err(W128, Wr)
    _log(test="many_sources_64", fixture=fixture + " iid", model=model, n_iter=5, input="c128", mode="precise", W_vs_c128=e128)
    print(f"\n[parity] {fixture} iid {model} 5 its (precise): W err {e128:.2e} (bound 1e-06)")
    assert e128 < 1e-6
    # mixture-like input, complex64: within 1.5 of the reference's own complex64 floors
    if shape == (192, 128, 16, 5) and model == "gauss":
        return
    Xm = orc.synth_mixture(T, F, M, K, seed=sum(shape))
    _, Wmr = orc.overiva_staged(Xm, **kw)
    floor = _c64_floor(lambda: orc.overiva_faithful(Xm, **kw)[1], Wmr)
    _, Wm = oa.overiva(Xm, **kw)
    assert oa.last_solver_info()["precision"] == "mixed"
    em = orc.rel_err(Wm, Wmr)
    bound = max(TOL, 1.5 * floor)
    _log(test="many_sources_64", fixture=fixture + " mixture", model=model, n_iter=5, input="c64", mode="mixed", W_vs_c128=em,
         ref_c64_floor=floor, bound_c128=bound)
    print(f"\n[parity] {fixture} mixture {model} 5 its (mixed): W err {em:.2e} (reference c64 floor {floor:.2e}, bound {bound:.1e})")
    assert em < bound


_RANDOM_SKIPPED = []


def _random_shapes(n=60, seed=123):
    rng = np.random.default_rng(seed)
    out = []
    for it in range(n):
        M = int(rng.integers(2, 17))
        K = int(rng.integers(1, M + 1))
        F = int(rng.integers(1, 40))
        T = int(rng.integers(4 * M, 160))
        out.append((it, T, F, M, K, ("laplace", "gauss")[it % 2]))
    return out


@pytest.mark.parametrize("case", _random_shapes(), ids=lambda c: f"{c[0]}-T{c[1]}F{c[2]}M{c[3]}K{c[4]}-{c[5]}")
def test_random_shapes_against_oracle(oa, case):
    """60 shapes drawn with a fixed seed -- 2..16 channels, 1..M sources, 1..39 bins, 4 M..159 frames, both models, complex64 and
    complex128 input -- through every dispatch of the covariance and update kernels, 3 iterations on i.i.d. input: W and Y
    within the north star's 1e-5 of the oracle's complex128 result, or -- where the reference's own complex64 arithmetic
    (oracle, reference-faithful form) is farther than that from it: gauss over a handful of bins -- within 1.5 of its floors;
    skipped, visibly, where that arithmetic is itself chaotic (floor > 1e-2) or the algorithm degenerate"""
    it, T, F, M, K, model = case
    X = orc.synth_iid(T, F, M, seed=1000 + it)
    with np.errstate(all="ignore"):
        try:
            Yr, Wr = orc.overiva_staged(X, n_src=K, n_iter=3, proj_back=True, model=model, return_filters=True)
        except np.linalg.LinAlgError:
            pytest.skip("degenerate for the algorithm itself (singular in complex128)")
    if not (np.all(np.isfinite(Wr)) and np.all(np.isfinite(Yr))):
        pytest.skip("degenerate for the algorithm itself (oracle non-finite)")
    floor = None
    for dt in (np.complex64, np.complex128):
        try:
            Y, W = oa.overiva(X.astype(dt), n_src=K, n_iter=3, proj_back=True, model=model, return_filters=True)
            eW, eY = orc.rel_err(W, Wr), orc.rel_err(Y, Yr)
        except np.linalg.LinAlgError:
            eW = eY = np.inf          # (accepted only where the reference's own complex64 arithmetic is chaotic, below)
        bound = TOL
        if not (eW < TOL and eY < TOL):
            if floor is None:
                floor = _c64_floor(lambda: orc.overiva_faithful(X, n_src=K, n_iter=3, proj_back=True, model=model, return_filters=True)[1], Wr)
            if not floor < 1e-2:
                _RANDOM_SKIPPED.append(case)
                assert len(_RANDOM_SKIPPED) <= 6, f"too many of the 60 random shapes skipped as chaotic: {_RANDOM_SKIPPED}"
                pytest.skip(f"the reference's complex64 arithmetic is chaotic here (floor {floor:.1e}); ours {eW:.1e} ({dt.__name__})")
            #  the reference's complex64 floor loosens the bound of the complex64 leg only: complex128 input runs the
            # float64 arithmetic (`precise`), which owes the 1e-5 whatever the complex64 arithmetic does on this input
            if dt == np.complex64:
                bound = max(TOL, 1.5 * floor)
        print(f"\n[parity] random {case[1:]} {dt.__name__}: W err {eW:.2e} Y err {eY:.2e} (bound {bound:.1e})")
        assert eW < bound and eY < 2 * bound, ((T, F, M, K), model, dt.__name__, eW, eY, floor)


@pytest.mark.parametrize("shape", [(5, 1, 1, 1), (17, 3, 2, 1), (33, 70, 3, 3), (5000, 2, 4, 2), (16, 16, 8, 8),
                                   (2, 5, 2, 2), (1000, 1, 6, 2), (337, 3, 4, 3), (1000, 40, 8, 2), (1029, 5, 8, 1)])
def test_ragged_and_extreme_shapes(oa, shape):
    """frames not a multiple of the 16-frame step (incl. frame counts that leave whole waves of the last step
    past the end of the tensor), fewer bins than a 16-bin wave, single bin / channel, very long and very short
    frame axes; both arithmetic modes"""
    T, F, M, K = shape
    X = orc.synth_iid(T, F, M, seed=7 + sum(shape))
    Yr, Wr = orc.overiva_staged(X, n_src=K, n_iter=3, proj_back=False, return_filters=True)
    if not np.all(np.isfinite(Wr)):
        pytest.skip("degenerate for the algorithm itself (oracle non-finite)")
    floor = _c64_floor(lambda: orc.overiva_faithful(X, n_src=K, n_iter=3, proj_back=False, return_filters=True)[1], Wr)
    for mode in ("precise", "mixed", "fast"):      # (mixed and fast run the X-resident kernel where the shape qualifies)
        oa.set_precision(mode)
        try:
            Y, W = oa.overiva(X, n_src=K, n_iter=3, proj_back=False, return_filters=True)
        finally:
            oa.set_precision("auto")
        eW, eY = orc.rel_err(W, Wr), orc.rel_err(Y, Yr)
        print(f"\n[parity] T{T} F{F} M{M} K{K} {mode}: W err {eW:.2e} Y err {eY:.2e} (reference c64 floor {floor:.1e})")
        fl = 1.5 if mode != "fast" else FAST_FLOORS
        assert eW < max(TOL, fl * floor) and eY < max(TOL, fl * floor)


def test_config1_shape_against_oracle(oa):
    """BASELINE.json configs[0] shape: 2049 bins x ~160 frames x 4 mics / 2 src, complex128 in, 20 iterations,
    proj_back and the callback every 10 epochs (overiva_oneshot.py -a overiva -m 4 -s 2 -n 20)"""
    X = orc.synth_mixture(160, 2049, 4, 2, seed=3).astype(np.complex128)
    got, ref_got = [], []
    Y = oa.overiva(X, n_src=2, n_iter=20, proj_back=True, callback=lambda y: got.append(y.copy()))
    Yr = orc.overiva_staged(X, n_src=2, n_iter=20, proj_back=True, callback=lambda y: ref_got.append(y.copy()))
    e = orc.rel_err(Y, Yr)
    _log(test="cfg1", fixture="T160F2049M4K2 mixture", model="laplace", n_iter=20, input="c128", mode="precise", Y_vs_c128=e)
    print(f"\n[parity] cfg1 shape mixture 20 its proj_back: Y err {e:.2e}")
    assert Y.dtype == np.complex128 and len(got) == len(ref_got) == 2
    assert e < TOL
    assert orc.rel_err(got[1], ref_got[1]) < TOL


def test_errors(oa):
    X = orc.synth_iid(32, 4, 3, seed=1)
    with pytest.raises(ValueError):
        oa.overiva(X, n_src=2, model="cauchy")
    with pytest.raises(ValueError):
        oa.overiva(X, n_src=4)
    with pytest.raises(TypeError):
        oa.overiva(X.real, n_src=2)
    # a rank-deficient input makes W_hat^H V singular: numpy raises LinAlgError in the reference
    Xz = np.zeros((32, 4, 3), np.complex64)
    with pytest.raises(np.linalg.LinAlgError):
        oa.overiva(Xz, n_src=2, n_iter=1, proj_back=False)


def test_complex128_in_and_out_are_converted_on_the_device(oa):
    """complex128 arrays cross the boundary as they are (the conversion to the device's complex64 and back runs on the
    GPU): same bits as converting on the host, for X, for Y, for a bin shard of a larger array and for a callback"""
    T, F, M, K = 130, 21, 4, 2
    X128 = orc.synth_mixture(T, F, M, K, seed=4).astype(np.complex128) * (1 + 1e-9)      # not representable in complex64
    X64 = X128.astype(np.complex64)
    seen = []
    oa.set_precision("precise")        # one arithmetic for both dtypes (the default follows the dtype of X)
    try:
        Y128, W128 = oa.overiva(X128, n_src=K, n_iter=11, return_filters=True, callback=lambda Y: seen.append(Y.copy()))
        Y64, W64 = oa.overiva(X64, n_src=K, n_iter=11, return_filters=True, callback=lambda Y: None)   # (same launch cadence)
    finally:
        oa.set_precision("auto")
    assert Y128.dtype == np.complex128 and W128.dtype == np.complex128 and Y64.dtype == np.complex64
    assert np.array_equal(Y128, Y64.astype(np.complex128))
    assert np.array_equal(W128.astype(np.complex64), W64)
    assert len(seen) == 2 and all(y.dtype == np.complex128 and y.shape == (T, F, K) for y in seen)
    with oa.Plan(T, 8, M, K, "laplace") as p:                  # bins 5..12 of the larger arrays
        p.set_x(X128, f0=5)
        p.covariance()
        p.set_w(None)
        p.iterate(2)
        out = np.zeros((T, F, K), np.complex128)
        p.demix(True, out=out, f0=5)
        ref = p.demix(True)
        assert np.array_equal(out[:, 5:13], ref.astype(np.complex128)) and not out[:, :5].any() and not out[:, 13:].any()
    with oa.Plan(T, 8, M, K, "laplace") as q:
        q.set_x(X64, f0=5)
        q.covariance()
        q.set_w(None)
        q.iterate(2)
        assert np.array_equal(q.demix(True), ref)


def test_input_not_mutated_and_noncontiguous(oa):
    X = orc.synth_iid(64, 9, 4, seed=2)
    Xt = np.asfortranarray(X)            # non C-contiguous view of the same values
    keep = X.copy()
    Y1 = oa.overiva(X, n_src=2, n_iter=3, proj_back=True)
    Y2 = oa.overiva(Xt, n_src=2, n_iter=3, proj_back=True)
    assert np.array_equal(X, keep)
    assert np.array_equal(Y1, Y2)        # deterministic: same input, bitwise same output


def test_graph_replay_equals_eager(oa):
    X = orc.synth_iid(128, 40, 4, seed=3)
    outs = []
    for graph in (False, True):
        with _plan(oa, X, 2) as p:
            p.use_graph(graph)
            p.set_w(None)
            p.iterate(3)
            p.iterate(2)
            p.iterate(19)          # one replayed graph per call (cached by length), 40: 32 + 8
            p.iterate(40)
            outs.append(p.get_w())
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("shape", [(4000, 2048, 8, 2), (4000, 1700, 8, 2), (1024, 2048, 8, 2), (4096, 2047, 8, 2)],
                         ids=lambda s: "x".join(str(v) for v in s))
@pytest.mark.parametrize("mode,model", [("mixed", "laplace"), ("fast", "gauss")])
def test_covariance_and_update_in_one_launch_give_the_bits_of_two(oa, shape, mode, model):
    """cov_update_kernel (csrc/kernels_cov_update.hip; overiva.py:158-190 for 8 channels / 2 sources where the plan's covariance
    geometry is four frame splits: the headline shape): 4 bins x all frames per workgroup, one wave per split, the update of
    the four bins in the same launch -- the lane chains, the order of the float64 sums over phases and splits and the update
    chain are those of cov_dma_kernel + update_bg_kernel, so W must be THE SAME BITS, eagerly and from replayed graphs, on
    i.i.d. and on mixture input, with ragged bin counts"""
    T, F, M, K = shape
    X = orc.synth_mixture(T, F, M, K, seed=8) if F % 2 else orc.synth_iid(T, F, M, seed=8)
    outs = []
    for fuse in (False, True):
        for graph in (False, True):
            with oa.Plan(T, F, M, K, model) as p:
                p.set_precision(mode)
                p.set_x(X)
                p.covariance()
                p.set_w(None)
                active = p.set_fuse_cov_update(fuse)
                if p.cov_splits() != 4:
                    pytest.skip(f"the plan chose {p.cov_splits()} frame splits for this shape: the one-launch form does not apply")
                assert active == fuse
                p.use_graph(graph)
                p.iterate(3)
                p.iterate(2)
                _, wscale = p.t_get_rinv()
                outs.append((p.get_w(np.complex128), p.demix(True), wscale))
    for W, Y, ws in outs[1:]:
        assert np.array_equal(W, outs[0][0]) and np.array_equal(Y, outs[0][1]) and np.array_equal(ws, outs[0][2])
    assert np.all(np.isfinite(outs[0][0]))


# --------------------------------------------------------------------------------------------
# BASELINE configs against the oracle; the headline size also through size-independent properties
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["precise", "mixed", "fast"])
def test_cfg2_against_oracle(oa, mode):
    """513 bins x 1000 frames x 4 mics / 2 src, laplace (BASELINE.json configs[1])"""
    X = orc.synth_iid(1000, 513, 4, seed=0)
    oa.set_precision(mode)
    try:
        Y, W = oa.overiva(X, n_src=2, n_iter=10, proj_back=False, return_filters=True)
    finally:
        oa.set_precision("auto")
    Yr, Wr = orc.overiva_staged(X, n_src=2, n_iter=10, proj_back=False, return_filters=True)
    eW, eY = orc.rel_err(W, Wr), orc.rel_err(Y, Yr)
    _log(test="cfg2", fixture="T1000F513M4K2 iid", model="laplace", n_iter=10, input="c64", mode=mode, W_vs_c128=eW, Y_vs_c128=eY)
    print(f"\n[parity] cfg2 iid 10 its {mode}: W err {eW:.2e}  Y err {eY:.2e}")
    assert eW < TOL and eY < TOL


@pytest.mark.parametrize("mode", ["precise", "mixed", "fast"])
def test_cfg2_mixture_against_oracle(oa, mode):
    X = orc.synth_mixture(1000, 513, 4, 2, seed=1)
    oa.set_precision(mode)
    try:
        Y, W = oa.overiva(X, n_src=2, n_iter=10, proj_back=False, return_filters=True)
    finally:
        oa.set_precision("auto")
    Yr, Wr = orc.overiva_staged(X, n_src=2, n_iter=10, proj_back=False, return_filters=True)
    _, Wf = orc.overiva_faithful(X, n_src=2, n_iter=10, proj_back=False, return_filters=True)
    floor = orc.rel_err(Wf, Wr)          # the reference's own complex64 arithmetic on this input
    eW, eY, e64 = orc.rel_err(W, Wr), orc.rel_err(Y, Yr), orc.rel_err(W, Wf)
    _log(test="cfg2", fixture="T1000F513M4K2 mixture", model="laplace", n_iter=10, input="c64", mode=mode, W_vs_c128=eW,
         Y_vs_c128=eY, W_vs_ref_c64=e64, ref_c64_floor=floor)
    print(f"\n[parity] cfg2 mixture 10 its {mode}: W err {eW:.2e}  Y err {eY:.2e}, vs reference-c64 {e64:.2e} (floor {floor:.2e})")
    if mode == "precise":
        assert eW < TOL and eY < TOL and e64 < max(TOL, 1.5 * floor)
    elif mode == "mixed":
        assert eW < max(TOL, floor) and eY < max(TOL, floor) and e64 < max(TOL, 1.5 * floor)
    else:
        assert eW < max(TOL, FAST_FLOORS * floor)


@pytest.fixture(scope="module")
def headline_iid():
    """the headline input and the oracle's reference-faithful results after 3 iterations, both models (computed once: ~20 s
    of CPU work each on the GPU box)"""
    T, F, M, K = 4000, 2048, 8, 2
    X = orc.synth_iid(T, F, M, seed=0)
    ref = {}
    for model in ("laplace", "gauss"):
        ref[model] = orc.overiva_faithful(X, n_src=K, n_iter=3, proj_back=False, model=model, return_filters=True)
    return X, ref


def _one_launch_env(oa, monkeypatch, shape, on):
    """$OIVA_COV_UPDATE for the plans overiva() creates from here on (read at plan creation: plans kept from earlier calls are
    dropped); on: checks that a plan of this shape really runs covariance and update as ONE launch (cov_update_kernel)"""
    oa.release_cached_buffers()
    if not on:
        monkeypatch.delenv("OIVA_COV_UPDATE", raising=False)
        return
    monkeypatch.setenv("OIVA_COV_UPDATE", "1")
    T, F, M, K = shape
    with oa.Plan(T, F, M, K, "laplace") as p:
        p.set_precision("mixed")
        assert p.set_fuse_cov_update(True), "the one-launch form does not apply to this shape"


@pytest.mark.parametrize("model", ["laplace", "gauss"])
@pytest.mark.parametrize("mode,one_launch", [("precise", False), ("mixed", False), ("fast", False), ("mixed", True), ("fast", True)])
def test_headline_size_against_oracle(oa, headline_iid, mode, one_launch, model, monkeypatch):
    """2048 x 4000 x 8 / 2 (BASELINE.json configs[2]) end to end against the oracle's reference-faithful form
    (the reference's own arithmetic: complex64 data, float64 activations) for a few iterations, both source models.
    one_launch: covariance + IP1 + J of a bin batch in ONE kernel (cov_update_kernel, the north star's fusion at this shape, opt-in
    because it measures no faster) against the oracle directly, not only against the two launches' bits."""
    X, ref = headline_iid
    K = 2
    _one_launch_env(oa, monkeypatch, (X.shape[0], X.shape[1], X.shape[2], K), one_launch)
    oa.set_precision(mode)
    try:
        Y, W = oa.overiva(X, n_src=K, n_iter=3, proj_back=False, model=model, return_filters=True)
    finally:
        oa.set_precision("auto")
        oa.release_cached_buffers()
    Yr, Wr = ref[model]
    eW, eY = orc.rel_err(W, Wr), orc.rel_err(Y, Yr)
    _log(test="headline" + ("-one-launch" if one_launch else ""), fixture="T4000F2048M8K2 iid", model=model, n_iter=3, input="c64", mode=mode,
         W_vs_ref_c64=eW, Y_vs_ref_c64=eY)
    print(f"\n[parity] headline shape iid {model} 3 its {mode} vs reference-faithful c64: W err {eW:.2e}  Y err {eY:.2e}")
    assert eW < TOL and eY < TOL


@pytest.mark.parametrize("model", ["laplace", "gauss"])
def test_shard_size_mixture_20_iterations(oa, model):
    """256 bins x 4000 frames x 8 mics / 2 src (one rank's share of the headline shape at 8 GPUs), mixture-like
    input, 20 iterations: against the reference-faithful complex64 oracle (the target for complex64 input) and the
    complex128 one"""
    T, F, M, K = 4000, 256, 8, 2
    X = orc.synth_mixture(T, F, M, K, seed=11)
    Y, W = oa.overiva(X, n_src=K, n_iter=20, proj_back=False, model=model, return_filters=True)
    _, W128 = orc.overiva_staged(X, n_src=K, n_iter=20, proj_back=False, model=model, return_filters=True)
    _, W64 = orc.overiva_faithful(X, n_src=K, n_iter=20, proj_back=False, model=model, return_filters=True)
    floor = orc.rel_err(W64, W128)
    e128, e64 = orc.rel_err(W, W128), orc.rel_err(W, W64)
    eY = orc.rel_err(Y, _demix(X, W128))
    oa.set_precision("fast")
    try:
        _, Wfast = oa.overiva(X, n_src=K, n_iter=20, proj_back=False, model=model, return_filters=True)
    finally:
        oa.set_precision("auto")
    efast = orc.rel_err(Wfast, W128)
    _log(test="shard20", fixture="T4000F256M8K2 mixture", model=model, n_iter=20, input="c64", mode="mixed", W_vs_c128=e128,
         Y_vs_c128=eY, W_vs_ref_c64=e64, ref_c64_floor=floor)
    _log(test="shard20", fixture="T4000F256M8K2 mixture", model=model, n_iter=20, input="c64", mode="fast", W_vs_c128=efast,
         ref_c64_floor=floor)
    print(f"\n[parity] 256x4000x8 mixture {model} 20 its: default (mixed, X-resident kernel) W vs c128 {e128:.2e}, vs reference-c64 {e64:.2e} "
          f"(floor {floor:.2e}), Y {eY:.2e}; fast W vs c128 {efast:.2e}")
    assert e64 < max(TOL, 1.5 * floor) and e128 < max(TOL, 0.5 * floor) and eY < max(TOL, 0.5 * floor)
    assert efast < max(TOL, FAST_FLOORS * floor)


@pytest.mark.parametrize("mode", ["mixed", "precise", "fast"])
def test_cfg5_shape_full_frame_axis(oa, mode):
    """BASELINE.json configs[4] shape at full T with few bins: 8 bins x 4000 frames x 16 mics / 16 src, in every arithmetic
    -- `mixed` is what bench.py times and overiva() runs on it: cov_hmfma_kernel<true> (all 16 sources on the fp32 matrix
    cores, Hermitian products from LDS partners, float32 chains over the frame splits, float64 partials), the matrix-core
    power pass of > 4 sources (8 bins: power_mfma_kernel; 64 bins or more: power_lds_kernel) and update_det16r_kernel
    (w = V_s^-1 u by one elimination per source with recorded multipliers, C = (W_hat^H)^-1 kept by rank-one steps);
    `precise`: cov_hmfma64_kernel (the same GEMM on the fp64 matrix cores); `fast`: float32 per-bin algebra"""
    T, F, M, K = 4000, 8, 16, 16
    X = orc.synth_iid(T, F, M, seed=5)
    oa.set_precision(mode)
    try:
        Y, W = oa.overiva(X, n_src=K, n_iter=3, proj_back=False, return_filters=True)
    finally:
        oa.set_precision("auto")
    Yr, Wr = orc.overiva_staged(X, n_src=K, n_iter=3, proj_back=False, return_filters=True)
    eW, eY = orc.rel_err(W, Wr), orc.rel_err(Y, Yr)
    _log(test="cfg5", fixture="T4000F8M16K16 iid", model="laplace", n_iter=3, input="c64", mode=mode, W_vs_c128=eW, Y_vs_c128=eY)
    print(f"\n[parity] cfg5 shape (8 bins) iid 3 its {mode}: W err {eW:.2e}  Y err {eY:.2e}")
    assert eW < TOL and eY < TOL


def test_headline_size_properties(oa):
    """2048 bins x 4000 frames x 8 mics / 2 src (BASELINE.json configs[2]): invariants that need no
    oracle, plus a spot check of a few bins against the oracle."""
    T, F, M, K = 4000, 2048, 8, 2
    X = orc.synth_iid(T, F, M, seed=0)
    with oa.Plan(T, F, M, K, "laplace") as p:
        p.set_x(X)
        p.covariance()
        p.set_w(None)
        p.set_fuse_cov_update(False)                   # (the one-launch form keeps the covariances in LDS: this test looks at them)
        p.iterate(3)
        rinv, wscale = p.t_get_rinv()
        What = p.t_get_what().astype(np.complex128)
        V = p.t_get_v().astype(np.complex128)          # covariances of the last iteration
        Cx = p.get_cx().astype(np.complex128)
        W = p.get_w()
    assert np.all(np.isfinite(W))
    # mean_t r = 1 before the eps floor (overiva.py:158-159)
    assert abs(np.mean(1.0 / rinv.astype(np.float64), axis=0) - 1.0).max() < 1e-5
    # w_s^H V_s w_s = 1 for the last-updated source (overiva.py:185-186)
    s = K - 1
    w = What[:, :, s]
    q = np.einsum("fc,fcd,fd->f", np.conj(w), V[s], w)
    assert np.abs(q - 1.0).max() < 1e-4
    # orthogonality constraint W^H Cx [J; -I] = 0 (overiva.py:96-98, :123)
    R = np.conj(np.swapaxes(What[:, :, :K], 1, 2)) @ Cx @ What[:, :, K:]
    scale = np.abs(np.conj(np.swapaxes(What[:, :, :K], 1, 2)) @ Cx).max()
    assert np.abs(R).max() < 1e-4 * scale
    # spot check: covariances of 3 bins against the oracle, given the device's own r_inv
    for f in (0, 1023, 2047):
        ref = orc.weighted_cov_all(X[:, f:f + 1, :], rinv.astype(np.float64))[:, 0]
        assert orc.rel_err(V[:, f], ref) < TOL_KERNEL
    # and the whole run against the oracle on a bin subset is impossible (r couples all bins); instead
    # the activation itself: r from the device's W before the last iteration is covered by
    # test_activation at small sizes; here only its normalisation is checked (above).


@pytest.mark.parametrize("mode", ["mixed", "fast", "precise"])
def test_cfg5_full_size_properties(oa, mode):
    """2048 bins x 4000 frames x 16 mics / 16 src (BASELINE.json configs[4]) at FULL size, in the geometry and the arithmetic
    bench.py times -- `mixed`: cov_hmfma_kernel<true> (the sources on the fp32 matrix cores, 4 frame splits, float64 partials),
    power_lds_kernel, update_det16r_kernel (one matrix row per lane, three waves per four bins: 512 workgroups); `precise`:
    cov_hmfma64_kernel + the same update; `fast`: cov_hmfma_kernel + update_wave16_kernel<float> -- invariants that need no
    oracle, the covariances of three bins against the oracle, and the per-bin update of those bins (overiva.py:181-190, all
    16 sources) against orc.ip_update_bin from the device's own covariances"""
    T, F, M, K = 4000, 2048, 16, 16
    X = orc.synth_iid(T, F, M, seed=2)
    bins = (0, 1023, 2047)
    with oa.Plan(T, F, M, K, "laplace") as p:
        p.set_precision(mode)
        p.set_x(X)
        p.covariance()
        p.set_w(None)
        p.iterate(2)
        rinv, wscale = p.t_get_rinv()
        What = p.t_get_what(np.complex128)
        V = p.t_get_v(np.complex128)                       # covariances of the last iteration, (K, F, M, M)
        W = p.get_w()
        # the update kernel alone, at this geometry: W_hat as it stands, covariances from given weights, one update
        Cx = p.get_cx(np.complex128)
        rinv2 = np.random.default_rng(9).gamma(2.0, 1.0, (T, K)).astype(np.float32)
        p.t_set_rinv(rinv2)
        p.t_run_weighted_cov()
        V2 = p.t_get_v(np.complex128)
        p.t_run_update()
        What2 = p.t_get_what(np.complex128)
    assert np.all(np.isfinite(W)) and W.shape == (F, M, K)
    # mean_t r = 1 before the eps floor (overiva.py:158-159), every source
    assert abs(np.mean(1.0 / rinv.astype(np.float64), axis=0) - 1.0).max() < 1e-5
    # w_s^H V_s w_s = 1 for the last-updated source (overiva.py:185-186), every bin
    s = K - 1
    w = What[:, :, s]
    q = np.einsum("fc,fcd,fd->f", np.conj(w), V[s], w)
    assert np.abs(q - 1.0).max() < (1e-4 if mode == "fast" else 1e-9)      # (float64 algebra in `mixed` and `precise`)
    # V Hermitian
    assert np.abs(V[s] - np.conj(np.swapaxes(V[s], 1, 2))).max() < 1e-6 * np.abs(V[s]).max()
    # the covariances of three bins, all 16 sources, against the oracle given the device's own weights
    tol = 1e-6 if mode == "precise" else 5e-6      # (float32 products and chains in `fast` / `mixed`; the weights travel as float32 in all)
    for f in bins:
        ref = orc.weighted_cov_all(X[:, f:f + 1, :], rinv.astype(np.float64))[:, 0]
        assert orc.rel_err(V[:, f], ref) < tol
    # the update of those bins against the oracle's chain (IP1 solve, normalisation; no background at K = M)
    for f in bins:
        ref = orc.ip_update_bin(What[f:f + 1], V2[:, f:f + 1], Cx[f:f + 1], K)
        e = orc.rel_err(What2[f:f + 1], ref)
        print(f"\n[parity] cfg5 full size {mode}: update of bin {f} vs oracle {e:.2e}")
        assert e < (2e-5 if mode == "fast" else 1e-9)


@pytest.fixture(scope="module")
def headline_mixture():
    """2048 x 4000 x 8 / 2 mixture-like input and the oracle's results after 20 iterations: the reference's own arithmetic
    for complex64 input (reference-faithful form) and its complex128 result.  Two minutes of CPU work on the GPU box: taken
    from tests/golden/headline_mixture20.npz (written by make_headline_mixture.py from the same oracle calls) when the
    regenerated input has the digest stored there, computed here otherwise"""
    import importlib.util
    import os

    from conftest import GOLDEN_DIR

    spec = importlib.util.spec_from_file_location("make_headline_mixture", os.path.join(GOLDEN_DIR, "make_headline_mixture.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    (T, F, M, K), seed = mk.SHAPE, mk.SEED
    X = orc.synth_mixture(T, F, M, K, seed=seed)
    if os.path.exists(mk.OUT):
        with np.load(mk.OUT) as d:
            if str(d["x_digest"]) == mk.x_digest(X) and int(d["n_iter"]) == 20:
                return X, d["W64"], d["W128"]
    W64, W128 = mk.compute(X, K)
    return X, W64, W128


@pytest.mark.parametrize("mode,one_launch", [("mixed", False), ("fast", False), ("precise", False), ("mixed", True), ("fast", True)])
def test_headline_mixture_20_iterations(oa, headline_mixture, mode, one_launch, monkeypatch):
    """the headline shape (BASELINE.json configs[2]) on ill-conditioned mixture-like input for 20 iterations, every
    arithmetic mode, against the reference's own complex64 arithmetic (oracle, reference-faithful form): as close to it as
    its distance from the complex128 result (the floor) allows.  one_launch: through cov_update_kernel (see above)."""
    X, W64, W128 = headline_mixture
    K = 2
    floor = orc.rel_err(W64, W128)
    _one_launch_env(oa, monkeypatch, (X.shape[0], X.shape[1], X.shape[2], K), one_launch)
    oa.set_precision(mode)
    try:
        Y, W = oa.overiva(X, n_src=K, n_iter=20, proj_back=False, return_filters=True)
    finally:
        oa.set_precision("auto")
        oa.release_cached_buffers()
    e64, e128 = orc.rel_err(W, W64), orc.rel_err(W, W128)
    eY = orc.rel_err(Y, _demix(X, W128))
    _log(test="headline20" + ("-one-launch" if one_launch else ""), fixture="T4000F2048M8K2 mixture", model="laplace", n_iter=20, input="c64", mode=mode, W_vs_c128=e128,
         Y_vs_c128=eY, W_vs_ref_c64=e64, ref_c64_floor=floor)
    print(f"\n[parity] headline mixture 20 its {mode}: W vs reference-c64 {e64:.2e} (floor {floor:.2e}), vs c128 {e128:.2e}, Y {eY:.2e}")
    if mode == "fast":
        assert e128 < max(TOL, FAST_FLOORS * floor)
    else:
        assert e64 < max(TOL, 1.5 * floor) and e128 < max(TOL, floor) and eY < max(TOL, floor)


def test_plain_c_program_runs(oa, tmp_path):
    """examples/c_abi_demo.c: the C ABI driven from plain C on the GPU"""
    import os
    import subprocess

    from conftest import REPO

    exe = tmp_path / "c_abi_demo"
    pkg = os.path.join(REPO, "overiva_amd")
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), os.path.join(REPO, "examples", "c_abi_demo.c"),
                        "-L", pkg, "-loveriva_hip", f"-Wl,-rpath,{pkg}", "-lm", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "output energy" in run.stdout


def test_two_plans_are_independent_and_no_leak(oa):
    """distinct plans may be alive and interleaved; repeated create/destroy does not accumulate device memory"""
    import torch

    Xa = orc.synth_iid(128, 40, 4, seed=11)
    Xb = orc.synth_iid(96, 33, 3, seed=12)
    oa.set_precision("precise")
    os.environ["OIVA_RESIDENT"] = "0"          # the four-launch path, which the bare plans below run as well
    try:
        Ya = oa.overiva(Xa, n_src=2, n_iter=4, proj_back=False)
        Yb = oa.overiva(Xb, n_src=1, n_iter=4, proj_back=False)
    finally:
        oa.set_precision("auto")
        del os.environ["OIVA_RESIDENT"]
    pa = oa.Plan(128, 40, 4, 2)
    pb = oa.Plan(96, 33, 3, 1)
    pa.set_precision("precise"); pb.set_precision("precise")      # what overiva() used above
    pa.set_x(Xa); pb.set_x(Xb)
    pa.covariance(); pb.covariance()
    pa.set_w(None); pb.set_w(None)
    for _ in range(4):                      # interleaved iterations on two streams
        pa.iterate(1)
        pb.iterate(1)
    assert np.array_equal(pa.demix(False), Ya) and np.array_equal(pb.demix(False), Yb)
    pa.close(); pb.close()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(20):
        with oa.Plan(512, 256, 8, 2) as p:
            p.set_x(orc.synth_iid(512, 256, 8, seed=1))
            p.covariance(); p.set_w(None); p.iterate(2); p.demix(True)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < 64 << 20
