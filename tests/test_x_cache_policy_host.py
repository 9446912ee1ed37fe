"""Host-side checks of the load policy of X (csrc/kernel_choice.h::choose_x_policy, through the host-only hook
oiva_test_x_policy): which frames the two streaming passes read with plain loads, so that they may stay in the last-level cache,
and which they stream non-temporally.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

REASONS = ("off", "fits", "kernels", "geometry", "share")
F, M = 2048, 8


@pytest.fixture(scope="module")
def lib():
    from overiva_amd import build, _lib

    build.build_library()
    return _lib.load()


def _policy(lib, T, ctc, tcp, budget_mb, F=F, M=M):
    out = (C.c_int * 3)()
    cov = np.empty(T, np.int8)
    pw = np.empty(T, np.int8)
    assert lib.oiva_test_x_policy(T, F, M, ctc, tcp, float(budget_mb), out, cov.ctypes.data, pw.ctypes.data) == 0
    return out[0], bool(out[1]), REASONS[out[2]], cov, pw


def _geometries():
    """(T, frames per covariance split, frames per power chunk)"""
    yield 4000, 1008, 336             # the headline shape: 4 splits, 12 chunks
    yield 4000, 512, 168              # the 1024-bin shard: 8 splits, 24 chunks
    yield 4000, 288, 84               # the 512-bin shard: 14 splits
    yield 517, 528, 44                # T no multiple of 16, one split
    yield 517, 272, 44
    yield 517, 144, 44
    yield 70, 80, 12
    yield 333, 96, 32
    yield 1040, 272, 36               # chunks that start 4 frames into a group
    yield 1040, 528, 36
    yield 203, 80, 36
    yield 235, 80, 32
    yield 64, 64, 64                  # one chunk, as long as the split
    yield 50, 64, 52                  # a chunk longer than the frame axis
    yield 1000, 512, 500
    yield 2048, 512, 128              # whole periods
    yield 4001, 1008, 336


GEOMS = list(_geometries())


def _x_mb(T, F=F, M=M):
    return T * F * M * 8 / 1e6


@pytest.mark.parametrize("T,ctc,tcp", GEOMS)
@pytest.mark.parametrize("share", [0.03, 0.07, 0.3, 0.5, 0.77, 0.97])
def test_every_frame_has_one_policy_in_both_passes(lib, T, ctc, tcp, share):
    n16, nt, why, cov, pw = _policy(lib, T, ctc, tcp, share * _x_mb(T))
    assert why == "share" and nt and 0 <= n16 <= 15
    # every frame met exactly once by each pass, and by both with the same policy: no step straddles two policies
    assert set(np.unique(cov)) <= {0, 1} and set(np.unique(pw)) <= {0, 1}
    assert np.array_equal(cov, pw)
    # the rule itself: groups of 16 frames counted from the start of the split, the first n16 of every 16 resident
    t = np.arange(T)
    want = (((t % ctc) // 16) % 16 >= n16).astype(np.int8)
    assert np.array_equal(cov, want)


@pytest.mark.parametrize("T,ctc,tcp", GEOMS)
@pytest.mark.parametrize("share", [0.03, 0.07, 0.3, 0.5, 0.77, 0.97])
def test_resident_bytes_are_within_one_group_of_the_budget(lib, T, ctc, tcp, share):
    """the share is n16 sixteenths of X, one group of every period of 16: as many as the budget holds, so less than one
    sixteenth below it.  Frame by frame: of a period that its split cuts short after r frames min(r, 16 n16) are resident
    where the sixteenths make r n16 / 16, never fewer and at most n16 (16 - n16) <= 64 frames more, once per split."""
    budget = share * _x_mb(T)
    n16, nt, why, cov, _ = _policy(lib, T, ctc, tcp, budget)
    assert n16 / 16 * _x_mb(T) <= budget < (n16 + 1) / 16 * _x_mb(T)
    resident = int((cov == 0).sum())
    splits = -(-T // ctc)
    assert 0 <= resident - n16 / 16 * T <= n16 * (16 - n16) * splits
    if ctc % 256 == 0 and T % ctc == 0:
        assert resident * 16 == n16 * T


@pytest.mark.parametrize("T,ctc,tcp", GEOMS)
def test_off_and_fits_are_all_plain(lib, T, ctc, tcp):
    for budget, reason, n in ((0., "off", 0), (-1., "off", 0), (_x_mb(T), "fits", 16), (1e6, "fits", 16)):
        n16, nt, why, cov, pw = _policy(lib, T, ctc, tcp, budget)
        assert (n16, nt, why) == (n, False, reason)
        assert not cov.any() and not pw.any()


@pytest.mark.parametrize("T,ctc,tcp,M,why", [
    (4000, 1000, 336, 8, "geometry"),     # splits that do not start on a group
    (4000, 144, 336, 8, "geometry"),      # a chunk that crosses more than one split boundary
    (4000, 1008, 336, 4, "kernels"),      # the streamed form of the two passes exists at 8 channels
    (4000, 1008, 336, 6, "kernels"),
    (4000, 1008, 336, 7, "kernels"),
])
def test_share_zero_where_a_step_could_straddle(lib, T, ctc, tcp, M, why):
    n16, nt, reason, cov, pw = _policy(lib, T, ctc, tcp, 0.3 * _x_mb(T, M=M), M=M)
    assert (n16, nt, reason) == (0, False, why)
    assert not cov.any() and not pw.any()


def test_headline_share(lib):
    """2048 bins x 4000 frames x 8 channels: 524 MB of X, sixteenths of 32.8 MB"""
    n16, nt, why, cov, _ = _policy(lib, 4000, 1008, 336, 200.)
    assert (n16, nt, why) == (6, True, "share")
    assert int((cov == 0).sum()) == 4 * (3 * 96 + 96)      # 201.3 MB: splits of 3 periods and 15 groups


def test_bad_arguments_are_refused(lib):
    out = (C.c_int * 3)()
    buf = np.empty(16, np.int8)
    assert lib.oiva_test_x_policy(0, F, M, 16, 4, 1., out, buf.ctypes.data, buf.ctypes.data) != 0
    assert lib.oiva_test_x_policy(16, F, M, 16, 4, 1., None, buf.ctypes.data, buf.ctypes.data) != 0
    assert lib.oiva_test_x_policy(16, F, M, 16, 4, 1., out, None, buf.ctypes.data) != 0
