"""Host-side checks of the order in which the power pass takes its frame chunks (csrc/oiva_internal.h::power_chunk_tail_first,
through the host-only hook oiva_test_power_order): no GPU needed."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from overiva_amd import build, _lib

    build.build_library()
    return _lib.load()


def _order(lib, n, tcp, cs, ctc):
    out = (C.c_int * n)()
    assert lib.oiva_test_power_order(n, tcp, cs, ctc, out) == 0
    return list(out)


def _geometries():
    yield 4000, 336, 4, 1000          # the headline shape: 12 chunks against 4 splits
    yield 4000, 168, 4, 1000          # the 1024-bin shard: 24 chunks
    yield 517, 44, 1, 528
    yield 517, 44, 2, 272
    yield 517, 44, 4, 144
    yield 64, 64, 1, 64               # one chunk
    yield 203, 36, 3, 80
    yield 1000, 500, 7, 144           # more splits than chunks: splits that own no chunk
    yield 4000, 32, 28, 144
    yield 235, 32, 3, 80
    for T in (1, 5, 97, 1024):
        for tcp in (4, 12, 100):
            for cs in (1, 2, 3, 5, 16):
                yield T, tcp, cs, -(-(-(-T // cs)) // 16) * 16


@pytest.mark.parametrize("T,tcp,cs_req,ctc", list(_geometries()))
def test_order_is_a_bijection_and_runs_from_the_tails_to_the_heads(lib, T, tcp, cs_req, ctc):
    n = -(-T // tcp)
    cs = -(-T // ctc)                 # the splits the covariance pass really has
    order = _order(lib, n, tcp, cs, ctc)
    assert sorted(order) == list(range(n))
    # the split a chunk belongs to: the one that holds its last frame
    split = [min(cs - 1, (min(T, (c + 1) * tcp) - 1) // ctc) for c in range(n)]
    owned = {s: [c for c in range(n) if split[c] == s] for s in range(cs)}
    # rank of a chunk from the tail of its split; the dispatch order never takes a chunk before the ones behind it in its own
    # split, and never goes a full row deeper into one split while another still has a shallower chunk left
    rank = {c: len(owned[split[c]]) - 1 - owned[split[c]].index(c) for c in range(n)}
    ranks = [rank[c] for c in order]
    assert ranks == sorted(ranks)
    # first row: the last chunk of every split that owns one
    tails = {owned[s][-1] for s in range(cs) if owned[s]}
    assert set(order[:len(tails)]) == tails


def test_bad_arguments_are_refused(lib):
    out = (C.c_int * 4)()
    assert lib.oiva_test_power_order(0, 4, 1, 16, out) != 0
    assert lib.oiva_test_power_order(4, 4, 0, 16, out) != 0
    assert lib.oiva_test_power_order(4, 4, 1, 16, None) != 0
