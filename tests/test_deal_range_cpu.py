"""dropest_deal_range: the one statement of how a feeder deals a stream to shards (read k belongs to shard
min(n_shards - 1, k // quota)), against a model of three lines.  Host logic: no GPU."""
import ctypes as C

import pytest

from dropest_amd import capi


def _model(first, n, quota, shards):
    """The pieces as (shard, offset, count): runs of equal min(shards - 1, ordinal // quota) over the n ordinals from `first`."""
    owner = [min(shards - 1, (first + i) // quota) for i in range(n)]
    starts = [i for i in range(n) if i == 0 or owner[i] != owner[i - 1]]
    return [(owner[a], a, (starts[k + 1] if k + 1 < len(starts) else n) - a) for k, a in enumerate(starts)]


CASES = [
    # (first_ordinal, n, quota, n_shards)
    (0, 100, 100, 3),        # ends exactly on a quota boundary: one piece, nothing for shard 1
    (50, 150, 100, 3),       # ... from inside a shard to the end of the next
    (100, 100, 100, 3),      # begins and ends on boundaries
    (90, 120, 100, 4),       # crosses two boundaries: 10 + 100 + 10
    (0, 7001 * 2 + 5, 7001, 3),
    (250, 500, 100, 3),      # starts in the last shard: no cut beyond it
    (199, 500, 100, 3),      # one read before the last shard
    (0, 0, 100, 3),          # n = 0: no piece
    (777, 0, 100, 3),
    (3, 9, 1, 5),            # a quota of 1: a piece per read until the last shard
    (0, 4, 1, 8),
    (0, 1000, 10, 3),        # quota x shards smaller than the run: the last shard takes the rest
    (25, 1000, 10, 3),
    (0, 10, 100, 1),         # one shard
    (12345, 1, 7001, 3),
]


@pytest.mark.parametrize("first,n,quota,shards", CASES)
def test_pieces_equal_the_model(first, n, quota, shards):
    got = capi.deal_range(first, n, quota, shards)
    assert got == _model(first, n, quota, shards)
    assert sum(c for _, _, c in got) == n and all(c > 0 for _, _, c in got) and len(got) <= shards
    assert [s for s, _, _ in got] == sorted(set(s for s, _, _ in got))      # ascending, every shard once


def test_ordinals_beyond_32_bits():
    q = (1 << 33) + 7
    assert capi.deal_range(q - 2, 5, q, 4) == [(0, 0, 2), (1, 2, 3)]
    assert capi.deal_range(3 * q + 1, 1 << 40, q, 4) == [(3, 0, 1 << 40)]


def test_bad_arguments_are_refused():
    L = capi.lib()
    out = (C.c_uint64 * 9)()
    k = C.c_uint32(77)
    assert L.dropest_deal_range(0, 10, 0, 3, out, C.byref(k)) == 1          # a quota of 0
    assert L.dropest_deal_range(0, 10, 5, 0, out, C.byref(k)) == 1          # no shard
    assert L.dropest_deal_range(0, 10, 5, 3, None, C.byref(k)) == 1
    assert L.dropest_deal_range(0, 10, 5, 3, out, None) == 1
    assert L.dropest_deal_range(0, 0, 5, 3, None, C.byref(k)) == 0 and k.value == 0      # nothing to write: no array needed
