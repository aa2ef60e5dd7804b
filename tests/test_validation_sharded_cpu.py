"""Merge validation statistics for sharded runs, the parts that need no GPU: the entry points exist, and dropest_validation_cut_pairs --
how the pairs of one sample are dealt to the shards for evaluation -- against a restatement of its rule.

The rule: range r ends behind the first pair at which the running sum of cnt reaches (r + 1) * total / world (integer division); pairs
with cnt = 0 ride along (the last range takes what is left); total = 0 deals equal numbers of pairs.  From the rule: a range's sum stays
below its share plus one pair, sum <= total / world + max(cnt) (the sum before a range's last pair is below its target, the sum before
its first pair is at least the previous target, and two neighbouring targets lie at most ceil(total / world) apart)."""
import numpy as np
import pytest

from dropest_amd import capi
from dropest_amd.multi import Shard, ShardGroup


def test_entry_points_exist():
    L = capi.lib()
    for name in ("dropest_shard_merge_validation_samples", "dropest_shard_group_merge_validation_samples", "dropest_validation_cut_pairs"):
        assert name in capi.EXPORTED_SYMBOLS and hasattr(L, name), name
    assert callable(getattr(Shard, "merge_validation")) and callable(getattr(ShardGroup, "merge_validation"))


def restated(cnt, world):
    cnt = [int(x) for x in cnt]
    n, total = len(cnt), sum(cnt)
    if total == 0:
        return [n * r // world for r in range(world + 1)]
    bounds, run, p = [0], 0, 0
    for r in range(world):
        while p < n and run < (r + 1) * total // world:
            run += cnt[p]
            p += 1
        bounds.append(p)
    bounds[world] = n
    return bounds


def check(cnt, world):
    cnt = np.asarray(cnt, np.uint32)
    bounds = capi.validation_cut_pairs(cnt, world)
    assert bounds == restated(cnt, world), (list(cnt[:16]), world)
    assert len(bounds) == world + 1 and bounds[0] == 0 and bounds[-1] == len(cnt)
    assert all(a <= b for a, b in zip(bounds, bounds[1:]))
    total, top = int(cnt.sum(dtype=np.uint64)), int(cnt.max()) if len(cnt) else 0
    for a, b in zip(bounds, bounds[1:]):
        assert int(cnt[a:b].sum(dtype=np.uint64)) <= total / world + top
    return bounds


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_cut_pairs_edges(world):
    assert check(np.zeros(10, np.uint32), world) == [10 * r // world for r in range(world + 1)]     # no common gene anywhere: equal counts
    check([7], world)                                                                              # one pair
    check([0], world)
    check([], world)
    check([3, 1, 2], 8)                                                                            # more shards than pairs
    big = check([1, 2, 1000, 3, 1, 1, 2], world)                                                   # one pair outweighs all the others
    assert sum(1 for a, b in zip(big, big[1:]) if a <= 2 < b) == 1                                 # ... and lies in exactly one range
    check([0, 0, 5, 0, 0, 5, 0, 0], world)                                                         # empty pairs ride along
    check([0xFFFFFFFF] * 5, world)                                                                 # sums beyond 32 bits


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_cut_pairs_random(world):
    rng = np.random.default_rng(20261019 + world)
    cnt = rng.integers(0, 50, 1000).astype(np.uint32)
    cnt[rng.random(1000) < 0.3] = 0
    bounds = check(cnt, world)
    assert all(b > a for a, b in zip(bounds, bounds[1:]))                                          # 1000 pairs: nobody idles
    check(rng.integers(0, 1 << 20, 1000), world)


def test_cut_pairs_refuses_bad_arguments():
    L = capi.lib()
    out = np.zeros(4, np.uint64)
    assert L.dropest_validation_cut_pairs(None, 3, 2, out.ctypes.data) == 1                        # INVALID
    assert L.dropest_validation_cut_pairs(None, 0, 0, out.ctypes.data) == 1
    assert L.dropest_validation_cut_pairs(None, 0, 2, None) == 1
