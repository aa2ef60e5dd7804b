"""dropest_shard_push_reads_device: a shard's resident reads appended from DEVICE columns (what the device BAM path hands a sharded
container) give exactly the run of the same stream pushed from host memory -- uneven pieces, a piece that ends on a shard boundary, host and
device pushes on one shard, and a push that leaves a gap refused without a trace."""
import os

import numpy as np
import pytest

from dropest_amd import capi
from dropest_amd.multi import ShardGroup, cfg_kwargs
from dropest_amd.synth import SynthStream, inject_n

import parity

pytestmark = pytest.mark.gpu

DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dropest_amd", "data", "barcodes")
N = 40_000
PIECES = [1, 4095, 4097]                                  # ... and the rest
# where a shard's range ends: 4096 = the end of the second piece; world 3 cuts the last piece once more
BOUNDS = {2: [0, 4096, N], 3: [0, 4096, 25_001, N]}
_cache = {}


def _stream():
    """The stream (whitelist neighbours to merge, UMIs with N whose fate depends on stream ordinals), made once."""
    if "stream" not in _cache:
        s = SynthStream(n_reads=N, n_cells=20, n_genes=500, umi_len=8, permille_neighbour=150)
        cb, umi, gene, aux = parity.canonical_stream(*s.generate_host())
        umi, side = inject_n(umi, gene, 5e-3, 11, 8)
        kw = cfg_kwargs({"min_before": 3, "min_after": 10, "merge": {"barcodes_kind": capi.BARCODES_CONST, "barcodes_file": os.path.join(DATA, "10x_aug_2016_split")}})
        _cache["stream"] = ((cb, umi, gene, aux), side, kw)
    return _cache["stream"]


def _pieces(world):
    """(shard, begin, end) of every push: the pieces 1, 4095, 4097, rest, cut where a shard's range ends."""
    cuts = sorted(set(np.cumsum([0] + PIECES).tolist() + BOUNDS[world]))
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        shard = max(k for k in range(world) if BOUNDS[world][k] <= a)
        out.append((shard, a, b))
    return out


def _result(g):
    g.step()
    s0 = g.shards[0]
    got = {"cm": [x.copy() for x in s0.matrix(True)], "raw": [x.copy() for x in s0.matrix(False)], "merged": [x.copy() for x in s0.merged_barcodes()]}
    g.close()
    return got


def _host_reference(world):
    """The same pieces from host memory (dropest_shard_push_reads), once per world."""
    if world not in _cache:
        arrays, side, kw = _stream()
        g = ShardGroup([0] * world, **kw)
        for sh in g.shards:
            sh.set_side_strings(side)
        for shard, a, b in _pieces(world):
            g.shards[shard].push_reads(*[x[a:b] for x in arrays], a)
        _cache[world] = _result(g)
    return _cache[world]


def _same(got, want):
    for name in ("cm", "raw"):
        assert len(got[name]) == len(want[name]) == 4
        for x, y in zip(got[name], want[name]):      # colptr, rowidx, values, column barcodes
            assert np.array_equal(x, y), name
    assert np.array_equal(got["merged"][0], want["merged"][0]) and np.array_equal(got["merged"][1], want["merged"][1])


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("world", [2, 3])
def test_device_pieces_equal_host_pieces(world, mixed):
    """mixed: the second and the third push come from host memory -- shard 0 takes a device push and then a host push, shard 1 a host push and then a
    device push."""
    arrays, side, kw = _stream()
    want = _host_reference(world)
    assert want["cm"][0][-1] > 1000 and len(want["merged"][0]) > 0 and len(want["raw"][3]) >= len(want["cm"][3]) >= 10      # (the stream has cells to merge and columns to compare)
    pieces = _pieces(world)
    assert [b - a for _, a, b in pieces][:3] == PIECES and any(b == BOUNDS[world][1] for _, a, b in pieces)      # a piece ends where shard 0's range does
    dev = capi.DeviceArrays.from_host(0, *arrays)
    g = ShardGroup([0] * world, **kw)
    try:
        for sh in g.shards:
            sh.set_side_strings(side)
        kinds = []
        for k, (shard, a, b) in enumerate(pieces):
            from_host = mixed and k in (1, 2)
            if from_host:
                g.shards[shard].push_reads(*[x[a:b] for x in arrays], a)
            else:
                g.shards[shard].push_device(dev, a, offset=a, n=b - a)
            kinds.append((shard, "host" if from_host else "device"))
        if mixed:
            assert [k for s, k in kinds if s == 0] == ["device", "host"] and [k for s, k in kinds if s == 1][:2] == ["host", "device"]
        # a push that does not continue the shard's range: invalid argument, and the shard is what it was (the result below says so)
        for first in (BOUNDS[world][1] + 1, BOUNDS[world][1] - 1, 0):
            with pytest.raises(capi.DropestError) as e:
                g.shards[0].push_device(dev, first, offset=0, n=10)
            assert e.value.status == 1 and "without a gap" in str(e.value)
        with pytest.raises(capi.DropestError) as e:      # null arrays
            g.shards[0]._chk(g.shards[0].L.dropest_shard_push_reads_device(g.shards[0].h, None, None, None, None, 10, BOUNDS[world][1], 0, None))
        assert e.value.status == 1
        got = _result(g)
    finally:
        g.close()
        dev.free()
    _same(got, want)
