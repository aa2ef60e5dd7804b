"""The directional UMI correction on the device (k_umi_directional.h, umi_directional_host.h) against the plain model
(directional_model.py, pinned on the oracle by test_directional_model_cpu.py) on the hand-built cases of directional_cases.py.

  targets    umi_merge_targets() as {(cell, gene): {source: target}} equals the model's per-group targets, the groups that must be absent
             included
  container  molecules() and the total_umis column of cell_rows() equal the model's; every observable equals the oracle's
  routes     count:umi_groups_host / _wave / _huge / umi_rekeyed of kernel_stats() are the numbers the case declares
  layouts    the cases at the 16/17 line, in the heapsort and at max_ed 2 and 3 once more under the forced sort layouts
  reads      the UMI every read is written under (read_corrections(), the -F decisions) equals the model's: the surviving UMI, read by read
  shards     every case the device decides through 2 and 3 in-process shards: the oracle's matrices, the one context's, and -- since ties
             leave the same COUNTS whichever UMI survives -- the model's written UMI of every read from the group's read_corrections()

One fresh context per case, profiling on.  Everything compared is an integer, a string or a set: nothing here has a tolerance."""
import ctypes
from functools import lru_cache

import numpy as np
import pytest

from dropest_amd import capi
from dropest_amd.multi import ShardGroup
import directional_cases as dc
import directional_model as dm
import parity
from test_directional_model_cpu import oracle_of
from test_gpu_multi_oracle import check_vs_oracle, even_bounds

pytestmark = pytest.mark.gpu

_libc = ctypes.CDLL("libc.so.6")
WRITTEN = 0                                     # verdict of a read that -F writes (filtered_model.py)
COUNTS = {"host": "count:umi_groups_host", "wave": "count:umi_groups_wave", "huge": "count:umi_groups_huge"}


def run_on_device(name):
    """merge_and_filter over the case's stream in a fresh context (rand() starts from srand(1), as in a fresh reference process), every
    observable compared with the oracle's, and what the tests below look at"""
    c = dc.case(name)
    o = oracle_of(name)
    _libc.srand(1)
    ctx = capi.Context(**c.kw())
    try:
        ctx.set_profiling(True)
        ctx.set_save_umi_merge_targets(True)
        if c.side:
            ctx.set_side_strings(c.side)
        ctx.push_reads(*c.arrays())
        ctx.set_initialized()
        ctx.merge_and_filter()
        out = {"targets": {}}
        rows = list(zip(*[x.tolist() for x in ctx.umi_merge_targets()]))
        assert [r[:3] for r in rows] == sorted({r[:3] for r in rows})                    # ascending (cell, gene, source code), one row per source
        for cell, gene, src, tgt in rows:
            out["targets"].setdefault((cell, gene), {})[capi.unpack_code(src, c.side)] = capi.unpack_code(tgt, c.side)
        cell, gene, umi, reads, _ = ctx.molecules()
        out["molecules"] = {(int(a), int(b), capi.unpack_code(u, c.side)): int(r) for a, b, u, r in zip(cell, gene, umi, reads)}
        assert len(out["molecules"]) == len(cell)
        cells = ctx.cell_rows()
        out["total_umis"] = {i: int(x) for i, x in enumerate(cells["total_umis"])}
        stats = ctx.kernel_stats()
        out["counts"] = {k: int(stats[k]["launches"]) for k in list(COUNTS.values()) + ["count:umi_rekeyed"]}
        out["kernels"] = set(stats)
        out["written"] = written(ctx.read_corrections(), c.side)
        out["matrices"] = {}
        for filtered in (True, False):
            columns = [int(k) for k in ctx.filtered_cells()] if filtered else [int(k) for k in np.flatnonzero(cells["is_real"])]
            out["matrices"][filtered] = ([x.tolist() for x in ctx.count_matrix(filtered=filtered)],
                                         [capi.unpack_code(int(cells["barcode"][k]), c.side) for k in columns])
        parity.compare(o, ctx, c.side)
    finally:
        ctx.close()
    return out


device_run = lru_cache(maxsize=None)(run_on_device)


def written(corrections, side):
    """per read: the UMI it is written under, None if it is not written"""
    verdict, _, umi = corrections
    return [capi.unpack_code(int(u), side) if v == WRITTEN else None for v, u in zip(verdict.tolist(), umi.tolist())]


def check_against_the_model(name, got):
    want = dc.expected(name)
    assert got["targets"] == want.targets, (name, sorted(set(got["targets"]) ^ set(want.targets))[:5],
                                            [(k, sorted(set(got["targets"][k].items()) ^ set(want.targets[k].items()))[:6])
                                             for k in want.targets if k in got["targets"] and got["targets"][k] != want.targets[k]][:3])
    assert got["molecules"] == want.molecules
    assert got["total_umis"] == want.total_umis
    assert got["written"] == dm.written_umis(dc.case(name), want)


def check_routes(name, got):
    c = dc.case(name)
    assert {r: got["counts"][k] for r, k in COUNTS.items()} == {r: c.routes[r] for r in COUNTS}, name
    assert got["counts"]["count:umi_rekeyed"] == c.rekeyed, name
    assert "umi_directional" in got["kernels"]
    assert ("umi_directional:big" in got["kernels"]) == (c.routes["wave"] > 0) and ("umi_directional:huge" in got["kernels"]) == (c.routes["huge"] > 0)


@pytest.mark.parametrize("name", dc.MODELLED)
def test_device_equals_the_model(name):
    check_against_the_model(name, device_run(name))


@pytest.mark.parametrize("name", dc.NAMES)
def test_routes_are_the_declared_ones(name):
    check_routes(name, device_run(name))


@pytest.mark.parametrize("name", dc.HOST)
def test_host_routes_equal_the_oracle(name):
    """An N-UMI, UMIs of two lengths: the host's replay (the model is not asked).  device_run compared every observable with the oracle's;
    the targets the context kept are those that turn the stream's molecules into the oracle's."""
    got = device_run(name)
    o = oracle_of(name)
    cell, gene, umi, reads, _ = o.molecules()
    assert got["molecules"] == {(int(a), int(b), u): int(r) for a, b, u, r in zip(cell, gene, umi, reads)}
    assert sum(len(t) for t in got["targets"].values()) > got["counts"]["count:umi_rekeyed"]        # the host re-keyed something as well


def test_the_heapsort_ran_with_ties_that_matter():
    """heap_fallback_64 is one wave group whose introsort reaches the heapsort (the model's does, and the model's order is the oracle's
    std::sort's): a device that sorted stably, or left the heapsort's range to a stable sort, would report other targets."""
    got = device_run("heap_fallback_64")
    assert got["counts"]["count:umi_groups_wave"] == 1 and got["counts"]["count:umi_groups_huge"] == 0
    c = dc.case("heap_fallback_64")
    for variant in ("stable_sort", "no_heap_fallback"):
        assert got["targets"] != dm.run(c, {variant}).targets


@pytest.mark.parametrize("env", ["DROPEST_FORCE_BYTE_VALUES", "DROPEST_FORCE_GENERAL_LAYOUT"])
@pytest.mark.parametrize("name", dc.LAYOUT_CASES)
def test_layouts(name, env, monkeypatch):
    monkeypatch.setenv(env, "1")
    got = run_on_device(name)
    check_against_the_model(name, got)
    check_routes(name, got)


def shards_run(c, arrays, bounds):
    """test_gpu_multi_oracle.run_shards with the UMI merge targets kept, and the group's read corrections beside the matrices"""
    g = ShardGroup([0] * (len(bounds) - 1), **c.kw())
    try:
        for i, s in enumerate(g.shards):
            if c.side:
                s.set_side_strings(c.side)
            s.ctx.set_save_umi_merge_targets(True)
            s.set_reads(capi.DeviceArrays.from_host(0, *[a[bounds[i]:bounds[i + 1]] for a in arrays]), bounds[i])
        g.step()
        s0 = g.shards[0]
        return {"cm": [x.copy() for x in s0.matrix(True)], "raw": [x.copy() for x in s0.matrix(False)], "merged": s0.merged_barcodes(),
                "written": written(g.read_corrections(), c.side)}
    finally:
        g.close()


def triplets(matrix):
    p, i, x, _ = matrix
    col = np.repeat(np.arange(len(p) - 1), np.diff(p.astype(np.int64)))
    return [i.tolist(), col.tolist(), x.tolist()]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", dc.MODELLED)
def test_shards_equal_the_oracle_and_the_one_context(name, world):
    """index_order is the case that needs the UMI index of the whole stream (globalize_umi_first): its bounds put the earlier sightings on
    the first shard and the deciding groups on the last (asserted in test_directional_model_cpu.py, and here)."""
    c = dc.case(name)
    arrays = c.arrays()
    bounds = c.cuts[world] if c.cuts else even_bounds(len(arrays[0]), world)
    if name == "index_order":
        genes = [g for _, g, _ in c.reads]
        assert {"early", "other", None} <= set(genes[:bounds[1]]) and not {"cell", "gene", "geneless"} & set(genes[:bounds[-2]])
        owners = [int(capi.lib().dropest_owner_of(dc.pack(dc.barcode(k)), world)) for k in (dc.SIGHTING_CELL, 1)]
        assert owners == [dc.owner(k, world) for k in (dc.SIGHTING_CELL, 1)] and owners[0] != owners[1]   # ... and after the exchange by barcode
    got = shards_run(c, arrays, bounds)
    check_vs_oracle(got, oracle_of(name), tuple(c.side))
    want = dc.expected(name)
    assert got["written"] == dm.written_umis(c, want)                    # which UMI survived, read by read
    one = device_run(name)
    for filtered, key in ((True, "cm"), (False, "raw")):
        matrix, barcodes = one["matrices"][filtered]
        assert triplets(got[key]) == matrix, key
        assert [capi.unpack_code(int(b), c.side) for b in got[key][3]] == barcodes, key
    if name == "index_order":    # the count matrix shows the index order by itself: X and Z, X and Z, Z alone
        p, i, x, b = got["raw"]
        column = [capi.unpack_code(int(k), c.side) for k in b].index(dc.barcode(1))
        umis_of = dict(zip(i[p[column]:p[column + 1]].tolist(), x[p[column]:p[column + 1]].tolist()))
        assert [umis_of[want.stream.genes[g]] for g in dc.INDEX_ORDER_GENES] == [2, 2, 1]
