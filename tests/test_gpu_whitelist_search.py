"""The two whitelist search kernels (k_merge.h: wl_table_search_kernel, wl_neighbours_kernel; merge_host.h:
search_merge_candidates) against the plain model of the reference's search (whitelist_model.py, pinned on the oracle
by test_whitelist_model_cpu.py), base by base.

capi.Context.shard_merge_search hands the search a universe of cells as host arrays and returns its (base, candidate)
pairs, so every candidate of every base is compared -- missing, extra and doubled ones too, not only the one that wins
a merge.  Every case (whitelist_cases.py) runs on two fresh contexts: as is, and under DROPEST_WL_NO_TABLE=1 (read when
the whitelist is uploaded), where every base takes the full search.  Both must equal the model exactly; the route each
base took is checked from kernel_stats(): count:wl_bases_full_search and the presence of wl_table_search / wl_neighbours."""
import numpy as np
import pytest

from dropest_amd import capi

import whitelist_cases as wc
import whitelist_model as wm

pytestmark = pytest.mark.gpu


def run_search(c, tmp_path, monkeypatch, no_table):
    """-> (pair bases, pair candidates, kernel stats) of one search on a fresh context"""
    if no_table:
        monkeypatch.setenv("DROPEST_WL_NO_TABLE", "1")
    else:
        monkeypatch.delenv("DROPEST_WL_NO_TABLE", raising=False)
    path = tmp_path / ("wl_no_table" if no_table else "wl")
    path.write_text(wm.whitelist_text(c.parts))
    u = c.universe
    side, codes = [], []
    for t in u.barcode:
        code = capi.pack_seq(t)
        if code is None:
            side.append(t)
            code = capi.ESCAPE | (len(side) - 1)
        codes.append(code)
    ctx = capi.Context(merge_kind=capi.MERGE_POISSON_REAL if c.poisson else capi.MERGE_REAL_BARCODES, barcodes_kind=c.kind,
                       barcodes_file=str(path), min_genes_before_merge=c.min_genes, min_genes_after_merge=0)
    try:
        ctx.set_profiling(True)
        if side:
            ctx.set_side_strings(side)
        one = np.array([capi.pack_seq("".join(part[0] for part in c.parts))], np.uint64)      # a read that fits the whitelist
        ctx.push_reads(one, np.array([capi.pack_seq("ACGTAC")], np.uint64), np.zeros(1, np.uint32), np.full(1, 2 << 16, np.uint32))
        ctx.set_initialized()
        pb, pc = ctx.shard_merge_search(np.array(codes, np.uint64), u.n_genes, u.total_umis, c.bases, np.zeros(len(c.bases), np.uint32))
        return [int(x) for x in pb], [int(x) for x in pc], ctx.kernel_stats()
    finally:
        ctx.close()


def check_pairs(c, pb, pc):
    want = c.pairs()
    got = {b: [] for b in c.bases}
    for b, x in zip(pb, pc):
        got[b].append(x)
    for b in c.bases:                                            # every base, duplicates counted
        assert sorted(got[b]) == want[b], (c.name, c.universe.barcode[b], sorted(got[b]), want[b])
    # the documented order: pairs of one base adjacent, bases in the order they were given
    runs = [b for k, b in enumerate(pb) if k == 0 or pb[k - 1] != b]
    assert runs == [b for b in c.bases if want[b]]


def check_route(c, stats, no_table):
    launches = lambda name: stats[name]["launches"] if name in stats else None
    if len(c.parts) > wc.MAX_PARTS:                              # the host search: no search kernel at all
        assert launches("wl_table_search") is None and launches("wl_neighbours") is None
        assert launches("count:wl_bases_full_search") is None
    elif no_table or not c.has_tables:
        assert launches("wl_table_search") is None and launches("wl_table_build") is None
        assert launches("count:wl_bases_full_search") is None and launches("wl_neighbours") >= 1
    else:
        n = c.n_full_search()
        rounds = launches("wl_table_search")
        assert rounds >= 1 and launches("count:wl_bases_full_search") == n * rounds, (c.name, n, stats.get("count:wl_bases_full_search"))
        assert launches("wl_neighbours") == (rounds if n else None)
    return launches


@pytest.mark.parametrize("no_table", [False, True], ids=["tables", "no_table"])
@pytest.mark.parametrize("name", wc.CASE_NAMES)
def test_search_equals_the_model(name, no_table, tmp_path, monkeypatch):
    c = wc.case(name)
    if c.error is not None:
        with pytest.raises(capi.DropestError) as e:
            run_search(c, tmp_path, monkeypatch, no_table)
        assert c.error in str(e.value), str(e.value)
        return
    pb, pc, stats = run_search(c, tmp_path, monkeypatch, no_table)
    check_pairs(c, pb, pc)
    launches = check_route(c, stats, no_table)
    if name == "dense_1200_candidates":                          # the flat lists were too small at first: the search ran twice
        assert launches("wl_neighbours") == 2
    elif len(c.parts) <= wc.MAX_PARTS:
        assert launches("wl_neighbours") in (None, 1)
