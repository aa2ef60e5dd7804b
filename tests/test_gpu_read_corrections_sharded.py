"""`dropest -F`, the decisions, over the shards of a sharded or split run (csrc/shard_read_corrections.h: dropest_shard_read_corrections and the
group entries) against ONE context on the same reads and, through test_gpu_read_corrections._check, against tests/filtered_model.py fed the
ORACLE's merge targets, filtered cells and final molecules.

All shards share device 0; the reads are dealt in contiguous even ranges.  A shard's `column` entries are columns of the filtered matrix: they
are compared as barcodes (col_barcode[column] against the barcode of the one context's target cell).  Every case asserts on the expected side
(the oracle, the stream and dropest_owner_of alone: guards(), which needs no GPU) that it is about something: reads resident on a shard that does
not own their barcode, merged cells whose target another shard owns, and what _check asks of one context."""
import collections
import ctypes as C
import os

import numpy as np
import pytest

import filtered_model as fm
from dropest_amd import capi
from dropest_amd.multi import ShardGroup
from oracle import Oracle
from test_gpu_read_corrections import BASE_G, BASE_O, N_READS, Stream, _check, _final_molecules, _run

pytestmark = pytest.mark.gpu

WORLDS = (2, 3)
NONE = 0xFFFFFFFF
WL_O, WL_G = dict(merge_kind=1, barcodes_kind=1), dict(merge_kind=capi.MERGE_REAL_BARCODES, barcodes_kind=capi.BARCODES_CONST)

# name -> stream arguments, oracle / device configuration on top of BASE_*, whether the UMI merge targets are kept, what _check asks for
CASES = {
    "no_merge": dict(stream=dict(seed=1), o={}, g={}, save=True, about=(fm.NO_GENE, fm.CELL_NOT_KEPT), identity=True),
    "whitelist": dict(stream=dict(seed=2, children=3), o=WL_O, g=WL_G, whitelist=True, save=True, about=(fm.CELL_NOT_KEPT,), identity=True, merge=True),
    "simple": dict(stream=dict(seed=3, children=3), o=dict(merge_kind=2, max_cb_merge_ed=2), g=dict(merge_kind=capi.MERGE_SIMPLE, max_cb_merge_edit_distance=2),
                   save=True, about=(fm.CELL_NOT_KEPT,), identity=True, merge=True),
    "max_cells": dict(stream=dict(seed=4), o=dict(max_cells=10), g=dict(max_cells=10), save=True, about=(fm.CELL_NOT_KEPT,), identity=True),
    # the whitelist lacks one large cell's barcode, three substitutions from every other: the strategy excludes the cell
    "excluded": dict(stream=dict(seed=5), o=WL_O, g=WL_G, whitelist=True, drop_from_whitelist=0, save=True, about=(fm.CELL_NOT_KEPT,), identity=True),
    "escaped": dict(stream=dict(seed=6, n_barcode=True), o={}, g={}, save=True, about=(fm.NO_GENE,), identity=True),
    "n_umis": dict(stream=dict(seed=7, n_umis=150), o={}, g={}, save=True, about=(fm.NO_GENE,), identity=True, min_sources=20),
    "n_umis_not_kept": dict(stream=dict(seed=7, n_umis=150), o={}, g={}, save=False, about=(fm.WRONG_UMI,), identity=False, min_sources=20),
    "directional": dict(stream=dict(seed=8, umi_errors=0.08, n_umis=20), o=dict(umi_merge_kind=1), g=dict(umi_merge_kind=capi.UMI_MERGE_DIRECTIONAL),
                        save=True, about=(fm.NO_GENE,), identity=True, min_sources=200),
    "directional_whitelist": dict(stream=dict(seed=19, children=3, umi_errors=0.08), o=dict(WL_O, umi_merge_kind=1),
                                  g=dict(WL_G, umi_merge_kind=capi.UMI_MERGE_DIRECTIONAL), whitelist=True, save=True, about=(fm.CELL_NOT_KEPT,),
                                  identity=True, min_sources=200, merge=True),
    # -C 2 on a seed where one shard of two owns both kept cells: the other owns no filtered cell
    "one_shard_owns_nothing": dict(stream=dict(seed=14), o=dict(max_cells=2), g=dict(max_cells=2), save=True, about=(fm.CELL_NOT_KEPT,), identity=True,
                                   quarter=False),
}
SPLIT_CASES = ("no_merge", "whitelist", "n_umis")


def even_bounds(n, world):
    return [n * i // world for i in range(world + 1)]


def owner(code, world):
    return int(capi.lib().dropest_owner_of(int(code), world))


def build_case(name, tmp):
    """(stream, oracle arguments, device arguments) of a case"""
    case = CASES[name]
    s = Stream(**case["stream"])
    okw, gkw = dict(BASE_O, **case["o"]), dict(BASE_G, **case["g"])
    if case.get("whitelist"):
        if "drop_from_whitelist" in case:
            s.dropped = s.whitelist.pop(case["drop_from_whitelist"])
        d = os.path.join(str(tmp), name)
        os.makedirs(d, exist_ok=True)
        okw["barcodes_file"] = gkw["barcodes_file"] = s.write_whitelist(d)
    return s, okw, gkw


def barcode_of_cells(s):
    out = np.zeros(int(s.cell.max()) + 1, np.uint64)
    out[s.cell[::-1]] = s.cb[::-1]
    return out


def guards(name, s, o, worlds=WORLDS):
    """On the expected side, without a GPU: what the shards of this case have to get right."""
    case = CASES[name]
    n = len(s.cb)
    bc = barcode_of_cells(s)
    mt = [int(t) for t in o.merge_targets()]
    kept = set(int(x) for x in o.filtered_cells())
    mols = _final_molecules(o)
    cbs = fm.merge_cbs(mt, kept)
    # (verdict 4 here = written when the targets are kept: both UMI strategies hand out final targets)
    reach = np.array([g != capi.NO_GENE and int(c) in cbs and (cbs[int(c)], int(g)) in mols for c, g in zip(s.cell, s.gene)])
    for world in worlds:
        own = np.array([owner(b, world) for b in bc])
        bounds = even_bounds(n, world)
        resident = np.searchsorted(np.array(bounds[1:]), np.arange(n), side="right")
        assert (resident != own[s.cell]).sum() >= min(100, n // 4), (name, world)
        if case.get("merge"):
            cross = [b for b, t in enumerate(mt) if t != b and t in kept and own[b] != own[t]]
            assert cross, (name, world)
            assert (np.isin(s.cell, cross) & reach).sum() >= 100, (name, world)
    if name == "excluded":
        victim = int(s.cell[np.nonzero(s.cb == capi.pack_seq(s.dropped))[0][0]])
        assert o.cell_rows()[victim, 1] and mt[victim] == victim and victim not in kept
        assert ((s.cell == victim) & (s.gene != capi.NO_GENE)).sum() >= 100
    if name == "one_shard_owns_nothing":
        assert len(kept) == 2 and len(set(own_of for own_of in (owner(bc[c], 2) for c in kept))) == 1
        assert reach.sum() >= 100


def make_group(s, gkw, world, save, split_from=None):
    if split_from is not None:
        g = ShardGroup.split(split_from, world)
    else:
        g = ShardGroup([0] * world, **gkw)
        bounds = even_bounds(len(s.cb), world)
        for i, sh in enumerate(g.shards):
            sh.set_side_strings(s.side)
            sh.ctx.set_save_umi_merge_targets(save)
            sh.set_reads(capi.DeviceArrays.from_host(0, *[a[bounds[i]:bounds[i + 1]] for a in (s.cb, s.umi, s.gene, s.aux)]), bounds[i])
    g.step()
    return g


def take(g):
    """what a group answers, as host copies"""
    verdict, column, umi = g.read_corrections()
    col_barcode = np.array(g.shards[0].matrix(True)[3], np.uint64).copy()
    world = len(g.shards)
    return dict(verdict=verdict, column=column, umi=umi, counts=g.read_correction_counts().tolist(), col_barcode=col_barcode,
                owned=[sum(1 for b in col_barcode if owner(b, world) == p) for p in range(world)],      # columns of cm whose cell a shard owns
                ranges=[sh.read_corrections_device()[:2] for sh in g.shards])


@pytest.fixture(scope="module")
def ones(tmp_path_factory):
    """case -> the stream, the oracle, the one context and what it answers (checked against the model once)"""
    tmp = tmp_path_factory.mktemp("read_corrections_sharded")
    made = {}

    def get(name):
        if name not in made:
            case = CASES[name]
            s, okw, gkw = build_case(name, tmp)
            o, c = _run(s, okw, gkw, save=case["save"])
            guards(name, s, o)
            if case.get("quarter", True):
                verdict, cell, umi = _check(s, o, c, about=case["about"], identity=case["identity"], min_sources=case.get("min_sources", 0), save=case["save"])
            else:   # (too few reads written for _check's guards: the model directly)
                genes = [None if g == capi.NO_GENE else int(g) for g in s.gene]
                want = fm.decide_reads([int(x) for x in s.cell], genes, s.umi_text, o.merge_targets(), o.filtered_cells(), _final_molecules(o), {})
                verdict, cell, umi = c.read_corrections()
                assert verdict.tolist() == want[0] and cell.tolist() == [NONE if x is None else x for x in want[1]]
                assert [capi.unpack_code(x, s.side) for x in umi] == want[2]
            made[name] = dict(s=s, o=o, c=c, gkw=gkw, verdict=verdict, cell=cell, umi=umi, counts=c.read_correction_counts().tolist(), bc=barcode_of_cells(s))
        return made[name]

    return get


@pytest.fixture(scope="module")
def runs(ones):
    made = {}

    def get(name, world):
        if (name, world) not in made:
            one = ones(name)
            g = make_group(one["s"], one["gkw"], world, CASES[name]["save"])
            try:
                made[(name, world)] = take(g)
            finally:
                g.close()
        return made[(name, world)]

    return get


def same_as_one_context(got, one):
    assert np.array_equal(got["verdict"], one["verdict"])
    none = one["cell"] == NONE
    assert np.array_equal(got["column"] == NONE, none)
    assert np.array_equal(got["col_barcode"][got["column"][~none]], one["bc"][one["cell"][~none]])
    assert np.array_equal(got["umi"], one["umi"])                                   # bit-equal codes
    assert got["counts"] == one["counts"]


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_group_equals_one_context(ones, runs, name, world):
    one, got = ones(name), runs(name, world)
    s, o = one["s"], one["o"]
    assert got["col_barcode"].tolist() == [int(one["bc"][int(i)]) for i in o.filtered_cells()]
    same_as_one_context(got, one)
    assert sum(got["owned"]) == len(o.filtered_cells())
    if name == "one_shard_owns_nothing" and world == 2:
        assert sorted(got["owned"]) == [0, 2]
    # every shard answered for its own contiguous range
    bounds = even_bounds(len(s.cb), world)
    assert got["ranges"] == [(bounds[i + 1] - bounds[i], bounds[i]) for i in range(world)]
    if CASES[name]["identity"]:   # the reads written under (target barcode, gene, corrected UMI) are the oracle's final molecules' reads
        w = got["verdict"] == fm.WRITTEN
        written = collections.Counter(zip(got["col_barcode"][got["column"][w]].tolist(), s.gene[w].tolist(), got["umi"][w].tolist()))
        kept = set(int(x) for x in o.filtered_cells())
        code = {u: int(x) for u, x in zip(s.umi_text, s.umi)}
        expect = {}
        for (cell, gene), m in _final_molecules(o).items():
            if cell in kept:
                for u, r in m.items():
                    expect[(int(one["bc"][cell]), gene, code.get(u, capi.pack_seq(u)))] = r
        assert written == expect


@pytest.mark.parametrize("n_reads,world", [(65, 3), (1, 2)])
def test_short_streams(n_reads, world):
    """65 reads over 3 shards; 1 read over 2: one shard has no resident read and still joins every collective"""
    s = Stream(11, n_reads=n_reads)
    kw_o, kw_g = dict(BASE_O, min_genes_before=0, min_genes_after=0), dict(BASE_G, min_genes_before_merge=0, min_genes_after_merge=0)
    o, c = _run(s, kw_o, kw_g, save=True)
    mols = _final_molecules(o)
    genes = [None if g == capi.NO_GENE else int(g) for g in s.gene]
    want_v, want_c, want_u = fm.decide_reads([int(x) for x in s.cell], genes, s.umi_text, o.merge_targets(), o.filtered_cells(), mols, {})
    assert fm.WRITTEN in want_v
    g = make_group(s, kw_g, world, True)
    try:
        got = take(g)
    finally:
        g.close()
    bc = barcode_of_cells(s)
    assert got["verdict"].tolist() == want_v
    assert [None if x == NONE else int(got["col_barcode"][x]) for x in got["column"]] == [None if x is None else int(bc[x]) for x in want_c]
    assert [capi.unpack_code(x, s.side) for x in got["umi"]] == want_u
    assert got["counts"] == [want_v.count(v) for v in range(5)]
    assert 0 in [r[0] for r in got["ranges"]] or n_reads > 1


def test_a_middle_range_that_straddles_a_shard_boundary(ones):
    one = ones("whitelist")
    g = make_group(one["s"], one["gkw"], 3, True)
    try:
        cut = even_bounds(N_READS, 3)[1]
        first, count = cut - 40, 101
        v, col, u = g.read_corrections(first=first, count=count)
        whole = take(g)
        assert np.array_equal(v, whole["verdict"][first:first + count]) and np.array_equal(col, whole["column"][first:first + count])
        assert np.array_equal(u, whole["umi"][first:first + count]) and np.array_equal(v, one["verdict"][first:first + count])
        assert len(g.read_corrections(first=N_READS, count=0)[0]) == 0
        with pytest.raises(capi.DropestError):
            g.read_corrections(first=N_READS - 5, count=6)
    finally:
        g.close()


@pytest.mark.parametrize("parts", WORLDS)
@pytest.mark.parametrize("name", SPLIT_CASES)
def test_split_context_equals_the_context_before_the_split(ones, name, parts):
    one = ones(name)
    s, gkw = one["s"], one["gkw"]
    c = capi.Context(**gkw)
    c.set_side_strings(s.side)
    c.set_save_umi_merge_targets(CASES[name]["save"])
    c.push_reads(s.cb, s.umi, s.gene, s.aux)
    c.set_initialized()
    g = make_group(s, gkw, parts, None, split_from=c)
    try:
        same_as_one_context(take(g), one)
        with pytest.raises(capi.DropestError) as e:                                  # the parent still refuses, and says where to ask
            c.read_corrections()
        assert "shard" in str(e.value) and "dropest_shard_group_read_corrections" in str(e.value)
        with pytest.raises(capi.DropestError) as e:
            g.shards[0].ctx.read_corrections()
        assert "shard" in str(e.value) and "dropest_shard_read_corrections" in str(e.value)
    finally:
        g.close()


# ---- the column table alone ---------------------------------------------------------------------------------------------------------------
def mix64(x):
    m = (1 << 64) - 1
    x ^= x >> 30; x = (x * 0xbf58476d1ce4e5b9) & m
    x ^= x >> 27; x = (x * 0x94d049bb133111eb) & m
    return x ^ (x >> 31)


def column_table(barcodes, columns, probes):
    L = capi.lib()
    L.dropest_test_column_table.restype = C.c_int
    L.dropest_test_column_table.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    b, c, p = np.array(barcodes, np.uint64), np.array(columns, np.uint32), np.array(probes, np.uint64)
    out = np.zeros(len(p), np.uint32)
    cap, flags = C.c_uint32(), C.c_uint32()
    assert L.dropest_test_column_table(0, b.ctypes.data, c.ctypes.data, len(b), p.ctypes.data, len(p), out.ctypes.data, C.byref(cap), C.byref(flags)) == 0
    return out, cap.value, flags.value


@pytest.mark.parametrize("n,capacity", [(0, 2), (1, 2), (64, 128), (65, 256), (3000, 8192)])
def test_column_table_capacity_and_probes(n, capacity):
    """capacity: the power of two of at least twice the entries -- 64 entries sit exactly at 128 slots, 65 take 256.  Every barcode is found
    with its column, among them barcodes that share a home slot with another or have it as their neighbour; absent barcodes are not."""
    rng = np.random.RandomState(n)
    codes = {int(capi.pack_seq("".join("ACGT"[k] for k in rng.randint(0, 4, 12)))) for _ in range(n * 2)}
    codes = sorted(codes)[:n]
    if n >= 64:   # a chain: barcodes whose home slot is that of codes[0], or the one behind it, so that they end up displaced
        mask, home, extra, k = capacity - 1, mix64(codes[0]) & (capacity - 1), [], 1 << 40
        while len(extra) < 4:
            k += 1
            if (mix64(k) & mask) in (home, (home + 1) & mask) and k not in codes:
                extra.append(k)
        codes = codes[:n - 4] + extra
    if n == 3000:
        codes[7] = capi.ESCAPE | 5                                                    # an escaped barcode is a key like any other
    columns = list(range(100, 100 + len(codes)))
    absent = [int(capi.pack_seq("ACGTACGTACGTA")), capi.ESCAPE | 77, (1 << 40) - 3]
    got, cap, flags = column_table(codes, columns, codes + absent)
    assert flags == 0 and cap == capacity
    assert got[:len(codes)].tolist() == columns and got[len(codes):].tolist() == [NONE] * len(absent)


def test_column_table_flags_a_barcode_with_two_columns():
    codes = [int(capi.pack_seq(x)) for x in ("ACGTAC", "TTTTGG", "ACGTAC")]
    assert column_table(codes, [1, 2, 1], codes)[2] == 0                            # the same pair twice is the same statement
    got, _, flags = column_table(codes, [1, 2, 3], codes[:2])
    assert flags == 1 and got[1] == 2 and got[0] in (1, 3)                           # flagged; one of the two stays, nothing else is touched


# ---- refusals and staleness ---------------------------------------------------------------------------------------------------------------
def test_before_a_step_is_refused_and_the_group_stays_usable(ones):
    one = ones("no_merge")
    s = one["s"]
    g = ShardGroup([0, 0], **one["gkw"])
    try:
        bounds = even_bounds(len(s.cb), 2)
        for i, sh in enumerate(g.shards):
            sh.set_side_strings(s.side)
            sh.ctx.set_save_umi_merge_targets(True)
            sh.set_reads(capi.DeviceArrays.from_host(0, *[a[bounds[i]:bounds[i + 1]] for a in (s.cb, s.umi, s.gene, s.aux)]), bounds[i])
        with pytest.raises(capi.DropestError) as e:
            g.read_corrections()
        assert e.value.status == 1 and "You must initialize container" in str(e.value)
        with pytest.raises(capi.DropestError):
            g.read_correction_counts()
        g.step()
        same_as_one_context(take(g), one)
    finally:
        g.close()


def test_umi_dictionary_mode_is_refused_and_the_group_stays_usable(ones, monkeypatch):
    one = ones("no_merge")
    monkeypatch.setenv("DROPEST_UMI_DICT", "2")
    g = make_group(one["s"], one["gkw"], 2, True)
    try:
        with pytest.raises(capi.DropestError) as e:
            g.read_corrections()
        assert e.value.status == 4 and "UMI-dictionary" in str(e.value)
        assert g.shards[0].matrix(True)[3].tolist() == [int(one["bc"][int(i)]) for i in one["o"].filtered_cells()]   # a matrix call still works
        monkeypatch.delenv("DROPEST_UMI_DICT")
        g.step()                                                                      # ... and so does the next step, and the question after it
        same_as_one_context(take(g), one)
    finally:
        g.close()


def test_corrections_are_cached_until_the_next_step(ones):
    one = ones("n_umis")
    g = make_group(one["s"], one["gkw"], 2, True)
    try:
        first = take(g)
        pointers = [sh.read_corrections_device() for sh in g.shards]
        again = take(g)
        assert all(np.array_equal(first[k], again[k]) for k in ("verdict", "column", "umi"))
        assert [sh.read_corrections_device() for sh in g.shards] == pointers          # the same arrays, by one shard alone: no collective to join
        for sh in g.shards:
            ph = sh.phase_stats()
            assert ph["read_corrections:view"]["steps"] == 1 and ph["read_corrections:table"]["steps"] == 1
        n, d_codes = g.shards[1].filtered_barcodes_device()
        assert n == len(first["col_barcode"]) and d_codes
        codes = np.zeros(n, np.uint64)
        assert capi.lib().dropest_dev_copy_to_host(0, codes.ctypes.data, C.c_void_p(d_codes), codes.nbytes) == 0
        assert np.array_equal(codes, first["col_barcode"])
        # another step without the targets: the arrays are rebuilt, the reads of merged-away UMIs are dropped now
        for sh in g.shards:
            sh.ctx.set_save_umi_merge_targets(False)
        g.step()
        rebuilt = take(g)
        assert g.shards[0].phase_stats()["read_corrections:view"]["steps"] == 2
        assert (rebuilt["verdict"] == fm.WRONG_UMI).sum() >= 20 and not (first["verdict"] == fm.WRONG_UMI).any()
        same = rebuilt["verdict"] != fm.WRONG_UMI
        assert np.array_equal(rebuilt["verdict"][same], first["verdict"][same])
    finally:
        g.close()
