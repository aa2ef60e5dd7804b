"""Pins tests/whitelist_model.py -- the plain-Python restatement of the reference's whitelist neighbour search that
test_gpu_whitelist_search.py compares the device with -- on the CPU oracle: the edit distance, and the candidate
multiset of every cell before any merge is applied, on random whitelist streams, on the reference's own fixture and
on the inputs of every GPU case (whitelist_cases.py).  No GPU."""
import random
import re

import numpy as np
import pytest

from dropest_amd import capi
from oracle import Oracle
from oracle import binding as ob

import test_gpu_stress
import whitelist_cases as wc
import whitelist_model as wm
from test_oracle_reference_kat import TEST_EST, fixture_container


def test_edit_distance_known_answers():
    """Tests/TestTools.cpp:47-54 (the defaults: N matches), as test_oracle_reference_kat.py::test_edit_distance"""
    assert wm.edit_distance("ATTTTC", "ATTTGC") == 1
    assert wm.edit_distance("ATTTTCC", "ATTTGNC") == 1
    assert wm.edit_distance("ATTTTCC", "ATTTGTC") == 2
    assert wm.edit_distance("ATTTTCC", "ATTTTCC") == 0


@pytest.mark.parametrize("n_side", ["none", "first", "second", "both"])
def test_edit_distance_equals_the_oracle(n_side):
    rng = random.Random({"none": 1, "first": 2, "second": 3, "both": 4}[n_side])
    lengths = list(range(32))
    for k in range(1500):
        la, lb = (rng.choice(lengths), rng.choice(lengths)) if k % 3 else (k % 32, (k // 3) % 32)
        a = wc.rnd_seq(rng, la)
        b = wc.substitute(rng, a, min(la, rng.randint(0, 3))) if k % 2 and la else wc.rnd_seq(rng, lb)   # relatives and strangers
        if k % 4 == 1 and b:
            i = rng.randrange(len(b))
            b = b[:i] + b[i + 1:] if k % 8 == 1 else b[:i] + rng.choice("ACGT") + b[i:]
        b = b[:31]
        if n_side in ("first", "both") and a:
            a = wc.with_n(a, rng.sample(range(len(a)), min(len(a), rng.randint(1, 3))))
        if n_side in ("second", "both") and b:
            b = wc.with_n(b, rng.sample(range(len(b)), min(len(b), rng.randint(1, 3))))
        assert wm.edit_distance(a, b) == ob.edit_distance(a, b), (a, b)


def test_whitelist_file_round_trip(tmp_path):
    for name in ("indrop", "parts_3", "repeated_entry"):
        c = wc.case(name)
        path = tmp_path / name
        path.write_text(wm.whitelist_text(c.parts))
        assert wm.parse_whitelist(path.read_text(), c.kind) == c.parts
        o = Oracle()
        o.wl_load(c.kind, str(path))
        assert [o.wl_part(p) for p in range(o.wl_parts())] == c.parts
    assert wm.parse_whitelist(open(TEST_EST).read(), wm.INDROP) == [["AAT", "GAA", "AAA"], ["TTAGGTCCA", "TTAGGGGCC", "TTAGGTCCC"]]


def universe_of(o):
    rows = o.cell_rows()
    return wm.Universe([o.cell_barcode(i) for i in range(o.n_cells)], [int(x) for x in rows[:, 3]], [int(x) for x in rows[:, 7]])


def assert_model_equals_oracle(o, kind, parts, poisson, min_genes, cells=None):
    u = universe_of(o)
    for cell in (range(len(u)) if cells is None else cells):
        s = wm.search(kind, parts, poisson, min_genes, u, cell)
        assert sorted(s.candidates) == sorted(int(x) for x in o.real_neighbours(cell)), u.barcode[cell]


def test_candidates_on_the_reference_fixture():
    """the container of Tests/TestEstimation.cpp (testRealNeighboursCbs)"""
    o = fixture_container()
    parts = [o.wl_part(0), o.wl_part(1)]
    assert_model_equals_oracle(o, wm.INDROP, parts, False, 0)
    u = universe_of(o)
    s = wm.search(wm.INDROP, parts, False, 0, u, u.by_barcode["CAATTAGGTCCG"])
    assert [u.barcode[c] for c in s.candidates] == ["AAATTAGGTCCA", "AAATTAGGTCCC"]
    s = wm.search(wm.INDROP, parts, False, 0, u, u.by_barcode["AAATTAGGTCCC"])
    assert [u.barcode[c] for c in s.candidates] == ["AAATTAGGTCCC"]


@pytest.mark.parametrize("poisson", [False, True])
@pytest.mark.parametrize("seed", range(10))
def test_candidates_on_random_whitelist_streams(seed, poisson, tmp_path):
    """the streams of test_gpu_stress.py::test_random_whitelist_merges: both kinds, 1-4 parts, barcodes that are exact, mutated,
    longer, shorter or carry an N"""
    cb, umi, gene, aux, side, okw, gkw = test_gpu_stress.random_whitelist_case(seed, poisson, tmp_path)
    o = Oracle(**okw)
    o.add_packed(cb, umi, gene, aux, side)
    o.set_initialized()
    parts = wm.parse_whitelist(open(okw["barcodes_file"]).read(), okw["barcodes_kind"])
    assert parts == [o.wl_part(p) for p in range(o.wl_parts())]
    assert_model_equals_oracle(o, okw["barcodes_kind"], parts, poisson, okw["min_genes_before"])


def oracle_of_case(c, path):
    """an oracle container whose cells are the case's universe, in its order: n_genes genes of one UMI each, the rest of
    TOTAL_UMIS on the first gene"""
    path.write_text(wm.whitelist_text(c.parts))
    side, cb, umi, gene = [], [], [], []
    u = c.universe
    for i in range(len(u)):
        code = capi.pack_seq(u.barcode[i])
        if code is None:
            side.append(u.barcode[i])
            code = capi.ESCAPE | (len(side) - 1)
        for k in range(u.total_umis[i]):
            cb.append(code)
            umi.append(capi.pack_seq("".join("ACGT"[(k >> (2 * j)) & 3] for j in range(6))))
            gene.append(k if k < u.n_genes[i] else 0)
    o = Oracle(merge_kind=3 if c.poisson else 1, barcodes_kind=c.kind, barcodes_file=str(path), min_genes_before=c.min_genes,
               min_genes_after=0)
    o.add_packed(np.array(cb, np.uint64), np.array(umi, np.uint64), np.array(gene, np.uint32), np.full(len(cb), 2 << 16, np.uint32), side)
    o.set_initialized()
    got = universe_of(o)
    assert (got.barcode, got.n_genes, got.total_umis) == (u.barcode, u.n_genes, u.total_umis)
    return o


@pytest.mark.parametrize("name", wc.CASE_NAMES)
def test_gpu_cases_through_model_and_oracle(name, tmp_path):
    c = wc.case(name)
    o = oracle_of_case(c, tmp_path / "wl")
    if c.error and c.error.startswith("Barcode"):
        good, bad = c.bases
        with pytest.raises(wm.BarcodeLengthError) as e:
            wm.split_barcode(c.kind, c.parts, c.universe.barcode[bad])
        assert str(e.value) == c.error
        # the oracle throws the reference's text for the const kind; for inDrop both throw what std::string::substr throws
        with pytest.raises(RuntimeError, match=re.escape(c.error) if c.kind == wm.CONST else "substr"):
            o.wl_split(c.universe.barcode[bad])
        s = wm.search(c.kind, c.parts, c.poisson, c.min_genes, c.universe, good)      # the base beside it is searched as usual
        assert s.candidates and sorted(s.candidates) == sorted(int(x) for x in o.real_neighbours(good))
        assert wm.split_barcode(c.kind, c.parts, c.universe.barcode[good]) == o.wl_split(c.universe.barcode[good])
        return
    for b, s in zip(c.bases, c.searches()):
        assert sorted(s.candidates) == sorted(int(x) for x in o.real_neighbours(b)), c.universe.barcode[b]
        assert wm.split_barcode(c.kind, c.parts, c.universe.barcode[b]) == o.wl_split(c.universe.barcode[b])
