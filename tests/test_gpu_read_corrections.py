"""dropest_read_corrections / dropest_umi_merge_targets (`dropest -F`, FilteringBamProcessor.cpp:14-40, :61-96) against
tests/filtered_model.py fed the ORACLE's merge targets, filtered cells and final molecules.

Streams of 20 011 reads (no multiple of 64 or 256): 20 large barcodes with all 30 genes, 20 small ones with 5 genes (real, never
filtered), UMIs of 6 bases.  Every case asserts on the expected side that it is about something: a quarter of the reads written, 100
reads in each verdict it names, 20 sources where a UMI merge runs.
"""
import collections
import os

import numpy as np
import pytest

import filtered_model as fm
import parity
from dropest_amd import capi
from dropest_amd.synth import reverse_complement
from oracle import Oracle

pytestmark = pytest.mark.gpu

N_READS = 20011
N_GENES = 30
UMI_LEN = 6
MAX_UMI_ED = 1


def _seq(rng, n):
    return "".join("ACGT"[k] for k in rng.randint(0, 4, n))


def _far_apart(rng, count, n, dist):
    out = []
    while len(out) < count:
        s = _seq(rng, n)
        if all(sum(a != b for a, b in zip(s, t)) >= dist for t in out):
            out.append(s)
    return out


class Stream:
    """cells: 20 large (weight 4, every gene), 20 small (weight 1, 5 genes), `children` of each kind: a barcode one substitution
    away that draws from its parent's molecules.  10 % of the reads have no gene.  umi_errors: share of the large cells' reads whose UMI
    gets one substitution (what -u folds back).  n_umis: that many reads of molecules with another clean read get one base replaced by N,
    at a position where no other UMI of the group fits, so that the original UMI is the one best target."""

    def __init__(self, seed, n_reads=N_READS, children=0, umi_errors=0.0, n_umis=0, n_barcode=False, umis_per_gene=6):
        rng = np.random.RandomState(seed)
        base = _far_apart(rng, 40, 8, 3)
        if n_barcode:
            base[0] = base[0][:4] + "N" + base[0][5:]
        self.whitelist = [b for b in base if "N" not in b]
        mols, weight, barcode = [], [], []
        for i, b in enumerate(base):
            genes = range(N_GENES) if i < 20 else rng.choice(N_GENES, 5, replace=False)
            mols.append([(int(g), u) for g in genes for u in _far_apart(rng, umis_per_gene, UMI_LEN, 2)])
            weight.append(4.0 if i < 20 else 1.0); barcode.append(b)
        for parent in list(range(children)) + list(range(20, 20 + children)):
            b = barcode[parent]
            while True:
                p = rng.randint(8); c = b[:p] + "ACGT"[rng.randint(4)] + b[p + 1:]
                if c not in barcode:
                    break
            mols.append(mols[parent]); weight.append(1.0); barcode.append(c)
        w = np.array(weight) / sum(weight)
        cell = rng.choice(len(w), n_reads, p=w)
        reads = []
        for c in cell:
            g, u = mols[c][rng.randint(len(mols[c]))]
            if c < 20 and rng.rand() < umi_errors:
                p = rng.randint(UMI_LEN); u = u[:p] + "ACGT"[rng.randint(4)] + u[p + 1:]
            reads.append([barcode[c], u, g if rng.rand() >= 0.1 else None])
        if n_umis:
            groups = collections.defaultdict(collections.Counter)
            for b, u, g in reads:
                if g is not None:
                    groups[(b, g)][u] += 1
            seen, done = collections.Counter(), 0
            for r in reads:
                b, u, g = r
                if g is None or done == n_umis:
                    continue
                seen[(b, g, u)] += 1
                if groups[(b, g)][u] < 3 or seen[(b, g, u)] != 2 or rng.rand() < 0.5:
                    continue
                for p in range(UMI_LEN):
                    bad = u[:p] + "N" + u[p + 1:]
                    if all(fm.hamming_n(bad, o) > 0 for o in groups[(b, g)] if o != u and "N" not in o):
                        r[1] = bad; done += 1
                        break
            assert done == n_umis
        # packed columns; side strings in the order of first appearance (UMIs: on gene-bearing reads only)
        side, index = [], {}

        def code(s):
            c = capi.pack_seq(s)
            if c is None:
                if s not in index:
                    index[s] = len(side); side.append(s)
                c = capi.ESCAPE | index[s]
            return c
        cb = np.zeros(n_reads, np.uint64); umi = np.zeros(n_reads, np.uint64)
        for i, (b, u, g) in enumerate(reads):
            cb[i] = code(b); umi[i] = code(u if g is not None or "N" not in u else u.replace("N", "A"))
        gene = np.array([capi.NO_GENE if g is None else g for _, _, g in reads], np.uint32)
        aux = np.full(n_reads, 2 << 16, np.uint32)
        self.cb, self.umi, self.gene, self.aux = parity.canonical_stream(cb, umi, gene, aux)
        self.side = side
        self.cell = parity.first_seen_ids(self.cb)                       # cell id of every read
        self.umi_text = [capi.unpack_code(x, side) for x in self.umi]

    def write_whitelist(self, tmp_path):
        path = os.path.join(str(tmp_path), "whitelist")
        with open(path, "w") as f:
            f.write(" ".join(reverse_complement(b) for b in self.whitelist) + "\n")
        return path


def _run(s, okw, gkw, save, pre=None, merge=True):
    o = Oracle(**okw); o.add_packed(s.cb, s.umi, s.gene, s.aux, s.side); o.set_initialized()
    c = capi.Context(**gkw)
    c.set_side_strings(s.side)
    c.set_save_umi_merge_targets(save)
    c.push_reads(s.cb, s.umi, s.gene, s.aux)
    c.set_initialized()
    if pre:
        pre(o, c)
    if merge:
        o.merge_and_filter(); c.merge_and_filter()
    return o, c


def _final_molecules(o):
    """{(cell, gene): {umi: reads}} of the oracle's cells that were not merged away"""
    merged = o.cell_rows()[:, 0]
    out = {}
    for c, g, u, r, _ in zip(*o.molecules()):
        if not merged[int(c)]:
            out.setdefault((int(c), int(g)), {})[u] = int(r)
    return out


def _targets(c, side):
    raw = [(int(a), int(b), int(x)) for a, b, x, _ in zip(*c.umi_merge_targets())]
    assert raw == sorted(set(raw))                                         # ascending (cell, gene, source code), one row per source
    rows = sorted((int(a), int(b), capi.unpack_code(x, side), capi.unpack_code(y, side)) for a, b, x, y in zip(*c.umi_merge_targets()))
    table = {}
    for cell, gene, src, tgt in rows:
        table.setdefault((cell, gene), {})[src] = tgt
    return rows, table


def expected_verdicts(s, o, save):
    """From the oracle alone: the verdict of every read, and the (cell, gene, UMI) of the reads that can only be written through
    Gene::merge_targets() -- their UMI is no molecule of the final state.  With the targets kept every such read is written (both UMI
    strategies hand out final targets); without them it is a wrong UMI."""
    mols = _final_molecules(o)
    cbs = fm.merge_cbs(o.merge_targets(), o.filtered_cells())
    verdicts, sources = [], set()
    for cell, g, u in zip(s.cell, s.gene, s.umi_text):
        v, t, _ = fm.decide_read(int(cell), None if g == capi.NO_GENE else int(g), u, cbs, mols, {})
        if v == fm.WRONG_UMI:
            sources.add((t, int(g), u))
            if save:
                v = fm.WRITTEN
        verdicts.append(v)
    return verdicts, sources


def check_guards(s, o, save, about, min_sources):
    verdicts, sources = expected_verdicts(s, o, save)
    by_verdict = collections.Counter(verdicts)
    assert by_verdict[fm.WRITTEN] * 4 >= len(verdicts), by_verdict
    for v in about:
        assert by_verdict[v] >= 100, (v, by_verdict)
    assert len(sources) >= min_sources, len(sources)
    return verdicts


def _check(s, o, c, about, identity, min_sources=0, save=True):
    """The guards; verdict, target cell and corrected UMI of every read; the counts; the written reads per molecule."""
    expected = check_guards(s, o, save, about, min_sources)
    mols = _final_molecules(o)
    rows, table = _targets(c, s.side)
    genes = [None if g == capi.NO_GENE else int(g) for g in s.gene]
    cells = [int(x) for x in s.cell]
    want_v, want_c, want_u = fm.decide_reads(cells, genes, s.umi_text, o.merge_targets(), o.filtered_cells(), mols, table)
    assert want_v == expected
    n = len(cells)
    by_verdict = collections.Counter(want_v)

    verdict, cell, umi = c.read_corrections()
    assert len(verdict) == n
    assert verdict.tolist() == want_v
    assert cell.tolist() == [0xFFFFFFFF if x is None else x for x in want_c]
    got_u = [capi.unpack_code(x, s.side) for x in umi]
    assert got_u == want_u
    assert c.read_correction_counts().tolist() == [by_verdict[v] for v in range(5)]
    # host copies of a range in the middle
    if n > 200:
        v2, c2, u2 = c.read_corrections(first=77, count=101)
        assert np.array_equal(v2, verdict[77:178]) and np.array_equal(c2, cell[77:178]) and np.array_equal(u2, umi[77:178])
    # a read whose UMI is no source keeps it
    for i in range(n):
        if want_v[i] == fm.WRITTEN and s.umi_text[i] not in table.get((want_c[i], genes[i]), {}):
            assert got_u[i] == s.umi_text[i]
    if identity:   # the reads written under a molecule are that molecule's reads
        written = collections.Counter((int(cell[i]), genes[i], got_u[i]) for i in range(n) if verdict[i] == fm.WRITTEN)
        kept = set(int(x) for x in o.filtered_cells())
        expect = {(cg[0], cg[1], u): r for cg, m in mols.items() if cg[0] in kept for u, r in m.items()}
        assert written == expect
    return verdict, cell, umi


BASE_O = dict(min_genes_before=3, min_genes_after=10, max_umi_merge_ed=MAX_UMI_ED)
BASE_G = dict(min_genes_before_merge=3, min_genes_after_merge=10, max_umi_merge_edit_distance=MAX_UMI_ED)


def test_no_barcode_merge():
    s = Stream(1)
    o, c = _run(s, BASE_O, BASE_G, save=True)
    assert len(o.filtered_cells()) == 20 and o.n_cells == 40          # half the cells are filtered
    _check(s, o, c, about=(fm.NO_GENE, fm.CELL_NOT_KEPT), identity=True)


def test_whitelist_merge_into_kept_and_not_kept_cells(tmp_path):
    s = Stream(2, children=3)
    path = s.write_whitelist(tmp_path)
    o, c = _run(s, dict(BASE_O, merge_kind=1, barcodes_kind=1, barcodes_file=path),
                dict(BASE_G, merge_kind=capi.MERGE_REAL_BARCODES, barcodes_kind=capi.BARCODES_CONST, barcodes_file=path), save=True)
    mt, kept = o.merge_targets(), set(int(x) for x in o.filtered_cells())
    moved = [(b, int(t)) for b, t in enumerate(mt) if int(t) != b]
    assert any(t in kept for _, t in moved) and any(t not in kept for _, t in moved)
    verdict, cell, _ = _check(s, o, c, about=(fm.CELL_NOT_KEPT,), identity=True)
    sources_kept = [b for b, t in moved if t in kept]
    reads = np.isin(s.cell, sources_kept) & (verdict == fm.WRITTEN)
    assert reads.sum() >= 100 and all(int(cell[i]) == int(mt[s.cell[i]]) for i in np.nonzero(reads)[0])


def test_simple_merge():
    s = Stream(3, children=3)
    o, c = _run(s, dict(BASE_O, merge_kind=2, max_cb_merge_ed=2), dict(BASE_G, merge_kind=capi.MERGE_SIMPLE, max_cb_merge_edit_distance=2), save=True)
    assert any(int(t) != b for b, t in enumerate(o.merge_targets()))
    _check(s, o, c, about=(fm.CELL_NOT_KEPT,), identity=True)


def test_max_cells_cuts_real_cells_out_of_the_filtered_list():
    s = Stream(4)
    o, c = _run(s, dict(BASE_O, max_cells=10), dict(BASE_G, max_cells=10), save=True)
    assert len(o.filtered_cells()) == 10 and o.n_real == 40
    _check(s, o, c, about=(fm.CELL_NOT_KEPT,), identity=True)


def test_excluded_cell():
    s = Stream(5)
    victim = int(s.cell[np.nonzero(s.gene != capi.NO_GENE)[0][0]])

    def pre(o, c):
        o.exclude_cell(victim); c.exclude_cell(victim)
    o, c = _run(s, BASE_O, BASE_G, save=True, pre=pre)
    assert victim not in set(int(x) for x in o.filtered_cells())
    verdict, _, _ = _check(s, o, c, about=(fm.CELL_NOT_KEPT,), identity=True)
    mine = (s.cell == victim) & (s.gene != capi.NO_GENE)
    assert mine.sum() >= 100 and set(verdict[mine].tolist()) == {fm.CELL_NOT_KEPT}


def test_kept_cell_with_an_escaped_barcode():
    s = Stream(6, n_barcode=True)
    o, c = _run(s, BASE_O, BASE_G, save=True)
    escaped = [i for i in range(o.n_cells) if "N" in o.cell_barcode(i)]
    assert len(escaped) == 1 and escaped[0] in set(int(x) for x in o.filtered_cells())
    verdict, cell, _ = _check(s, o, c, about=(fm.NO_GENE,), identity=True)
    assert ((cell == escaped[0]) & (verdict == fm.WRITTEN)).sum() >= 100


def test_n_umi_merge_with_the_targets_kept():
    s = Stream(7, n_umis=150)
    o, c = _run(s, BASE_O, BASE_G, save=True)
    _check(s, o, c, about=(fm.NO_GENE,), identity=True, min_sources=20)
    # Gene::merge_targets() against the model: the state before the UMI merge is the stream itself (no barcode merge)
    groups = {}
    for cell, g, u in zip(s.cell, s.gene, s.umi_text):
        if g != capi.NO_GENE:
            groups.setdefault((int(cell), int(g)), collections.Counter())[u] += 1
    real = o.cell_rows()[:, 2]
    log = [(cg[0], cg[1], bad, tgt) for cg, m in sorted(groups.items()) if real[cg[0]]
           for bad, tgt in fm.simple_umi_targets(m, MAX_UMI_ED).items()]
    rows, _ = _targets(c, s.side)
    assert rows == fm.record_merges(log) and len(rows) >= 100


def test_n_umi_merge_without_the_targets_drops_those_reads():
    s = Stream(7, n_umis=150)
    o, c = _run(s, BASE_O, BASE_G, save=False)
    assert c.umi_merge_targets()[0].size == 0
    verdict, _, _ = _check(s, o, c, about=(fm.WRONG_UMI,), identity=False, min_sources=20, save=False)
    bad = np.array(["N" in u for u in s.umi_text])
    kept = np.isin(s.cell, o.filtered_cells())
    assert set(verdict[bad & kept].tolist()) == {fm.WRONG_UMI} and not (verdict[~bad] == fm.WRONG_UMI).any()


def test_directional_merge_with_the_targets_kept():
    s = Stream(8, umi_errors=0.08, n_umis=20)
    o, c = _run(s, dict(BASE_O, umi_merge_kind=1), dict(BASE_G, umi_merge_kind=capi.UMI_MERGE_DIRECTIONAL), save=True)
    _check(s, o, c, about=(fm.NO_GENE,), identity=True, min_sources=200)


def test_directional_merge_behind_a_whitelist_merge(tmp_path):
    s = Stream(9, children=3, umi_errors=0.08)
    path = s.write_whitelist(tmp_path)
    o, c = _run(s, dict(BASE_O, merge_kind=1, barcodes_kind=1, barcodes_file=path, umi_merge_kind=1),
                dict(BASE_G, merge_kind=capi.MERGE_REAL_BARCODES, barcodes_kind=capi.BARCODES_CONST, barcodes_file=path,
                     umi_merge_kind=capi.UMI_MERGE_DIRECTIONAL), save=True)
    assert any(int(t) != b for b, t in enumerate(o.merge_targets()))
    _check(s, o, c, about=(fm.CELL_NOT_KEPT,), identity=True, min_sources=200)


def test_merge_umis_by_hand():
    s = Stream(10)
    cellf = int(s.cell[0])
    picked = {}

    def pre(o, c):
        g, u, r, m = c.cell_molecules(cellf)
        g0 = int(g[0]); mine = [int(x) for x, gg in zip(u, g) if int(gg) == g0]
        assert len(mine) >= 4
        new = capi.pack_seq("TTTTTT") if capi.pack_seq("TTTTTT") not in mine else capi.pack_seq("GGGGGG")
        # a source sent to one target, then to another: the last one stays; an identity pair; a source sent to a new UMI
        first = [(mine[0], mine[1]), (mine[2], new), (mine[3], mine[3])]
        c.merge_umis(cellf, g0, first)
        o.merge_umis_explicit(cellf, "G%d" % g0, {capi.unpack_code(x): capi.unpack_code(y) for x, y in first})
        second = [(mine[1], mine[0])]                                      # the molecule under mine[1] moves on, to a UMI that is back
        c.merge_umis(cellf, g0, second)
        o.merge_umis_explicit(cellf, "G%d" % g0, {capi.unpack_code(x): capi.unpack_code(y) for x, y in second})
        picked.update(g0=g0, log=[(cellf, g0, capi.unpack_code(x), capi.unpack_code(y)) for x, y in first + second])
    o, c = _run(s, BASE_O, BASE_G, save=True, pre=pre)
    rows, _ = _targets(c, s.side)
    assert rows == fm.record_merges(picked["log"]) and len(rows) == 3
    _check(s, o, c, about=(fm.NO_GENE,), identity=False)
    # one hop: the reads of mine[0] are written under mine[1], where no molecule is any more -- as the reference writes them
    verdict, cell, umi = c.read_corrections()
    src0, tgt0 = picked["log"][0][2], picked["log"][0][3]
    mine = [i for i in range(len(s.cell)) if s.cell[i] == cellf and s.gene[i] == picked["g0"] and s.umi_text[i] == src0]
    assert mine and all(verdict[i] == fm.WRITTEN and capi.unpack_code(umi[i], s.side) == tgt0 for i in mine)


@pytest.mark.parametrize("n_reads", [1, 65])
def test_short_streams(n_reads):
    s = Stream(11, n_reads=n_reads)
    kw_o, kw_g = dict(BASE_O, min_genes_before=0, min_genes_after=0), dict(BASE_G, min_genes_before_merge=0, min_genes_after_merge=0)
    o, c = _run(s, kw_o, kw_g, save=True)
    mols = _final_molecules(o)
    genes = [None if g == capi.NO_GENE else int(g) for g in s.gene]
    want_v, want_c, want_u = fm.decide_reads([int(x) for x in s.cell], genes, s.umi_text, o.merge_targets(), o.filtered_cells(), mols, {})
    verdict, cell, umi = c.read_corrections()
    assert verdict.tolist() == want_v and cell.tolist() == [0xFFFFFFFF if x is None else x for x in want_c]
    assert [capi.unpack_code(x, s.side) for x in umi] == want_u
    assert fm.WRITTEN in want_v and c.read_correction_counts().tolist() == [want_v.count(v) for v in range(5)]


def test_corrections_are_never_stale():
    s = Stream(12, n_umis=60)
    o, c = _run(s, BASE_O, BASE_G, save=True)
    first = _check(s, o, c, about=(fm.NO_GENE,), identity=True, min_sources=20)
    n, pv, pc, pu = c.read_corrections_device()
    assert n == N_READS and pv and pc and pu
    # a mutator changes the container: the next question is answered from the new state
    victim = int(o.filtered_cells()[0])
    c.exclude_cell(victim); o.exclude_cell(victim)
    verdict, _, _ = c.read_corrections()
    mine = (s.cell == victim) & (s.gene != capi.NO_GENE)
    assert mine.sum() >= 100 and set(verdict[mine].tolist()) == {fm.CELL_NOT_KEPT}
    assert np.array_equal(verdict[~mine], first[0][~mine])
    # reset: nothing to answer from, and the targets are gone; the same pass again gives the first answer again
    c.reset_results()
    with pytest.raises(capi.DropestError):
        c.read_corrections()
    with pytest.raises(capi.DropestError):
        c.umi_merge_targets()
    c.set_initialized(); c.merge_and_filter()
    again = c.read_corrections()
    assert all(np.array_equal(a, b) for a, b in zip(again, first))
    with pytest.raises(capi.DropestError):
        c.set_save_umi_merge_targets(False)                                  # after merge_and_filter
