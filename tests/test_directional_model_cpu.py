"""directional_model.py pinned on the oracle (no GPU), piece by piece, and the claims of directional_cases.py.

  std_sort_order   equals the order of the oracle's real std::sort (the sort of its find_targets, through orc_directional_sort_order) on
                   every group of every case, on killer(n) at tie factors 1, 2 and 4, and on seeded tie-heavy vectors; and -- through
                   Oracle.directional_targets on tied_neighbours sequences at mult = 1.0 -- which UMI of every block of tied neighbours
                   the oracle leaves uppermost
  find_targets     equals Oracle.directional_targets on every group of every modelled case
  run              equals the oracle's container: molecules and total_umis
  edit_distance    equals the oracle's on all pairs of every group (of a group beyond 40 UMIs: all pairs of its first 40 and 2000 pairs drawn
                   over the whole group), and on all pairs of 4-base strings at max_ed 1 .. 3; it equals the plain
                   Levenshtein distance whenever either is within max_ed (what k_umi_directional.h relies on)
  teeth            every wrong variant of directional_model.VARIANTS changes the expected answer of the cases named for it
  routes           the groups of every case take the routes it declares
  shards           what a sharded run shows -- the count matrix's UMIs per (cell, gene), the UMI every read is written under -- changes on
                   index_order if a shard takes the first occurrences among its own reads only"""
import ctypes
import itertools
import random
from functools import lru_cache

import pytest

import directional_cases as dc
import directional_model as dm
from oracle import Oracle, binding as ob

_libc = ctypes.CDLL("libc.so.6")
KILLER_SIZES = (17, 33, 64, 100, 256, 1000, 4096)
TIE_FACTORS = (1, 2, 4)


def oracle_cfg(c):
    return dict(umi_merge_kind=1, max_umi_merge_ed=c.max_ed, umi_mult=c.mult, min_genes_before=c.min_genes, min_genes_after=c.min_genes)


@lru_cache(maxsize=None)
def oracle_of(name):
    """The oracle's container over the case's stream after merge_and_filter.  The directional strategy never seeds rand(): a fresh
    reference process starts from srand(1)."""
    c = dc.case(name)
    _libc.srand(1)
    o = Oracle(**oracle_cfg(c))
    o.add_packed(*c.arrays(), c.side)
    o.set_initialized()
    o.merge_and_filter()
    return o


# ---- std::sort ------------------------------------------------------------------------------------------------------------------
def tie_heavy(n, seed):
    rng = random.Random(seed)
    return [rng.choice((1, 1, 1, 2, 2, 3, 5, 9)) for _ in range(n)]     # the read counts of test_directional_very_large_groups


def sort_vectors():
    out = {}
    for name in dc.MODELLED:
        for key, umis in dm.stream_of(dc.case(name)).groups.items():
            out["%s:%d:%d" % ((name,) + key)] = [r for _, r in umis]
    for n in KILLER_SIZES:
        for f in TIE_FACTORS:
            out["killer(%d)/%d" % (n, f)] = dc.killer_reads(n, f)
    for seed, n in enumerate((17, 40, 300, 5000)):
        out["tie_heavy(%d)" % n] = tie_heavy(n, seed)
    return out


def test_std_sort_order_equals_the_oracles_std_sort():
    fallbacks = {}
    for label, reads in sort_vectors().items():
        order, fallbacks[label] = dm.std_sort_order(reads)
        assert order == ob.directional_sort_order(reads), label
        assert sorted(order) == list(range(len(reads))) and [reads[i] for i in order] == sorted(reads)
    # random read counts never reach the heapsort, the adversary does from 64 elements on -- with distinct counts and with every count shared
    assert not any(n for label, n in fallbacks.items() if label.startswith("tie_heavy"))
    for n in KILLER_SIZES:
        for f in (1, 2):
            assert (fallbacks["killer(%d)/%d" % (n, f)] >= 1) == (n >= 64), (n, f)
    assert fallbacks["killer(4096)/4"] >= 1


def uppermost_of_blocks(umis, order):
    """{UMI: the UMI of its block at the highest sorted position} for the others of every block of a tied_group"""
    at = {umis[i][0]: p for p, i in enumerate(order)}
    top = {}
    for u in at:
        if u[:7] not in top or at[u] > at[top[u[:7]]]:
            top[u[:7]] = u
    return {u: top[u[:7]] for u in at if top[u[:7]] != u}


@pytest.mark.parametrize("label,reads", [("killer(%d)/%d" % (n, f), (n, f)) for n in KILLER_SIZES for f in (2, 4)] +
                         [("tie_heavy(%d)" % n, (n, None)) for n in (17, 40, 300, 1500)])
def test_the_order_of_ties_shows_in_the_oracles_targets(label, reads):
    """The same through the function under test itself: on tied_neighbours sequences at mult = 1.0 every UMI falls to the one of its block
    that the oracle's sort left uppermost (at tie factor 2 that is the whole order of the ties)."""
    n, f = reads
    reads = dc.killer_reads(n, f) if f else tie_heavy(n, n)
    umis, _ = dc.tied_group(reads)
    got = Oracle(umi_merge_kind=1, max_umi_merge_ed=1, umi_mult=1.0).directional_targets(umis)
    assert got == uppermost_of_blocks(umis, dm.std_sort_order(reads)[0])
    assert len(got) == dc.collapsing(umis) > 0


def test_killer_drives_the_sort_into_its_heapsort():
    for n in (64, 100, 680, 4096, 4200):
        k = dm.killer(n)
        assert sorted(k) == list(range(n)) and dm.std_sort_order(k)[1] >= 1


@pytest.mark.parametrize("n,f", dc.WAVE + (dc.HUGE,))
def test_the_tie_factors_of_the_large_cases_are_the_largest(n, f):
    """The heapsort is reached at factor f and at no larger one.  Every factor up to n was tried when the cases were built (73 of 680, 519
    of 4096, 532 of 4200; a minute of sorting); here all of them for 680, and for the two large sizes the next 128 and every 16th beyond."""
    k = dm.killer(n)
    assert dm.std_sort_order([v // f + 1 for v in k])[1] >= 1
    larger = range(f + 1, n + 1) if n < 1000 else list(range(f + 1, f + 129)) + list(range(f + 129, n + 1, 16))
    for g in larger:
        assert dm.std_sort_order([v // g + 1 for v in k])[1] == 0, (n, g)


# ---- distances ------------------------------------------------------------------------------------------------------------------
def check_distance(a, b, max_ed):
    banded, plain = dm.edit_distance(a, b, max_ed), dm.levenshtein(a, b)
    assert banded == ob.edit_distance(a, b, True, max_ed), (a, b, max_ed)
    if banded <= max_ed or plain <= max_ed:
        assert banded == plain, (a, b, max_ed)
    else:
        assert banded > max_ed                      # (a lower bound of its own past the band: only "too far" is used)


def test_edit_distance_on_the_pairs_of_the_cases():
    n = 0
    for name in dc.MODELLED:
        c = dc.case(name)
        for umis in dm.stream_of(c).groups.values():
            pairs = itertools.permutations(umis, 2)
            if len(umis) > 40:       # a large group: all pairs of its first 40 UMIs and 2000 pairs drawn over the whole of it
                rng = random.Random(len(umis))
                pairs = itertools.chain(itertools.permutations(umis[:40], 2), (rng.sample(umis, 2) for _ in range(2000)))
            for (a, _), (b, _) in pairs:
                check_distance(a, b, c.max_ed)
                n += 1
    assert n > 10000
    assert dm.edit_distance("ACGTACGT", "CGTACGTA", 2) == 2 and dm.hamming("ACGTACGT", "CGTACGTA") == 8


@pytest.mark.parametrize("max_ed", [1, 2, 3])
def test_edit_distance_on_all_pairs_of_four_bases(max_ed):
    words = [dc.text(i, 4) for i in range(256)]
    for a in words:
        for b in words:
            check_distance(a, b, max_ed)


# ---- find_targets and the whole stream ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.MODELLED)
def test_find_targets_equals_the_oracle(name):
    c = dc.case(name)
    o = Oracle(**oracle_cfg(c))
    groups = dm.stream_of(c).groups
    assert groups
    for key, umis in groups.items():
        want = o.directional_targets(umis)
        assert dm.find_targets(umis, c.mult, c.max_ed) == want, (name, key)
        if c.max_ed == 1 and len(umis) <= 700:       # the lookup that serves the groups of thousands, against the literal search
            assert dm.find_targets(umis, c.mult, 1, by_lookup=True) == dm.find_targets(umis, c.mult, 1, by_lookup=False) == want
        assert dc.expected(name).targets.get(key, {}) == want


def test_find_targets_refuses_what_the_host_replays():
    with pytest.raises(ValueError):
        dm.find_targets([("ACGT", 1), ("ACNT", 2)], 2.0, 1)
    with pytest.raises(ValueError):
        dm.find_targets([("ACGT", 1), ("ACGTA", 2)], 2.0, 1)
    for name in dc.HOST:
        with pytest.raises(ValueError):
            dm.run(dc.case(name))


@pytest.mark.parametrize("name", dc.MODELLED)
def test_run_equals_the_oracles_container(name):
    c = dc.case(name)
    want, o = dc.expected(name), oracle_of(name)
    st = want.stream
    assert [o.cell_barcode(i) for i in range(o.n_cells)] == sorted(st.cells, key=st.cells.get)
    assert [o.gene_name(i) for i in range(o.n_genes)] == ["G%d" % i for i in range(len(st.genes))]   # (packed reads name their genes by id)
    cell, gene, umi, reads, _ = o.molecules()
    got = {(int(a), int(b), u): int(r) for a, b, u, r in zip(cell, gene, umi, reads)}
    assert len(got) == len(cell) and got == want.molecules
    assert {i: int(x) for i, x in enumerate(o.cell_rows()[:, 7])} == want.total_umis
    assert sum(want.removed.values()) == sum(len(t) for t in want.targets.values()) == c.rekeyed


# ---- what the cases claim -------------------------------------------------------------------------------------------------------
def targets_by_gene(name, variant=()):
    c = dc.case(name)
    res = dm.run(c, variant) if variant else dc.expected(name)
    gene_of = {i: g for g, i in res.stream.genes.items()}
    return {(cell, gene_of[g]): t for (cell, g), t in res.targets.items()}


def test_the_hand_derived_answers():
    """what the small cases are built to show, written out"""
    assert targets_by_gene("fixture") == {(0, "g0"): {"GTAAAA": "GTAAGT", "GTAAAT": "GTAAGT", "GTACCC": "GTATCC"}}
    assert targets_by_gene("chains") == {(0, "line"): {"AAAAAA": "AAACCC", "AAAAAC": "AAACCC", "AAAACC": "AAACCC"},
                                         (0, "join"): {"GGGGGT": "GGGCGG", "GGGGTG": "GGGCGG", "GGGGGG": "GGGCGG"}}
    want = {}
    for g in dc.INDEX_ORDER_GENES:
        x, y, z = dc.index_order_umis(g)
        assert (dm.hamming(x, y), dm.hamming(y, z), dm.hamming(x, z)) == (1, 1, 2)
        want[1, g] = {x: z, y: z} if g == "geneless" else {y: z}             # Y seen earlier in a gene-bearing read: X finds nothing above itself
    assert targets_by_gene("index_order") == want
    assert targets_by_gene("untouched") == {(2, "a"): {"ACACAC": "ACACAG"}}
    assert dc.expected("untouched").total_umis == {0: 2, 1: 2, 2: 2}
    for mult, pairs in dc.MULT_PAIRS.items():
        got = targets_by_gene("mult_edges_%.1f" % mult)
        assert {g for _, g in got} == {"g%d" % i for i, (_, _, merges) in enumerate(pairs) if merges}, mult
    for max_ed in (2, 3):
        got = targets_by_gene("edit_distance_%d" % max_ed)
        assert set(got) == {(0, g) for g in ("indel", "displaced", "kept", "breaks", "exact")}
        assert got[0, "indel"] == {"ACGTACGT": "CGTACGTA"}
        far = dc.substituted("AAAAAAAA", *range(max_ed))
        assert got[0, "displaced"] == {"AAAAAAAA": dc.substituted("AAAAAAAA", *range(1, max_ed))} and far not in got[0, "displaced"].values()
        assert got[0, "kept"] == {"CCCCCCCC": dc.substituted("CCCCCCCC", *range(max_ed))}
        assert got[0, "breaks"] == {"GGGGGGGG": dc.substituted("GGGGGGGG", 0)}


def test_the_same_ties_on_both_sides_of_16():
    """gene "a" of cell 0: 17 UMIs in introsort's arrangement; gene "b": its first 16, stably sorted.  The 17 fall otherwise than a stable
    sort would have them, the 16 exactly so; and one UMI that both groups hold falls to another target in each."""
    c = dc.case("boundary_16_17")
    got, stable = targets_by_gene("boundary_16_17"), targets_by_gene("boundary_16_17", {"stable_sort"})
    assert got[0, "a"] != stable[0, "a"] and got[0, "b"] == stable[0, "b"]
    groups = dm.stream_of(c).groups
    assert [len(g) for g in groups.values()] == [17, 16] + list(dc.BOUNDARY_SIZES)
    assert groups[0, 0][:16] == groups[0, 1]
    assert any(got[0, "a"].get(u) != t for u, t in got[0, "b"].items())


TEETH = {
    "stable_sort": ("boundary_16_17", "heap_fallback_64", "heap_fallback_wave", "heap_fallback_huge"),
    "no_heap_fallback": ("heap_fallback_64", "heap_fallback_wave", "heap_fallback_huge"),
    "hamming": ("edit_distance_2", "edit_distance_3"),
    "local_index": ("index_order",),
    "geneless_indexed": ("index_order",),
    "mult_ge": ("mult_edges_1.0", "mult_edges_1.5", "mult_edges_2.0", "mult_edges_1.1"),
    "ed_le": ("edit_distance_2", "edit_distance_3"),
    "no_chain": ("chains", "fixture"),
}


@pytest.mark.parametrize("variant,name", [(v, n) for v, names in TEETH.items() for n in names])
def test_every_wrong_variant_changes_a_named_case(variant, name):
    assert set(TEETH) == set(dm.VARIANTS)
    wrong = dm.run(dc.case(name), {variant})
    assert wrong.targets != dc.expected(name).targets
    assert wrong.molecules != dc.expected(name).molecules or variant == "no_chain"     # (the fold follows a chain to its end either way)


def test_heap_fallback_64_decides_with_ties_that_matter():
    c = dc.case("heap_fallback_64")
    assert c.fallbacks_of_the_model() >= 1 and 900 < len(c.reads) < 1200
    reads = [r for _, r in dm.stream_of(c).groups[0, 0]]
    assert sorted(reads) == sorted(2 * list(range(1, 33)))                               # every count shared by two UMIs
    assert dc.expected(c.name).targets != dm.run(c, {"stable_sort"}).targets
    assert dc.expected(c.name).targets != dm.run(c, {"no_heap_fallback"}).targets


@pytest.mark.parametrize("name", dc.NAMES)
def test_routes_and_counts_are_the_declared_ones(name):
    c = dc.case(name)
    assert c.routes_taken() == c.routes
    assert c.fallbacks_of_the_model() == c.fallbacks
    assert all(6 <= len(u) <= 8 for _, _, u in c.reads)
    assert len(c.reads) < (40_000 if name.startswith("heap_fallback") else 5000)
    if name == "index_order":    # the sightings on the first shard, the deciding groups on the last
        early = [i for i, (_, g, _) in enumerate(c.reads) if g in ("early", "other", None)]
        deciding = [i for i, (_, g, _) in enumerate(c.reads) if g in ("cell", "gene", "geneless")]
        for bounds in c.cuts.values():
            assert max(early) < bounds[1] and bounds[-2] <= min(deciding) and bounds[-1] == len(c.reads)
        assert c.reads[0][0] == dc.barcode(dc.SIGHTING_CELL) and {c.reads[i][0] for i in deciding} == {dc.barcode(1)}
        assert all(dc.owner(dc.SIGHTING_CELL, world) != dc.owner(1, world) for world in c.cuts)


# ---- what a sharded run of index_order must get right ---------------------------------------------------------------------------
def umis_per_group(result):
    out = {}
    for c, g, _ in result.molecules:
        out[c, g] = out.get((c, g), 0) + 1
    return out


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("known", ["range", "owned"])
def test_a_shard_that_knows_only_its_own_first_occurrences_answers_index_order_otherwise(world, known):
    """The UMI index taken among the reads of the deciding groups' shard alone -- those of its range of the stream, or those of the cells
    it owns after the exchange -- in place of the whole stream's: both observables of test_gpu_directional's sharded runs change."""
    c, want = dc.case("index_order"), dc.expected("index_order")
    bounds = c.cuts[world]
    barcode_index = {dc.barcode(k): k for k in (dc.SIGHTING_CELL, 1, 2)}
    seen_by = (range(bounds[-2], bounds[-1]) if known == "range" else
               [i for i, (b, _, _) in enumerate(c.reads) if dc.owner(barcode_index[b], world) == dc.owner(1, world)])
    wrong = dm.run(c, seen_by=seen_by)
    genes = want.stream.genes
    assert umis_per_group(wrong) != umis_per_group(want) and dm.written_umis(c, wrong) != dm.written_umis(c, want)
    assert umis_per_group(want)[1, genes["cell"]] == 2 and umis_per_group(wrong)[1, genes["cell"]] == 1
    assert (umis_per_group(wrong)[1, genes["gene"]] == 1) == (known == "range")      # (cell 1's own earlier sighting travels with the cell)
    assert umis_per_group(want)[1, genes["geneless"]] == umis_per_group(wrong)[1, genes["geneless"]] == 1
