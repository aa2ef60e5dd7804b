"""The inputs of the directional UMI correction tests (test_directional_model_cpu.py runs them through directional_model.py and the
oracle, test_gpu_directional.py through the device): hand-built streams, each at the smallest size at which the code it is named for can
still go wrong.

A case holds its reads [(barcode, gene or None, UMI)] in stream order, mult, max_ed and min_genes, and what it expects of the library:
  routes    how many (real cell, gene) groups go which way: "thread" (2 .. 16 clean UMIs of one length, one thread each), "wave"
            (17 .. 4096, libstdc++'s introsort restated, one wave each), "huge" (beyond, work arrays in global scratch), "host" (an N-UMI,
            or a stream with UMIs of several lengths: replayed on the host)
  rekeyed   the UMIs re-keyed by the device (count:umi_rekeyed); fallbacks: how many times the model's introsort reaches its heapsort
Both are written down by the builder, not taken from the model: test_directional_model_cpu.py holds them against the model,
test_gpu_directional.py against kernel_stats().  mult_edges, edit_distance and the host routes are one case per multiplier, per max_ed and
per reason (mult_edges_1.1, edit_distance_3, host_n, ...): a stream has one configuration.
What a case claims beyond that is said in its builder's docstring and asserted in test_directional_model_cpu.py."""
import random
from functools import lru_cache

import numpy as np

import directional_model as dm

NO_GENE = 0xFFFFFFFF
ESCAPE = 1 << 63
ACGT = "ACGT"
ROUTES = ("thread", "wave", "huge", "host")


def text(code, length):
    return "".join(ACGT[(code >> (2 * (length - 1 - i))) & 3] for i in range(length))


def pack(seq):
    code = 1
    for ch in seq:
        code = (code << 2) | ACGT.index(ch)
    return code


def barcode(i):
    return "ACGTACGT" + text(i, 4)


class Case:
    def __init__(self, name, reads, mult, max_ed, routes, rekeyed, min_genes=1, fallbacks=0, cuts=None):
        self.name, self.reads, self.mult, self.max_ed, self.min_genes = name, list(reads), mult, max_ed, min_genes
        self.routes = dict(dict.fromkeys(ROUTES, 0), **routes)
        self.rekeyed, self.fallbacks, self.cuts = rekeyed, fallbacks, cuts
        self.side = list(dm.first_seen(u for _, g, u in self.reads if g is not None and "N" in u))   # first seen over gene-bearing reads
        assert all("N" not in u for _, g, u in self.reads if g is None)

    def arrays(self):
        """(cb, umi, gene, aux) as the C-ABI takes them: packed codes, an N-UMI as an index into the side strings, gene ids by first occurrence"""
        genes = dm.first_seen(g for _, g, _ in self.reads if g is not None)
        cb = [pack(b) for b, _, _ in self.reads]
        umi = [ESCAPE | self.side.index(u) if "N" in u else pack(u) for _, _, u in self.reads]
        gene = [NO_GENE if g is None else genes[g] for _, g, _ in self.reads]
        return (np.array(cb, np.uint64), np.array(umi, np.uint64), np.array(gene, np.uint32), np.full(len(cb), 2 << 16, np.uint32))

    def kw(self):
        """capi.Context keyword arguments (test_gpu_multi_oracle.oracle_kw turns them into the oracle's)"""
        return dict(umi_merge_kind=1, max_umi_merge_edit_distance=self.max_ed, umi_merge_multiplier=self.mult,
                    min_genes_before_merge=self.min_genes, min_genes_after_merge=self.min_genes)

    def routes_taken(self):
        """the routes of the groups by size and content (k_umi_directional.h: directional_kernel), from the stream alone"""
        groups = dm.stream_of(self).groups
        one_length = len({len(u) for _, g, u in self.reads if g is not None and "N" not in u}) == 1
        out = dict.fromkeys(ROUTES, 0)
        for umis in groups.values():
            has_n = any("N" in u for u, _ in umis)
            if len(umis) < 2 and not has_n:
                continue
            out["host" if has_n or not one_length else "huge" if len(umis) > 4096 else "wave" if len(umis) > 16 else "thread"] += 1
        return out

    def fallbacks_of_the_model(self):
        return sum(dm.std_sort_order([r for _, r in umis])[1] for umis in dm.stream_of(self).groups.values())


def group_reads(cell, gene, umis):
    """the reads of one group: the first occurrences in the listed order (= the UMI-index order, unless a sequence was seen before), then the rest"""
    b = barcode(cell)
    return [(b, gene, u) for u, _ in umis] + [(b, gene, u) for u, r in umis for _ in range(r - 1)]


def block_prefix(block):
    """7 bases, any two of them at least two substitutions apart: six free bases and their sum as a check base"""
    assert 0 <= block < 4 ** 6
    return text(block, 6) + ACGT[sum((block >> (2 * i)) & 3 for i in range(6)) % 4]


def tied_neighbours(reads, first_block=0):
    """8-base sequences for a read-count vector (in index order) under which exactly the UMIs of EQUAL read counts are Hamming-1
    neighbours: every class of equal counts is cut, in index order, into blocks of up to four UMIs that differ in their last base; blocks
    are at least two substitutions apart.  Under mult = 1.0 every UMI of a block then falls to the one that std::sort leaves uppermost:
    the answer shows how the sort arranges equal elements.  Returns (sequences, next free block)."""
    rank, seqs, block_of, block = {}, [], {}, first_block
    for r in reads:
        k = rank.get(r, 0)
        rank[r] = k + 1
        if (r, k // 4) not in block_of:
            block_of[r, k // 4] = block
            block += 1
        seqs.append(block_prefix(block_of[r, k // 4]) + ACGT[k % 4])
    return seqs, block


def tied_group(reads, first_block=0):
    seqs, block = tied_neighbours(reads, first_block)
    return list(zip(seqs, reads)), block


def collapsing(umis):
    """the UMIs of a tied_group that fall to another at mult = 1.0: all but one of every block"""
    return len(umis) - len({u[:7] for u, _ in umis})


def killer_reads(n, factor):
    """killer(n) with every read count shared by `factor` UMIs"""
    return [v // factor + 1 for v in dm.killer(n)]


# ---- the cases ------------------------------------------------------------------------------------------------------------------
FIXTURE = [("AAA", 2), ("AAC", 5), ("AAT", 6), ("AGT", 20), ("CCC", 10), ("TCC", 20)]


def fixture():
    """The UMI list of testUMIMergeStrategyDirectional (Tests/TestEstimation.cpp:588-608) behind a common prefix of three bases (distances
    and read counts are the test's): AAA and AAT collapse into AGT, CCC into TCC."""
    return Case("fixture", group_reads(0, "g0", [("GTA" + u, r) for u, r in FIXTURE]), 2.0, 1, {"thread": 1}, 3)


BOUNDARY_17 = [2, 1, 3, 1, 2, 2, 3, 1, 1, 2, 3, 3, 1, 2, 1, 3, 2]             # index order; see boundary_16_17
BOUNDARY_SIZES = (2, 15, 16, 17, 18, 33)


def boundary_16_17():
    """mult = 1.0, tied UMIs are Hamming-1 neighbours (tied_neighbours).  Cell 0, gene "a": the 17 UMIs of BOUNDARY_17 -- introsort's own
    arrangement of the ties; gene "b": the first 16 of them with the same read counts -- a stable insertion sort, (reads, first occurrence).
    Cells 1 ..: groups of 2, 15, 16, 17, 18 and 33 UMIs with seeded tie-laden read counts, on sequences of their own."""
    umis, block = tied_group(BOUNDARY_17)
    reads = group_reads(0, "a", umis) + group_reads(0, "b", umis[:16])
    rekeyed = collapsing(umis) + collapsing(umis[:16])
    rng = random.Random(16)
    for cell, k in enumerate(BOUNDARY_SIZES, 1):
        other, block = tied_group([rng.choice((1, 1, 2, 2, 3)) for _ in range(k)], block)
        reads += group_reads(cell, "a", other)
        rekeyed += collapsing(other)
    return Case("boundary_16_17", reads, 1.0, 1, {"thread": 4, "wave": 4}, rekeyed)


def heap_fallback_64():
    """killer(64) with every read count shared by two UMIs, which are Hamming-1 neighbours: at mult = 1.0 one of each pair falls to the
    other, and which one is the sort's doing.  The model's introsort reaches its heapsort once."""
    umis, _ = tied_group(killer_reads(64, 2))
    return Case("heap_fallback_64", group_reads(0, "g", umis), 1.0, 1, {"wave": 1}, 32, fallbacks=1)


# (UMIs, tie factor): the largest factor of all -- the fewest reads -- at which the model's introsort still reaches the heapsort on killer(n)
# (every factor up to n was tried once; test_directional_model_cpu.py repeats a part of that scan)
WAVE = ((680, 73), (4096, 519))
HUGE = (4200, 532)


def heap_fallback_wave():
    """The same with 680 UMIs in cell 0 and exactly 4096 in cell 1 (the wave kernel's last size), at tie factors 73 and 519: classes of
    equal read counts of several hundred UMIs, cut into blocks of four neighbours."""
    reads, block, rekeyed = [], 0, 0
    for cell, (n, factor) in enumerate(WAVE):
        umis, block = tied_group(killer_reads(n, factor), block)
        reads += group_reads(cell, "g", umis)
        rekeyed += collapsing(umis)
    return Case("heap_fallback_wave", reads, 1.0, 1, {"wave": 2}, rekeyed, fallbacks=2)


def heap_fallback_huge():
    """One group of 4200 UMIs: the global-scratch kernel (32-bit index vector) with the heapsort reached."""
    umis, _ = tied_group(killer_reads(*HUGE))
    return Case("heap_fallback_huge", group_reads(0, "g", umis), 1.0, 1, {"huge": 1}, collapsing(umis), fallbacks=1)


MULT_PAIRS = {   # mult: [(reads of the lesser UMI, reads of its Hamming-1 neighbour, merges?)]: on, below and above the line
    1.0: [(4, 4, True), (4, 5, True), (3, 4, True)],
    1.5: [(2, 3, True), (2, 2, False), (2, 4, True), (4, 6, True), (4, 5, False)],                  # 2 * 1.5 > 3 is false: a candidate
    2.0: [(3, 6, True), (3, 5, False), (3, 7, True), (1, 2, True), (1, 1, False)],
    # 1.1 is no double; 10 * 1.1 lies exactly between 11 and the next double and rounds (to even) to 11.0 -- a candidate -- while 50 * 1.1
    # rounds to 55.00000000000001 > 55: the search breaks
    1.1: [(10, 11, True), (10, 10, False), (10, 12, True), (50, 55, False), (50, 56, True), (50, 54, False), (5, 6, True), (5, 5, False)],
}
assert 10 * 1.1 == 11.0 and 50 * 1.1 > 55 and 2 * 1.5 == 3.0


def mult_edges(mult):
    """One pair of Hamming-1 neighbours per gene, read counts exactly on, one below and one above reads(src) * mult in double arithmetic"""
    reads = []
    for g, (low, high, _) in enumerate(MULT_PAIRS[mult]):
        reads += group_reads(0, "g%d" % g, [(block_prefix(g) + "A", low), (block_prefix(g) + "C", high)])
    return Case("mult_edges_%.1f" % mult, reads, mult, 1, {"thread": len(MULT_PAIRS[mult])}, sum(m for _, _, m in MULT_PAIRS[mult]))


def substituted(seq, *positions):
    s = list(seq)
    for p in positions:
        s[p] = ACGT[(ACGT.index(s[p]) + 1) % 4]
    return "".join(s)


def edit_distance_case(max_ed):
    """mult = 2.0, one gene each (src is the UMI with one read; `far` is max_ed substitutions from it, `near` one fewer):
      indel     ACGTACGT / CGTACGTA: one deletion and one insertion apart, Hamming distance 8 -- merged
      displaced far (9 reads), near (5 reads): the first hit at max_ed is displaced by the later, nearer one -- src falls to near
      kept      far (9 reads), another far (5 reads): the first hit stays against a later one as far away -- src falls to the 9-read UMI
      breaks    a Hamming-1 neighbour with 9 reads, another with 5: the search ends at the first
      exact     a pair exactly max_ed apart -- merged; beyond: a pair max_ed + 1 apart -- left alone"""
    src = {"displaced": "AAAAAAAA", "kept": "CCCCCCCC", "breaks": "GGGGGGGG", "exact": "TTTTTTTT", "beyond": "AACCGGTT"}
    far = tuple(range(max_ed))
    groups = {
        "indel": [("ACGTACGT", 1), ("CGTACGTA", 5)],
        "displaced": [(src["displaced"], 1), (substituted(src["displaced"], *far), 9), (substituted(src["displaced"], *far[1:]), 5)],
        "kept": [(src["kept"], 1), (substituted(src["kept"], *far), 9), (substituted(src["kept"], *range(4, 4 + max_ed)), 5)],
        "breaks": [(src["breaks"], 1), (substituted(src["breaks"], 0), 9), (substituted(src["breaks"], 7), 5)],
        "exact": [(src["exact"], 1), (substituted(src["exact"], *far), 5)],
        "beyond": [(src["beyond"], 1), (substituted(src["beyond"], *range(0, 2 * max_ed + 2, 2)), 5)],
    }
    assert dm.levenshtein(*[u for u, _ in groups["indel"]]) == 2 and dm.hamming(*[u for u, _ in groups["indel"]]) == 8
    assert dm.levenshtein(*[u for u, _ in groups["exact"]]) == max_ed and dm.levenshtein(*[u for u, _ in groups["beyond"]]) == max_ed + 1
    for name in ("displaced", "kept"):
        (s, _), (a, _), (b, _) = groups[name]
        assert (dm.levenshtein(s, a), dm.levenshtein(s, b)) == (max_ed, max_ed - 1 if name == "displaced" else max_ed)
        assert dm.levenshtein(a, b) > max_ed or name == "displaced"
    reads = []
    for gene, umis in groups.items():
        reads += group_reads(0, gene, umis)
    return Case("edit_distance_%d" % max_ed, reads, 2.0, max_ed, {"thread": 6}, 5)


def chains():
    """mult = 2.0, max_ed = 1.  Gene "line": a -> b -> c -> d by read counts 1, 2, 4, 8, each one substitution from the next only: all three
    end at d.  Gene "join": e (1) and f (2) both fall to g (4), g to h (8): all three end at h."""
    line = [("AAAAAA", 1), ("AAAAAC", 2), ("AAAACC", 4), ("AAACCC", 8)]
    join = [("GGGGGT", 1), ("GGGGTG", 2), ("GGGGGG", 4), ("GGGCGG", 8)]
    return Case("chains", group_reads(0, "line", line) + group_reads(0, "join", join), 2.0, 1, {"thread": 2}, 6)


def owner(cell, world):
    """the shard that holds a cell's reads after the exchange: mix64(barcode code) mod world, mix64 = the splitmix64 finaliser (util.h)"""
    x = pack(barcode(cell))
    x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & (2 ** 64 - 1)
    x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & (2 ** 64 - 1)
    return (x ^ (x >> 31)) % world


SIGHTING_CELL = next(i for i in range(3, 256) if all(owner(i, w) != owner(1, w) for w in (2, 3)))   # a barcode that lives on another shard than barcode(1)


INDEX_ORDER_GENES = ("cell", "gene", "geneless")


def index_order_umis(gene):
    """X, Y, Z: X - Y and Y - Z one substitution apart, X - Z two"""
    base = block_prefix(INDEX_ORDER_GENES.index(gene))
    return base + "A", base + "C", substituted(base + "C", 0)


def index_order():
    """mult = 1.0, max_ed = 1, min_genes = 1.  Cell 0 is barcode(SIGHTING_CELL), cell 1 barcode(1).  Three genes of cell 1 hold X, Y, Z of
    three reads each, read in this order (index_order_umis).  In the order X, Y, Z both X and Y end at Z: one UMI is left.  In the order
    Y, X, Z only Y falls to Z -- X finds no neighbour above itself: two UMIs are left, so the count matrix shows the order too.  Y was seen
    earlier in the stream
      "cell"      in cell 0 (gene "early"): Y has the lowest UMI index, X and Z are left
      "gene"      in another gene of cell 1 itself ("other"): X and Z are left
      "geneless"  in a read of cell 0 without a gene, which takes no part in the index: Z alone is left
    The sightings open the stream, 60 reads of cell 2 (single UMIs) follow, the three groups close it: cuts = the bounds of two and of three
    shards with the sightings on the first shard and the groups on the last -- and after the exchange by barcode cell 0 and cell 1 still lie
    on different shards, whichever side of it the first occurrences are taken on."""
    sighting = barcode(SIGHTING_CELL)
    early = [(sighting, "early", index_order_umis("cell")[1]), (barcode(1), "other", index_order_umis("gene")[1]),
             (sighting, None, index_order_umis("geneless")[1])]
    filler = [(barcode(2), "f%d" % (i % 20), block_prefix(100 + i % 20) + "G") for i in range(60)]
    groups = []
    for g in INDEX_ORDER_GENES:
        groups += group_reads(1, g, [(u, 3) for u in index_order_umis(g)])
    reads = early + filler + groups
    first_group_read = len(early) + len(filler)
    return Case("index_order", reads, 1.0, 1, {"thread": 3}, 4,
                cuts={2: [0, first_group_read, len(reads)], 3: [0, len(early) + len(filler) // 2, first_group_read, len(reads)]})


def untouched():
    """min_genes = 2, mult = 2.0.  Cell 0 (real): two genes of one UMI each, and gene-less reads whose UMIs would merge; cell 1 (one gene: not
    real): a group that would merge; cell 2 (real): one group that does merge, and one of a single UMI.  Only cell 2's pair is re-keyed."""
    pair = [("ACACAC", 1), ("ACACAG", 5)]
    reads = group_reads(0, "a", [("TTTTTT", 4)]) + group_reads(0, "b", [("TTTTTG", 9)]) + group_reads(0, None, pair)
    reads += group_reads(1, "a", pair)
    reads += group_reads(2, "a", pair) + group_reads(2, "b", [("ACACAC", 2)])
    return Case("untouched", reads, 2.0, 1, {"thread": 1}, 1, min_genes=2)


def host_n():
    """One group with an N-UMI beside a clean pair in another gene: the first is replayed on the host, the second decided by a thread."""
    reads = group_reads(0, "n", [("ACGTAC", 1), ("ACGNAC", 2), ("ACGTAG", 6)]) + group_reads(0, "clean", [("CCCCCC", 1), ("CCCCCG", 4)])
    return Case("host_n", reads, 2.0, 1, {"host": 1, "thread": 1}, 1)


def host_two_lengths():
    """UMIs of six and of seven bases in one stream: every group of two and more UMIs is the host's (the banded distance is no Levenshtein
    distance between strings of two lengths)."""
    reads = group_reads(0, "mixed", [("ACGTAC", 1), ("ACGTACG", 5), ("ACGTAG", 6)]) + group_reads(0, "six", [("CCCCCC", 1), ("CCCCCG", 4)])
    reads += group_reads(0, "single", [("GGGGGGG", 3)])
    return Case("host_two_lengths", reads, 2.0, 1, {"host": 2}, 0)


BUILDERS = {"fixture": fixture, "boundary_16_17": boundary_16_17, "heap_fallback_64": heap_fallback_64, "heap_fallback_wave": heap_fallback_wave,
            "heap_fallback_huge": heap_fallback_huge, "edit_distance_2": lambda: edit_distance_case(2), "edit_distance_3": lambda: edit_distance_case(3),
            "chains": chains, "index_order": index_order, "untouched": untouched, "host_n": host_n, "host_two_lengths": host_two_lengths}
BUILDERS.update({"mult_edges_%.1f" % m: (lambda m=m: mult_edges(m)) for m in MULT_PAIRS})
NAMES = sorted(BUILDERS)
HOST = ("host_n", "host_two_lengths")
MODELLED = [n for n in NAMES if n not in HOST]
LAYOUT_CASES = ("boundary_16_17", "heap_fallback_64", "edit_distance_2", "edit_distance_3")


@lru_cache(maxsize=None)
def case(name):
    c = BUILDERS[name]()
    assert c.name == name
    return c


@lru_cache(maxsize=None)
def expected(name):
    """the model's answer, computed once and shared by the tests"""
    return dm.run(case(name))
