"""The inputs of the -M estimator tests (test_poisson_model_cpu.py runs them through poisson_model.py and the oracle,
test_gpu_poisson_estimator.py through the device), built directly as (cell, gene, UMI) molecules.

Adjuster cases (ADJUSTER_NAMES): integer UMI counts and a largest size, for the stand-alone table entry; the sizes step around the
64 lanes of a wave, the 256 threads of a block and the 65 536 threads of its grid.
Container cases (CONTAINER_NAMES): molecules, the cell pairs to estimate, and -- the decision cases -- a whitelist and thresholds.
What a case claims about itself is asserted from the model where it is built or in test_poisson_model_cpu.py.

A container case numbers its cells and genes in the order of their first read, as the library does: one gene-less read per cell
opens the stream (cell ids = the order of `barcodes`), the molecules follow in (gene, cell, UMI) order.
"""
import random
from collections import Counter
from functools import lru_cache, partial

import numpy as np

import poisson_model as pm
import simple_merge_model as smm
import whitelist_model as wm

ACGT = "ACGT"
NO_GENE = 0xFFFFFFFF
MERGE_POISSON_REAL, MERGE_POISSON_SIMPLE = 3, 4          # capi.MERGE_* = the oracle's merge_kind


def pack(seq):
    code = 1
    for ch in seq:
        code = (code << 2) | ACGT.index(ch)
    return code


def text_of(number, length):
    return "".join(ACGT[(number >> (2 * (length - 1 - i))) & 3] for i in range(length))


# ---- adjuster cases ---------------------------------------------------------------------------------------------------------
class AdjusterCase:
    def __init__(self, name, counts, max_expression):
        self.name, self.counts, self.max_expression = name, [int(c) for c in counts], max_expression

    @property
    def probs(self):
        return pm.probabilities(self.counts)

    @lru_cache(maxsize=None)
    def model(self):
        """(table, margins, first diverged entry or None)"""
        try:
            table, margins = pm.adjusted_sizes(self.probs, self.max_expression)
            return table, margins, None
        except pm.CollisionsDiverged as e:
            return e.table, e.margins, e.at


def _counts(n, kind, order, seed):
    """n integer counts: uniform, a power law over a few dozen distinct values (affordable at any n), or n distinct values"""
    rng = random.Random(seed)
    if kind == "uniform":
        c = [3] * n
    elif kind == "twolevel":
        c = [1, 5] * (n // 2) + [1] * (n % 2)
    elif kind == "skewed":
        c = [1 + int(40 * (i / max(1, n - 1)) ** 4) for i in range(n)]          # 41 distinct values at most, most UMIs rare
    else:
        c = [1 + int(2000 / (i + 1) ** 0.7) + (n - i) for i in range(n)]          # "distinct": strictly falling
    if order == "random":
        rng.shuffle(c)
    elif order == "ascending":
        c.sort()
    else:
        c.sort(reverse=True)
    return c


def _adjuster_cases():
    out = {}
    k = 0
    for n in (1, 63, 64, 65, 255, 256, 257, 65535, 65536, 65537, 131073):
        # (131 073 equally likely UMIs: the first collision term itself, 1 / n = 7.6e-6, lies under the margin every case must keep
        # from an integer, so the flat distribution there has two levels)
        for kind in (("uniform",) if n < 100000 else ("twolevel",)) + ("skewed",) + (("distinct",) if 1 < n <= 1000 else ()):
            order = ("random", "ascending", "descending")[k % 3]
            k += 1
            if n == 1:
                smax = 1                                                            # one UMI: the second molecule must collide
            elif kind == "distinct":
                smax = min(300, n // 3)
            else:
                smax = min(20, max(2, n // 4))
            name = "adj_%d_%s_%s" % (n, kind, order)
            out[name] = partial(AdjusterCase, name, _counts(n, kind, order, 100 + k), smax)
    out["adj_1000_distinct_300"] = partial(AdjusterCase, "adj_1000_distinct_300", _counts(1000, "distinct", "random", 5), 300)
    # the fixed-order tree must not care: one distribution in all three orders
    for order in ("random", "ascending", "descending"):
        name = "adj_257_distinct_%s" % order
        out[name] = partial(AdjusterCase, name, _counts(257, "distinct", order, 7), 80)
    # few UMIs, sizes up to half their number: the collisions of one step exceed 1, floor(sum_collisions) steps by more than 1
    out["adj_40_steps"] = partial(AdjusterCase, "adj_40_steps", _counts(40, "uniform", "random", 9), 24)
    # 16 equally likely UMIs and sizes beyond their number: the recurrence diverges on the way
    out["adj_16_diverges"] = partial(AdjusterCase, "adj_16_diverges", [1] * 16, 40)
    return out


_ADJUSTER = _adjuster_cases()
ADJUSTER_NAMES = sorted(_ADJUSTER)


# ---- container cases --------------------------------------------------------------------------------------------------------
class ContainerCase:
    """molecules: {(cell, gene or None, umi number)}; cells are indices into `barcodes`; pairs: [(cell, cell)] to estimate.
    Decision cases also have parts (a CONST whitelist) and thresholds: list of (max_merge_prob, max_real_merge_prob)."""

    def __init__(self, name, barcodes, molecules, umi_len, min_genes, pairs, parts=None, thresholds=(), max_ed=1, hand_built=True):
        self.name, self.barcodes, self.umi_len, self.min_genes, self.pairs = name, list(barcodes), umi_len, min_genes, list(pairs)
        self.parts, self.thresholds, self.max_ed, self.hand_built = parts, list(thresholds), max_ed, hand_built
        assert len(set(self.barcodes)) == len(self.barcodes)
        mol = sorted(set(molecules), key=lambda m: (m[1] is None, m[1] if m[1] is not None else 0, m[0], m[2]))
        genes = sorted({g for _, g, _ in mol if g is not None})
        assert genes == list(range(len(genes))), "gene ids must be 0 .. n - 1"
        assert all(0 <= u < 4 ** umi_len for _, _, u in mol)
        self.molecules = mol
        self.container = {c: {} for c in range(len(self.barcodes))}
        for c, g, u in mol:
            if g is not None:
                self.container[c].setdefault(g, set()).add(u)
        self.n_genes = [len(self.container[c]) for c in range(len(self.barcodes))]
        self.total_umis = [sum(len(u) for u in self.container[c].values()) for c in range(len(self.barcodes))]
        # CellsDataContainer::update_filtered_gene_counts + compare_cells: genes, UMIs, barcode
        self.filtered = sorted((c for c in range(len(self.barcodes)) if self.n_genes[c] >= min_genes),
                               key=lambda c: (self.n_genes[c], self.total_umis[c], self.barcodes[c]))

    def arrays(self):
        """(cb, umi, gene, aux) of the read stream"""
        n_cells = len(self.barcodes)
        cb = [pack(b) for b in self.barcodes] + [pack(self.barcodes[c]) for c, _, _ in self.molecules]
        sentinel = 1 << (2 * self.umi_len)
        umi = [sentinel] * n_cells + [sentinel | u for _, _, u in self.molecules]
        gene = [NO_GENE] * n_cells + [NO_GENE if g is None else g for _, g, _ in self.molecules]
        return (np.array(cb, np.uint64), np.array(umi, np.uint64), np.array(gene, np.uint32), np.full(len(cb), 2 << 16, np.uint32))

    @lru_cache(maxsize=None)
    def estimator(self):
        return pm.Estimator(self.container, self.filtered)

    @property
    def n_classes(self):
        return len(self.estimator().classes)

    @lru_cache(maxsize=None)
    def pair_results(self):
        """[(intersection, expected, probability)] of self.pairs from the model"""
        e = self.estimator()
        return [e.intersection_prob(a, b) for a, b in self.pairs]

    # -- decisions --
    def universe(self):
        return wm.Universe(self.barcodes, self.n_genes, self.total_umis)

    def neighbours(self, kind, base):
        """(neighbours, levels) for get_best_merge_target, or None where get_merge_target answers without it"""
        if kind == MERGE_POISSON_REAL:
            s = wm.search(wm.CONST, self.parts, True, self.min_genes, self.universe(), base)
            if not s.candidates:
                return None
            pieces = wm.split_barcode(wm.CONST, self.parts, self.barcodes[base])
            level = lambda c: sum(wm.edit_distance(x, y) for x, y in zip(pieces, wm.split_barcode(wm.CONST, self.parts, self.barcodes[c])))
            return s.candidates, [level(c) for c in s.candidates]
        found = smm.poisson_simple_neighbours(self, base, self.max_ed)
        return (found, [0] * len(found)) if found else None               # an unordered_map's order: not known

    @lru_cache(maxsize=None)
    def decisions(self, kind, thresholds):
        """{base: Decision} over the filtered cells; `no neighbours` is a Decision of margin 1"""
        out = {}
        for base in self.filtered:
            nb = self.neighbours(kind, base)
            if nb is None:
                out[base] = pm.Decision(-1 if kind == MERGE_POISSON_REAL else base, pm.Decimal(1), None, [])
                continue
            d = pm.best_target(self.estimator(), base, nb[0], thresholds[0], thresholds[1], nb[1])
            if kind == MERGE_POISSON_SIMPLE and d.target == -1:
                d.target = base
            out[base] = d
        return out


class Builder:
    def __init__(self, seed, umi_len):
        self.rng, self.umi_len, self.mol = random.Random(seed), umi_len, set()

    def umis(self, n, lo=0, hi=None):
        """n distinct UMI numbers of [lo, hi)"""
        return self.rng.sample(range(lo, 4 ** self.umi_len if hi is None else hi), n)

    def add(self, cell, gene, umis):
        self.mol.update((cell, gene, u) for u in umis)


def barcodes_plain(n, length=10):
    return [text_of(i * 7919 + 13, length) for i in range(n)]


def frequency_case(name, n_freq, copies, n_cells, n_genes, n_singletons, seed, umi_len=8):
    """`copies` UMIs for each frequency 1 .. n_freq: a UMI of frequency f lies in f groups (gene-major, so that it is shared by
    neighbouring cells of one gene), plus a tail of singletons that keeps the genes small against the UMI space.  Every cell is
    filtered; the classes are the n_freq frequencies."""
    b = Builder(seed, umi_len)
    groups = [(c, g) for g in range(n_genes) for c in range(n_cells)]
    assert n_freq <= len(groups)
    codes = iter(b.umis(n_freq * copies + n_singletons))
    for f in range(1, n_freq + 1):
        for _ in range(copies):
            u, start = next(codes), b.rng.randrange(len(groups))
            for i in range(f):
                c, g = groups[(start + i) % len(groups)]
                b.add(c, g, [u])
    for _ in range(n_singletons):
        c, g = b.rng.choice(groups)
        b.add(c, g, [next(codes)])
    cells = list(range(n_cells))
    pairs = [(cells[i], cells[(i + 1) % n_cells]) for i in range(0, n_cells, max(1, n_cells // 12))][:12]
    pairs += [(y, x) for x, y in pairs[:3]] + [(0, n_cells // 2)]
    return ContainerCase(name, barcodes_plain(n_cells), b.mol, umi_len, 1, pairs)


def distribution_case(name, adjuster_name, n_cells, n_genes, seed):
    """The counts of an adjuster case as a container: UMI number i lies in counts[i] groups, so the filtered cells' distribution is
    that case's and the class kernel builds its table from it."""
    counts = _ADJUSTER[adjuster_name]().counts
    umi_len = max(8, (len(counts) - 1).bit_length() // 2 + 1)
    b = Builder(seed, umi_len)
    groups = [(c, g) for g in range(n_genes) for c in range(n_cells)]
    for u, k in enumerate(counts):
        for c, g in b.rng.sample(groups, k):
            b.add(c, g, [u])
    pairs = [(i, (i + 1) % n_cells) for i in range(0, n_cells, max(1, n_cells // 8))][:8]
    c = ContainerCase(name, barcodes_plain(n_cells), b.mol, umi_len, 1, pairs)
    assert sorted(c.estimator().distribution.values()) == sorted(counts)
    return c


def pair_edges_case():
    """The merge join of common_genes_kernel and the key lookup at their edges.  min_genes = 2; cells:
      0, 1   no gene in common (genes 1-10 / 11-20)
      2, 3   gene 0 only in 2 (the first gene id), the last gene only in 3, one gene (21) in common
      4, 5   300 genes in common with 300 different size pairs, both orders of the sizes; 5 also has the largest gene-less group
      6, 7   40 genes in common, every one of sizes (2, 3): one key
      8      one gene: not filtered, and that gene is the largest of the container (the table's length); shared with 4
    """
    b = Builder(21, 8)
    pool = 6000                                                             # UMIs come from the first 6000 numbers: chance intersections
    for g in range(1, 11):
        b.add(0, g, b.umis(b.rng.randint(1, 9), hi=pool))
        b.add(1, g + 10, b.umis(b.rng.randint(1, 9), hi=pool))
    b.add(2, 0, b.umis(5, hi=pool))
    shared = b.umis(12, hi=pool)
    b.add(2, 21, shared[:9]); b.add(3, 21, shared[4:])
    for k in range(300):                                                    # genes 22 .. 321: sizes (1 + k % 20, 22 + k // 20) and swapped
        g, s1, s2 = 22 + k, 1 + k % 20, 22 + k // 20
        if k % 2:
            s1, s2 = s2, s1
        u = b.umis(s1 + s2, hi=pool)
        b.add(4, g, u[:s1]); b.add(5, g, u[s1 - 1:-1] if k % 3 == 0 else u[s1:])       # every third gene: one UMI in both cells
    for k in range(40):                                                     # genes 322 .. 361
        u = b.umis(4, hi=pool)
        b.add(6, 322 + k, u[:2]); b.add(7, 322 + k, u[1:])
    big = b.umis(700)
    b.add(8, 362, big); b.add(4, 362, big[:30] + b.umis(10, hi=pool))
    b.add(3, 363, b.umis(3, hi=pool))                                       # the last gene id
    b.add(5, None, b.umis(900)); b.add(4, None, b.umis(50)); b.add(0, None, b.umis(4))
    pairs = [(0, 1), (1, 0), (2, 3), (3, 2), (4, 5), (5, 4), (6, 7), (7, 6), (4, 8), (8, 4), (2, 4), (5, 8), (0, 4), (3, 5), (6, 4)]
    c = ContainerCase("pair_edges", barcodes_plain(9), b.mol, 8, 2, pairs)
    assert 8 not in c.filtered and len(c.filtered) == 8
    e = c.estimator()
    assert e.max_size == 700 and max(len(u) for cell in c.filtered for u in c.container[cell].values()) < 700
    assert e.common_genes(0, 1) == [] and e.common_genes(2, 3) == [21] and len(e.common_genes(4, 5)) == 300
    keys = {tuple(sorted((e.adjusted(len(c.container[4][g])), e.adjusted(len(c.container[5][g]))))) for g in e.common_genes(4, 5)}
    assert len(keys) > 256
    assert len({(len(c.container[6][g]), len(c.container[7][g])) for g in e.common_genes(6, 7)}) == 1
    sizes = [(len(c.container[4][g]), len(c.container[5][g])) for g in e.common_genes(4, 5)]
    assert any(a > b_ for a, b_ in sizes) and any(a < b_ for a, b_ in sizes)
    return c


TAIL_OVERLAPS = (1, 2, 3)


def tail_case():
    """The Poisson tail's regimes through real pairs (every cell filtered, UMIs of 10 bases):
      0, 1    many large genes from a small pool, one UMI in common: intersection 1 against a large expectation
      2, 3    one gene, 80 UMIs in common, a tiny expectation: far below 1e-100
      4, 5    the same with 500 UMIs: below the smallest double
      6.. 11  three pairs whose intersections (TAIL_OVERLAPS) lie within 1 of their expectation, on both sides of the tail's
              switch between series and continued fraction (lambda < k + 1)
    The other UMIs come from 60 000 numbers, so that the distribution is wide."""
    b = Builder(31, 10)
    wide = 4 ** 10
    for g in range(8):                                                     # pool of 300 numbers, halves kept apart
        b.add(0, g, b.umis(100, 0, 150)); b.add(1, g, b.umis(100, 150, 300))
    b.add(1, 0, [next(iter(u for c, g, u in b.mol if c == 0 and g == 0))])
    same = b.umis(80, 1000, wide)
    b.add(2, 8, same); b.add(3, 8, same)
    same = b.umis(500, 1000, wide)
    b.add(4, 9, same); b.add(5, 9, same)
    for k, overlap in enumerate(TAIL_OVERLAPS):                            # 4 genes of 60 x 60 from 700 numbers: the same expectation
        for g in range(10, 14):
            u = b.umis(120, 300, 1000)
            b.add(6 + 2 * k, g, u[:60])
            b.add(7 + 2 * k, g, u[60 - overlap:120 - overlap] if g == 10 else u[60:])
    heavy = b.umis(30, 61000, 62000)                                       # 30 UMIs in every group of the background: SUM p^2 is large
    for c in range(12, 40):                                                # the wide background
        for g in range(14, 20):
            b.add(c, g, b.umis(350, 1000, 61000) + heavy)
    pairs = [(0, 1), (1, 0), (2, 3), (4, 5), (5, 4), (6, 7), (8, 9), (10, 11), (11, 10), (12, 13)]
    return ContainerCase("tail_regimes", barcodes_plain(40), b.mol, 10, 1, pairs)


def _container_of(self, cell, gene):
    return {u for c, g, u in self.mol if c == cell and g == gene}


Builder.container_of = _container_of


# ---- decision cases: a whitelist of a few dozen barcodes ---------------------------------------------------------------------
PARTS = [["AAAAA", "CCCCC", "GGGGG", "TTTTT", "ACACA", "GTGTG"], ["AACCG", "CCGGT", "CGGGA", "TTAAC", "AGAGA", "AGTCA", "CTCTC", "GACTC"]]
LOOSE, STRICT = (0.5, 0.5), (1e-4, 1e-7)
DECISION_BARCODES = {                                   # R: on the whitelist; B: one substitution beside it
    "R0": "AAAAA" + "AACCG", "R1": "CCCCC" + "CCGGT", "R2": "CCCCC" + "CGGGA", "R3": "ACACA" + "AGTCA", "R4": "ACACA" + "AGAGA",
    "R5": "GTGTG" + "CTCTC", "R6": "GTGTG" + "GACTC",
    "B0": "AAAAA" + "AAGCG", "B1": "CCCCC" + "CAGGT", "B2": "AAAAA" + "AACCT", "B4": "GTGTG" + "ATCTC", "B5": "CCCCC" + "CCGGA",
}


def sub(barcode, places):
    """a substitution at each of `places` (A <-> T, C <-> G)"""
    t = list(barcode)
    for i in places:
        t[i] = {"A": "T", "T": "A", "C": "G", "G": "C"}[t[i]]
    return "".join(t)


def decisions_case():
    """min_genes = 2.
      R0 <- B0       one neighbour at distance 1; B0 holds a third of R0's molecules: merges under both pairs of thresholds
      R1, R2 <- B1   distance 1 from R1 and 2 from R2 (two substitutions from R1); it holds a quarter of R1's molecules, none of R2's
      B2             beside R0, nothing in common with anybody: probability 1, no target
      R3 -> R4       R3 is a real barcode two substitutions from R4 with two of R4's molecules beside 60 of its own: max_merge_prob
                     applies to it
      R5, R6 <- B4   R5 (distance 1) and R6 (distance 2) are the same cell molecule for molecule and B4 holds a fifth of it: two
                     exactly equal probabilities, R5 comes first in the reference's order
      B5             beside R1 and R2 with two of R1's molecules beside 30 of its own: accepted only under loose thresholds"""
    b = Builder(41, 8)
    names = list(DECISION_BARCODES)
    n = {x: i for i, x in enumerate(names)}

    def fill(c, genes, lo, hi):
        for g in genes:
            b.add(n[c], g, b.umis(b.rng.randint(lo, hi)))

    def of(c):
        return sorted(m for m in b.mol if m[0] == n[c])

    def copy(src, dst, picked):
        b.mol.update((n[dst], g, u) for _, g, u in picked)

    fill("R0", range(0, 30), 4, 12); fill("R1", range(5, 35), 4, 12); fill("R2", range(10, 40), 4, 12)
    fill("R4", range(0, 25), 4, 10); fill("R5", range(20, 40), 3, 8)
    copy("R5", "R6", of("R5"))
    fill("R3", range(25, 37), 5, 5); copy("R4", "R3", of("R4")[:2])
    copy("R0", "B0", of("R0")[::3]); copy("R1", "B1", of("R1")[::4]); copy("R5", "B4", of("R5")[::5])
    fill("B2", range(40, 44), 2, 4)
    fill("B5", range(44, 54), 2, 4); copy("R1", "B5", of("R1")[:2])
    pairs = [("B0", "R0"), ("B4", "R5"), ("B4", "R6"), ("R3", "R4"), ("B1", "R1"), ("B1", "R2"), ("B5", "R1"), ("B2", "R0"), ("R5", "R6")]
    c = ContainerCase("decisions", [DECISION_BARCODES[x] for x in names], b.mol, 8, 2, [(n[x], n[y]) for x, y in pairs],
                      parts=PARTS, thresholds=[STRICT, LOOSE], max_ed=1)
    c.names = n
    return c


def random_case(seed):
    """A small random container beside a 36-barcode whitelist: <= 40 cells, <= 60 genes, UMIs of 5 to 8 bases, <= 30 000 reads."""
    rng = random.Random(1000 + seed)
    umi_len = 5 + seed % 4
    b = Builder(2000 + seed, umi_len)
    n_genes = rng.randint(30, 60)
    combos = [x + y for x in PARTS[0] for y in PARTS[1]]
    real = rng.sample(combos, rng.randint(6, 12))
    barcodes = list(real)
    pool = min(4 ** umi_len, 20000)
    for c in range(len(real)):
        for g in rng.sample(range(n_genes), rng.randint(n_genes // 2, n_genes)):
            b.add(c, g, b.umis(rng.randint(1, 10), hi=pool))
    while len(barcodes) < rng.randint(25, 40):
        src = rng.randrange(len(real))
        t = sub(real[src], rng.sample(range(10), rng.randint(1, 2)))
        if t in barcodes:
            continue
        barcodes.append(t)
        c = len(barcodes) - 1
        share = rng.choice((0.0, 0.02, 0.1, 0.4))
        for _, g, u in sorted(m for m in b.mol if m[0] == src):
            if rng.random() < share:
                b.add(c, g, [u])
        for g in rng.sample(range(n_genes), rng.randint(1, 8)):
            b.add(c, g, b.umis(rng.randint(1, 4), hi=pool))
    used = sorted({g for _, g, _ in b.mol})
    relabel = {g: i for i, g in enumerate(used)}
    mol = {(c, relabel[g], u) for c, g, u in b.mol}
    cells = list(range(len(barcodes)))
    pairs = [(c, rng.randrange(len(real))) for c in rng.sample(cells[len(real):], min(12, len(cells) - len(real)))]
    return ContainerCase("random_%d" % seed, barcodes, mol, umi_len, 2, [p for p in pairs if p[0] != p[1]], parts=PARTS,
                         thresholds=[STRICT, LOOSE], max_ed=2, hand_built=False)


_CONTAINER = {
    "classes_1": partial(frequency_case, "classes_1", 1, 3000, 6, 10, 0, 51),
    "classes_2": partial(frequency_case, "classes_2", 2, 40, 6, 10, 2000, 52),
    "classes_63": partial(frequency_case, "classes_63", 63, 1, 12, 20, 3000, 53),
    "classes_64": partial(frequency_case, "classes_64", 64, 1, 12, 20, 3000, 54),
    "classes_65": partial(frequency_case, "classes_65", 65, 1, 12, 20, 3000, 55),
    "classes_255": partial(frequency_case, "classes_255", 255, 1, 24, 40, 12000, 56),
    "classes_256": partial(frequency_case, "classes_256", 256, 1, 24, 40, 12000, 57),
    "classes_257": partial(frequency_case, "classes_257", 257, 1, 24, 40, 12000, 58),
    "classes_513": partial(frequency_case, "classes_513", 513, 1, 40, 65, 30000, 59),
    "multiplicity_thousands": partial(frequency_case, "multiplicity_thousands", 5, 3000, 10, 30, 0, 60),
    "dist_64_skewed": partial(distribution_case, "dist_64_skewed", "adj_64_skewed_random", 8, 6, 61),
    "dist_65_uniform": partial(distribution_case, "dist_65_uniform", "adj_65_uniform_descending", 8, 6, 62),
    "dist_257_skewed": partial(distribution_case, "dist_257_skewed", "adj_257_skewed_random", 8, 8, 63),
    "dist_65537_uniform": partial(distribution_case, "dist_65537_uniform", "adj_65537_uniform_random", 40, 50, 64),
    "pair_edges": pair_edges_case,
    "tail_regimes": tail_case,
    "decisions": decisions_case,
}
RANDOM_SEEDS = list(range(12))
for _seed in RANDOM_SEEDS:
    _CONTAINER["random_%d" % _seed] = partial(random_case, _seed)
CONTAINER_NAMES = sorted(_CONTAINER)
CLASS_COUNTS = {"classes_%d" % n: n for n in (1, 2, 63, 64, 65, 255, 256, 257, 513)}
CLASS_COUNTS["multiplicity_thousands"] = 5
DECISION_NAMES = ["decisions"] + ["random_%d" % s for s in RANDOM_SEEDS]

_built = {}


def adjuster_case(name):
    if ("a", name) not in _built:
        _built["a", name] = _ADJUSTER[name]()
    return _built["a", name]


def case(name):
    """the container case of that name, built once per process (its model results are cached on it)"""
    if name not in _built:
        _built[name] = _CONTAINER[name]()
        assert _built[name].name == name
    return _built[name]


# ---- the oracle beside the model: the scale D of a case ---------------------------------------------------------------------
ULP = 2.0 ** -52


def write_whitelist(c, directory):
    path = directory / (c.name + "_whitelist")
    path.write_text(wm.whitelist_text(c.parts))
    return str(path)


def oracle_of(c, kind=MERGE_POISSON_SIMPLE, thresholds=STRICT, whitelist=""):
    """the case in the oracle, initialised, with its estimator ready (not merged)"""
    from oracle import Oracle
    o = Oracle(merge_kind=kind, barcodes_kind=wm.CONST, barcodes_file=whitelist, min_genes_before=c.min_genes, min_genes_after=c.min_genes,
               max_cb_merge_ed=c.max_ed, max_merge_prob=thresholds[0], max_real_merge_prob=thresholds[1])
    o.add_packed(*c.arrays())
    o.set_initialized()
    o.poisson_init()
    return o


def oracle_scale(c, o):
    """(D of `expected`, D of the probability): the largest relative deviation of the oracle -- the reference's formulas in double,
    summed left to right -- from the exact model over the case's pairs with a non-empty intersection, each at least one ulp"""
    d_expected = d_prob = pm.Decimal(ULP)
    for (a, b), (n, expected, prob) in zip(c.pairs, c.pair_results()):
        if n:
            d_expected = max(d_expected, pm.relative_deviation(o.poisson_expected_intersection(a, b), expected))
            d_prob = max(d_prob, pm.relative_deviation(o.poisson_intersection_prob(a, b), prob))
    return d_expected, d_prob


def threshold_of(d_prob):
    """T: a base whose decision margin lies under it is not compared"""
    return max(100 * d_prob, pm.Decimal("1e-10"))
