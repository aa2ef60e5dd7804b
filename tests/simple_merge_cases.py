"""The inputs of the whitelist-free merge tests (test_simple_merge_model_cpu.py runs them through simple_merge_model.py and the oracle,
test_gpu_simple_merge.py through the device): hand-built containers, each at the smallest size at which the code it is named for can
still go wrong, and a dozen random ones for agreement in bulk.

A case is a poisson_cases.ContainerCase with the runs it is made for: Run(kind, max_ed, min_fraction), kind = "simple" (-m without a
whitelist), "poisson" (-M without a whitelist, loose thresholds) or "all" (merge_type = all).  What a case claims is said in the
docstring of its builder and asserted there from the model, or in test_simple_merge_model_cpu.py.  order_dependent = {run index:
{base: the set of targets}} names the bases whose answer hangs on the iteration order of the reference's unordered containers; every
other base of a hand-built case is decided.

The pair table of the device is the list of (UMI-gene, cell) records of the filtered cells sorted by (gene, UMI, cell) and cut into
tiles of 256 records (simple_merge.h); table_records() is that list, for the claims about where a run of equal UMI-genes lies.
"""
import random
from collections import namedtuple
from fractions import Fraction
from functools import partial

import numpy as np

import poisson_cases as pc
import simple_merge_model as smm
import whitelist_model as wm

Run = namedtuple("Run", "kind max_ed min_fraction")
ESCAPE = 1 << 63                                          # a barcode that is no clean code of at most 31 bases: index into the side strings
TILE = 256
NOT_ON_DEVICE = 0xFFFFFFFF                                # dropest_simple_merge_pairs: the host computes this distance


class MergeCase(pc.ContainerCase):
    def __init__(self, name, barcodes, molecules, umi_len, min_genes, runs, hand_built=True, order_dependent=None):
        super().__init__(name, barcodes, molecules, umi_len, min_genes, [], thresholds=[pc.LOOSE], max_ed=runs[0].max_ed, hand_built=hand_built)
        assert all(r.max_ed == self.max_ed for r in runs if r.kind == "poisson")     # (the -M model reads the case's max_ed)
        self.runs, self.order_dependent = list(runs), dict(order_dependent or {})
        self.side = [b for b in self.barcodes if not self.clean(b)]
        self._answers = {}

    @staticmethod
    def clean(barcode):
        return len(barcode) <= 31 and set(barcode) <= set(pc.ACGT)

    def on_device(self, a, b):
        return self.clean(self.barcodes[a]) and self.clean(self.barcodes[b])

    def arrays(self):
        code = [pc.pack(b) if self.clean(b) else ESCAPE | self.side.index(b) for b in self.barcodes]
        sentinel = 1 << (2 * self.umi_len)
        n_cells = len(self.barcodes)
        cb = code + [code[c] for c, _, _ in self.molecules]
        umi = [sentinel] * n_cells + [sentinel | u for _, _, u in self.molecules]
        gene = [pc.NO_GENE] * n_cells + [pc.NO_GENE if g is None else g for _, g, _ in self.molecules]
        return (np.array(cb, np.uint64), np.array(umi, np.uint64), np.array(gene, np.uint32), np.full(len(cb), 2 << 16, np.uint32))

    def answers(self, i):
        """{base: simple_merge_model.Answer} of run i ("simple" and "all" runs) over the filtered cells"""
        if i not in self._answers:
            run = self.runs[i]
            if run.kind == "simple":
                self._answers[i] = {b: smm.simple_target(self, b, run.max_ed, run.min_fraction) for b in self.filtered}
            else:
                assert run.kind == "all"
                self._answers[i] = {b: smm.Answer({smm.merge_all_target(self, b, run.max_ed)}, None) for b in self.filtered}
        return self._answers[i]

    def undecided(self, i):
        return sorted(b for b, a in self.answers(i).items() if not a.decided)

    def table_records(self):
        return sorted((g, u, c) for c in self.filtered for g, umis in self.container[c].items() for u in umis)

    def run_of(self, gene, umi):
        """(first record, number of records) of a UMI-gene in the sorted table"""
        at = [i for i, (g, u, _) in enumerate(self.table_records()) if (g, u) == (gene, umi)]
        assert at == list(range(at[0], at[0] + len(at)))
        return at[0], len(at)


SIMPLE = Run("simple", 2, 0.2)


class Mol:
    """molecules under construction; private() pads a cell with genes nobody shares (gene ids `first` ..), so that its gene count is
    what the case wants"""

    def __init__(self, umi_len):
        self.umi_len, self.mol = umi_len, set()

    def add(self, cell, gene, umis):
        self.mol.update((cell, gene, u) for u in umis)

    def private(self, cell, first, n_genes, n_cells):
        own = 4 ** self.umi_len - n_cells + cell                               # a UMI number that only this cell uses
        for g in range(first, first + n_genes):
            self.add(cell, g, [own])


def far_barcodes(n, length, seed, min_distance=None):
    """n random barcodes; with min_distance, every two of them are at least that far apart"""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        b = "".join(rng.choice(pc.ACGT) for _ in range(length))
        if b in out or (min_distance and any(wm.edit_distance(b, x) < min_distance for x in out)):
            continue
        out.append(b)
    return out


def all_barcodes(n, length):
    assert n <= 4 ** length
    return [pc.text_of(i * 389 % 4 ** length, length) for i in range(n)]     # (389 is odd: a permutation of the codes)


# ---- the pair table -----------------------------------------------------------------------------------------------------------
def pair_runs_case(name="pair_runs", front=0):
    """min_genes = 2.  Cells (ids after `front` barcodes of one read each, which are not filtered):
      0, 1   two genes each; (gene 0, UMI 0) is held by 0 alone: a run of 1, no pair; (gene 0, UMI 1) by both: a run of 2, and as their gene
             counts are equal both ordered pairs exist
      2, 3   2 and 3 genes, (gene 0, UMI 2) in common: the pair (base 2, other 3) exists, (base 3, other 2) does not
      4      one gene: not filtered; it holds every UMI-gene of cell 0 and appears neither as base nor as other
      5, 6   two genes each; all they share are three gene-less molecules: no pair
    With front = 5000 the filtered cells have ids beyond 2^12."""
    n = front + 7
    m = Mol(8)
    c = [front + i for i in range(7)]
    m.add(c[0], 0, [0, 1]); m.add(c[1], 0, [1])
    m.private(c[0], 1, 1, n); m.private(c[1], 1, 1, n)
    m.add(c[4], 0, [0, 1])
    m.add(c[2], 0, [2]); m.add(c[3], 0, [2])
    m.private(c[2], 1, 1, n); m.private(c[3], 1, 2, n)
    m.private(c[5], 1, 2, n); m.private(c[6], 1, 2, n)
    m.add(c[5], None, [7, 8, 9]); m.add(c[6], None, [7, 8, 9])
    barcodes = pc.barcodes_plain(front, 12) + far_barcodes(7, 12, 3, 4)
    assert len(set(barcodes)) == n
    case = MergeCase(name, barcodes, m.mol, 8, 2, [SIMPLE, Run("poisson", 2, 0)])
    assert sorted(case.filtered) == [c[i] for i in (0, 1, 2, 3, 5, 6)]
    assert case.run_of(0, 0)[1] == 1 and case.run_of(0, 1)[1] == 2
    assert smm.common_umigs(case, c[0]) == {c[1]: 1} and smm.common_umigs(case, c[1]) == {c[0]: 1}
    assert smm.common_umigs(case, c[2]) == {c[3]: 1} and smm.common_umigs(case, c[3]) == {}
    assert smm.common_umigs(case, c[5]) == {} and smm.common_umigs(case, c[6]) == {}
    assert all(c[4] not in smm.common_umigs(case, b) for b in case.filtered)
    assert front == 0 or min(case.filtered) >= 1 << 12
    return case


def hot_600_case():
    """600 filtered cells of 1, 2 or 3 genes that all hold (gene 0, UMI 0): one run of 600 records, 600 x 599 ordered pairs before the size
    rule.  Barcodes of 5 bases and max_ed = 1: nobody is admissible, every target is the cell itself."""
    n = 600
    m = Mol(8)
    for c in range(n):
        m.add(c, 0, [0])
        m.private(c, 1, c % 3, n)
    case = MergeCase("hot_600", all_barcodes(n, 5), m.mol, 8, 1, [Run("simple", 1, 0.2)])
    assert len(case.filtered) == n and case.run_of(0, 0) == (0, n)
    assert sum(len(smm.common_umigs(case, b)) for b in (0, 1, 2)) == (n - 1) + (2 * n // 3 - 1) + (n // 3 - 1)
    return case


def tiles_case():
    """300 filtered cells.  Gene 0: UMIs 0 .. 199 are held by one cell each (records 0 .. 199 of the sorted table), UMI 200 by all 300
    cells (records 200 .. 499: the run crosses the tile boundary at 256) and UMI 201 by all 300 again (records 500 .. 799: it crosses
    512 and 768).  Every second cell has a second gene.  Every pair that exists shares 2."""
    n = 300
    m = Mol(8)
    for u in range(200):
        m.add((u * 7) % n, 0, [u])
    for c in range(n):
        m.add(c, 0, [200, 201])
        m.private(c, 1, c % 2, n)
    case = MergeCase("tiles", all_barcodes(n, 5), m.mol, 8, 1, [Run("simple", 1, 0.2)])
    assert len(case.filtered) == n
    assert case.run_of(0, 200) == (200, 300) and case.run_of(0, 201) == (500, 300)
    assert set(smm.common_umigs(case, 0).values()) == {2} and len(smm.common_umigs(case, 0)) == n - 1
    assert len(smm.common_umigs(case, 1)) == n // 2 - 1
    return case


def run_end_case(end):
    """A run of two records that ends exactly at record `end` of the sorted table (255: the last of a tile, 256: across the boundary, 257),
    behind end - 1 records of UMI-genes held by one cell; a second run of two follows it at once."""
    n = 4
    m = Mol(8)
    for u in range(end - 1):
        m.add(u % n, 0, [u])
    m.add(0, 0, [end + 10]); m.add(1, 0, [end + 10])
    m.add(2, 0, [end + 11]); m.add(3, 0, [end + 11])
    case = MergeCase("run_end_%d" % end, far_barcodes(n, 10, 5, 4), m.mol, 8, 1, [SIMPLE])
    assert case.run_of(0, end + 10) == (end - 1, 2) and case.run_of(0, end + 11) == (end + 1, 2)
    assert smm.common_umigs(case, 0) == {1: 1} and smm.common_umigs(case, 3) == {2: 1}
    return case


SHARED_COUNTS = (1, 255, 256, 257, 70000)


def shared_counts_case():
    """Five pairs of cells (2k, 2k + 1) that share 1, 255, 256, 257 and 70 000 UMI-genes of gene k; their barcodes are one substitution
    apart and their sizes equal, so each merges into the other: fraction 1."""
    m = Mol(9)
    centres = far_barcodes(len(SHARED_COUNTS), 12, 7, 5)
    barcodes = []
    for k, count in enumerate(SHARED_COUNTS):
        m.add(2 * k, k, range(count)); m.add(2 * k + 1, k, range(count))
        barcodes += [centres[k], pc.sub(centres[k], [3])]
    case = MergeCase("shared_counts", barcodes, m.mol, 9, 1, [SIMPLE])
    for k, count in enumerate(SHARED_COUNTS):
        assert smm.common_umigs(case, 2 * k) == {2 * k + 1: count} and smm.common_umigs(case, 2 * k + 1) == {2 * k: count}
        assert case.answers(0)[2 * k].targets == {2 * k + 1}
    return case


KEY_WIDTHS = {62: 40, 63: 70, 64: 130}                     # UMI + gene + cell field -> number of cells
# What the library does with these widths (a width it refuses must raise UnsupportedError, not answer): one context sorts records of 64
# bits and answers all three; a sharded run needs the shard beside the cell in 63 bits and refuses all three.
KEY_WIDTH_REFUSED = {"one context": (), "shards": (62, 63, 64)}


def key_width_case(width):
    """UMIs of 26 bases (52 bits), 10 genes (4 bits) and 40, 70 or 130 cells (6, 7, 8 bits): a record of 62, 63 or 64 bits.  The first cells
    come in pairs one substitution apart that share most of their UMIs, one of them with the highest bit of the UMI field set."""
    n = KEY_WIDTHS[width]
    rng = random.Random(width)
    m = Mol(26)
    centres = far_barcodes(n // 2, 14, width, 4)
    barcodes = []
    for k in range(n // 2):
        barcodes += [centres[k], pc.sub(centres[k], [k % 14])]
        genes = rng.sample(range(10), 3)
        for g in genes:
            shared = rng.sample(range(4 ** 26), 6) + ([4 ** 26 - 1 - k] if g == genes[0] else [])
            m.add(2 * k, g, shared); m.add(2 * k + 1, g, shared[:4] + rng.sample(range(4 ** 26), 5))
    case = MergeCase("key_width_%d" % width, barcodes, m.mol, 26, 1, [SIMPLE])
    assert len(case.barcodes) == n and (n - 1).bit_length() + 4 + 52 == width and len({g for _, g, _ in case.molecules}) == 10
    return case


# ---- the barcode distance -----------------------------------------------------------------------------------------------------
DISTANCE_MAX_EDS = (1, 2, 3, 7)


def _at_distance(rng, barcode, d, style):
    """a barcode at Levenshtein distance d: by d substitutions, or by a deletion in front and an insertion behind (2) and d - 2
    substitutions; at distance 1 the other style is one insertion"""
    if style == "sub":
        other = pc.sub(barcode, rng.sample(range(len(barcode)), d))
    elif d == 1:
        at = rng.randrange(1, len(barcode))
        other = barcode[:at] + {"A": "C", "C": "A", "G": "T", "T": "G"}[barcode[at]] + barcode[at:]
    else:
        other = pc.sub(barcode, rng.sample(range(4, len(barcode) - 4), d - 2))[1:] + {"A": "C", "C": "A", "G": "T", "T": "G"}[barcode[-1]]
    return other


def distance_case(max_ed):
    """For each distance d of max_ed - 1, max_ed, max_ed + 1 (d >= 1) and both ways of making it, a pair (base, other): the base holds 10
    UMIs of a gene of its own, the other the same 10, 10 more and a second gene.  The other is the base's only candidate and the base is
    none of the other's.  Simple (distance < max_ed) merges d = max_ed - 1 alone, PoissonSimple (<=) also d = max_ed."""
    rng = random.Random(40 + max_ed)
    m = Mol(8)
    specs = [(d, style) for d in (max_ed - 1, max_ed, max_ed + 1) if d >= 1 for style in ("sub", "indel")]
    centres = far_barcodes(len(specs), 24, 50 + max_ed, 9)
    barcodes, pairs = [], []
    for k, (d, style) in enumerate(specs):
        for _ in range(100):
            other = _at_distance(rng, centres[k], d, style)
            if wm.edit_distance(centres[k], other) == d:
                break
        else:
            raise AssertionError("no barcode at distance %d" % d)
        barcodes += [centres[k], other]
        umis = rng.sample(range(60000), 20)
        m.add(2 * k, 2 * k, umis[:10]); m.add(2 * k + 1, 2 * k, umis); m.add(2 * k + 1, 2 * k + 1, rng.sample(range(60000), 3))
        pairs.append((2 * k, 2 * k + 1, d, style))
    case = MergeCase("distance_ed%d" % max_ed, barcodes, m.mol, 8, 1, [Run("simple", max_ed, 0.2), Run("poisson", max_ed, 0)])
    case.distance_pairs = pairs
    for base, other, d, _ in pairs:
        assert smm.common_umigs(case, base) == {other: 10} and smm.common_umigs(case, other) == {}
        assert case.answers(0)[base].targets == {other if d < max_ed else base}
        assert smm.poisson_simple_neighbours(case, base, max_ed) == ([other] if d <= max_ed else [])
    assert {d for _, _, d, _ in pairs} >= {max_ed, max_ed + 1}
    return case


def lengths_case():
    """Barcodes of 8 to 19 bases in one container: for every length L < 19 a pair (L, L + 1) one insertion apart, and for L < 18 a pair
    (L, L + 2) two insertions apart; bases and others as in the distance cases.  max_ed = 2: Simple merges the first kind, PoissonSimple both."""
    rng = random.Random(61)
    m = Mol(8)
    barcodes, pairs = [], []
    for length in range(8, 19):
        for extra in (1, 2) if length < 18 else (1,):
            for _ in range(100):
                base = "".join(rng.choice(pc.ACGT) for _ in range(length))
                other = base
                for _ in range(extra):
                    at = rng.randrange(len(other) + 1)
                    other = other[:at] + rng.choice(pc.ACGT) + other[at:]
                if wm.edit_distance(base, other) == extra and all(wm.edit_distance(x, y) > 3 for x in (base, other) for y in barcodes):
                    break
            else:
                raise AssertionError("no pair of lengths %d, %d" % (length, length + extra))
            k = len(barcodes) // 2
            barcodes += [base, other]
            umis = rng.sample(range(60000), 20)
            m.add(2 * k, 2 * k, umis[:10]); m.add(2 * k + 1, 2 * k, umis); m.add(2 * k + 1, 2 * k + 1, rng.sample(range(60000), 3))
            pairs.append((2 * k, 2 * k + 1, extra, "insert"))
    case = MergeCase("barcode_lengths", barcodes, m.mol, 8, 1, [Run("simple", 2, 0.2), Run("poisson", 2, 0)])
    case.distance_pairs = pairs
    assert {len(b) for b in barcodes} == set(range(8, 20))
    for base, other, d, _ in pairs:
        assert case.answers(0)[base].targets == {other if d < 2 else base}
    return case


def long_case():
    """Pairs one substitution apart: two barcodes of 31 bases (the device's distance), 31 against 32 bases by one insertion and two of 33
    bases (escaped: the host's), and a barcode with an N against the same barcode with a base in its place -- distance 0, N matches
    anything -- and against one with another substitution (1).  max_ed = 2."""
    rng = random.Random(71)
    m = Mol(8)
    b31, b31b, b33, b12 = ("".join(rng.choice(pc.ACGT) for _ in range(n)) for n in (31, 31, 33, 12))
    with_n = b12[:5] + "N" + b12[6:]
    groups = [(b31, pc.sub(b31, [30])), (b31b, b31b[:16] + "A" + b31b[16:]), (b33, pc.sub(b33, [0])), (with_n, b12), (pc.sub(with_n, [9]), pc.sub(b12, [2]))]
    barcodes, pairs = [], []
    for k, (base, other) in enumerate(groups):
        barcodes += [base, other]
        umis = rng.sample(range(60000), 20)
        m.add(2 * k, 2 * k, umis[:10]); m.add(2 * k + 1, 2 * k, umis); m.add(2 * k + 1, 2 * k + 1, rng.sample(range(60000), 3))
        pairs.append((2 * k, 2 * k + 1, wm.edit_distance(base, other), "long"))
    case = MergeCase("barcode_long", barcodes, m.mol, 8, 1, [Run("simple", 2, 0.2), Run("poisson", 2, 0)])
    case.distance_pairs = pairs
    assert [d for _, _, d, _ in pairs] == [1, 1, 1, 0, 2]
    assert [case.on_device(a, b) for a, b, _, _ in pairs] == [True, False, False, False, False] and len(case.side) == 5
    return case


# ---- the decision -------------------------------------------------------------------------------------------------------------
def exact_fractions_case():
    """Fractions that are exact in binary.  Cells 0, 1: two UMIs each, one in common (1 is the larger: two genes): 0.5 * 1 * (1/2 + 1/2) = 0.5.
    Cells 2, 3: two and four UMIs, one in common: 0.5 * 1 * (1/2 + 1/4) = 0.375.  min_merge_fraction equal to the fraction merges
    (the reference asks `<`), 1e-6 above it does not."""
    m = Mol(8)
    m.add(0, 0, [1, 2]); m.add(1, 0, [1]); m.add(1, 1, [3])
    m.add(2, 2, [1, 2]); m.add(3, 2, [1, 5]); m.add(3, 3, [3, 4])
    c = far_barcodes(2, 12, 81, 5)
    runs = [Run("simple", 2, f) for f in (0.5, 0.5 + 1e-6, 0.375, 0.375 + 1e-6)]
    case = MergeCase("exact_fractions", [c[0], pc.sub(c[0], [2]), c[1], pc.sub(c[1], [7])], m.mol, 8, 1, runs)
    assert case.answers(0)[0].fractions == {1: Fraction(1, 2)} and case.answers(0)[2].fractions == {3: Fraction(3, 8)}
    want = [(1, 2), (0, 2), (1, 3), (1, 2)]
    assert [(case.answers(i)[0].target, case.answers(i)[2].target) for i in range(4)] == want
    return case


def eps_band_case(d):
    """A base of 2 000 UMIs (one gene) that shares 1 000 UMI-genes with X (10 000 UMIs, two genes) and 1 000 others with Y (10 000 + d UMIs,
    three genes); both are one substitution from it.  X's fraction is larger by 500 d / (10 000 (10 000 + d)), about 5e-6 d:
      d = 1   inside the EPS band: the larger gene count decides, Y
      d = 3   between EPS and 2 EPS: X in every order (decided); the library takes it for a near tie and must get X from its replay
      d = 5   more than 2 EPS: X, no replay"""
    m = Mol(8)
    m.add(0, 0, range(2000))
    m.add(1, 0, range(1000)); m.add(1, 0, range(2000, 2000 + 8999)); m.add(1, 1, [1])
    m.add(2, 0, range(1000, 2000)); m.add(2, 0, range(20000, 20000 + 8998 + d)); m.add(2, 1, [2]); m.add(2, 2, [3])
    b = far_barcodes(1, 12, 90 + d)[0]
    case = MergeCase("eps_band_%d" % d, [b, pc.sub(b, [3]), pc.sub(b, [8])], m.mol, 8, 1, [SIMPLE])
    assert [case.total_umis[c] for c in range(3)] == [2000, 10000, 10000 + d] and case.n_genes == [1, 2, 3]
    a = case.answers(0)[0]
    difference = a.fractions[1] - a.fractions[2]
    assert difference == Fraction(500 * d, 10000 * (10000 + d))
    assert {1: difference < smm.EPS, 3: smm.EPS < difference < 2 * smm.EPS, 5: difference > 2 * smm.EPS}[d]
    assert a.targets == {2 if d == 1 else 1}
    return case


def _tie_case(name, others, order_dependent=None):
    """base 0 of 400 UMIs in one gene; others: [(UMIs, genes)], each holds the base's first 200 UMIs and is one substitution from it"""
    m = Mol(8)
    m.add(0, 0, range(400))
    b = far_barcodes(1, 14, len(name))[0]
    barcodes = [b]
    for k, (umis, genes) in enumerate(others):
        c = k + 1
        m.add(c, 0, range(200)); m.add(c, 0, range(1000 + 12000 * k, 1000 + 12000 * k + umis - 200 - (genes - 1)))
        m.private(c, 1, genes - 1, len(others) + 1)
        barcodes.append(pc.sub(b, [2 * k + 1]))
    case = MergeCase(name, barcodes, m.mol, 8, 1, [SIMPLE], order_dependent=order_dependent)
    assert [(case.total_umis[k + 1], case.n_genes[k + 1]) for k in range(len(others))] == list(others)
    return case


def tie_unique_case():
    """Three candidates with exactly equal fractions (10 000 UMIs each) and 2, 4 and 3 genes: the one with 4, in every order."""
    case = _tie_case("tie_unique_genes", [(10000, 2), (10000, 4), (10000, 3)])
    a = case.answers(0)[0]
    assert len(set(a.fractions.values())) == 1 and a.targets == {2}
    return case


def tie_shared_case():
    """Exactly equal fractions and gene counts 3, 3 and 2: whichever of the two with 3 genes the reference meets first."""
    case = _tie_case("tie_shared_genes", [(10000, 3), (10000, 3), (10000, 2)], {0: {0: {1, 2}}})
    assert case.answers(0)[0].targets == {1, 2}
    return case


def tie_chain_case():
    """Fractions x, x + 0.7 EPS, x + 1.4 EPS (10 014, 10 007 and 10 000 UMIs, equal gene counts): the relation `within EPS` is not transitive.
    The largest wins when the smallest is met before it, else the middle one can stay: the middle one or the largest, never the smallest."""
    case = _tie_case("tie_chain", [(10014, 2), (10007, 2), (10000, 2)], {0: {0: {2, 3}}})
    a = case.answers(0)[0]
    f = a.fractions
    assert smm.EPS * 6 / 10 < f[2] - f[1] < smm.EPS * 8 / 10 and smm.EPS * 6 / 10 < f[3] - f[2] < smm.EPS * 8 / 10 and f[3] - f[1] > smm.EPS
    assert a.targets == {2, 3}
    return case


def tie_band_case():
    """Two candidates 0.7 EPS apart (10 000 UMIs and two genes, 10 007 UMIs and three genes): inside the band the larger gene count wins in
    either order, although its fraction is the smaller one.  Taking the largest fraction without the walk would answer the other."""
    case = _tie_case("tie_band_genes", [(10000, 2), (10007, 3)])
    a = case.answers(0)[0]
    assert smm.EPS / 2 < a.fractions[1] - a.fractions[2] < smm.EPS and a.targets == {2}
    return case


def hot_umig_case():
    """40 cells of one gene that all hold (gene 0, UMI 0) and two or three UMIs of their own: everybody is everybody's candidate with one
    UMI-gene in common.  Cells 0 and 1 are one substitution apart, all others far: 0 and 1 -- equal in size -- are each other's target."""
    n = 40
    m = Mol(8)
    for c in range(n):
        m.add(c, 0, [0] + [100 + 3 * c + j for j in range(1 + c % 2 + (c > 1))])
    barcodes = far_barcodes(n - 1, 12, 95, 4)
    barcodes.insert(1, pc.sub(barcodes[0], [4]))
    assert all(wm.edit_distance(barcodes[1], x) >= 2 for x in barcodes[2:])
    case = MergeCase("hot_umig", barcodes, m.mol, 8, 1, [SIMPLE])
    assert len(smm.common_umigs(case, 0)) == n - 1 and case.n_genes[0] == case.n_genes[1]
    assert case.answers(0)[0].targets == {1} and case.answers(0)[1].targets == {0}
    assert all(case.answers(0)[c].targets == {c} for c in range(2, n))
    return case


def nobody_admissible_case():
    """A base whose three candidates -- half of its UMIs each -- are all 2 or more edits away with max_ed = 2: its target is itself."""
    m = Mol(8)
    m.add(0, 0, range(10))
    b = far_barcodes(1, 12, 97)[0]
    barcodes = [b, pc.sub(b, [1, 6]), pc.sub(b, [2, 3, 9]), b[1:] + "A"]
    for c in (1, 2, 3):
        m.add(c, 0, range(5)); m.add(c, 0, range(100 * c, 100 * c + 5)); m.add(c, 1, [c])
    case = MergeCase("nobody_admissible", barcodes, m.mol, 8, 1, [SIMPLE])
    assert all(wm.edit_distance(b, x) >= 2 for x in barcodes[1:])
    assert len(smm.common_umigs(case, 0)) == 3 and case.answers(0)[0].fractions == {} and case.answers(0)[0].targets == {0}
    return case


def second_loop_case():
    """Chains for merge_inited's second loop (max_ed = 2; barcodes one substitution apart where a target is wanted):
      0 -> 1 -> 2     1, 2, 3 genes: the filtered order is 0, 1, 2, so 0 has moved into 1 when 1 moves into 2 and goes along
      3 -> 4 -> 5     3 and 4 have one gene, 4 fewer UMIs: 4 comes BEFORE 3 in the filtered order and is merged away (into 5) when 3 asks for it
      6, 7 -> 8       two bases into one target"""
    m = Mol(8)
    m.add(0, 0, range(4)); m.add(1, 0, range(8)); m.add(1, 1, range(50, 56)); m.add(2, 1, range(50, 56)); m.add(2, 2, [1]); m.add(2, 3, [2])
    m.add(4, 4, range(4)); m.add(3, 4, [0, 1, 2, 3, 9, 10]); m.add(5, 4, range(4)); m.add(5, 5, [1])
    m.add(6, 6, range(5)); m.add(7, 6, range(5, 10)); m.add(8, 6, range(12)); m.add(8, 7, [1])
    c = far_barcodes(3, 14, 99, 6)
    barcodes = [pc.sub(c[0], [1]), c[0], pc.sub(c[0], [5]), pc.sub(c[1], [1]), c[1], pc.sub(c[1], [5]), pc.sub(c[2], [1]), pc.sub(c[2], [5]), c[2]]
    case = MergeCase("second_loop", barcodes, m.mol, 8, 1, [SIMPLE])
    t = {b: a.target for b, a in case.answers(0).items()}
    assert t == {0: 1, 1: 2, 2: 2, 3: 4, 4: 5, 5: 5, 6: 8, 7: 8, 8: 8}
    order = case.filtered
    assert order.index(0) < order.index(1) and order.index(4) < order.index(3)
    assert smm.final_targets(case, t) == [2, 2, 2, 5, 5, 5, 8, 8, 8]
    return case


# ---- merge_type = all ---------------------------------------------------------------------------------------------------------
ALL_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 513)
ALL_POSITIONS = (0, 63, 64, 255, 256)


def all_positions_of(n_filtered):
    """(positions of the 10-UMI block that hold a target, whether the last position holds one too)"""
    last = n_filtered >= 4
    positions = []
    for p in ALL_POSITIONS:
        bases = len(positions) + 1 + last
        if p < n_filtered - bases - last:
            positions.append(p)
    return positions, last


def all_size_case(n_filtered):
    """F filtered cells with random barcodes of 12 bases (max_ed = 2): K cells of one gene and 10 UMIs, which the
    filtered order sorts by barcode; those at positions 0, 63, 64, 255 and 256 (as far as F allows) are the one admissible target of a
    base of two genes and 2 UMIs, one substitution away.  From F = 4 on the last position holds a cell of three genes and 20 UMIs, the
    target of one more base.  Every other cell stays."""
    positions, last = all_positions_of(n_filtered)
    n_bases = len(positions) + last
    block = n_filtered - n_bases - last
    plain = sorted(far_barcodes(block + last, 12, 200 + n_filtered))
    m = Mol(8)
    barcodes, want = [], {}
    for i in range(block):
        barcodes.append(plain[i])
        m.add(i, 0, range(10))
    targets = list(positions)
    if last:
        barcodes.append(plain[block])                     # (its place among the barcodes does not matter: three genes sort last)
        c = len(barcodes) - 1
        m.add(c, 0, range(10)); m.add(c, 1, range(9)); m.add(c, 2, [0])
        targets.append(c)
    for k, t in enumerate(targets):
        barcodes.append(pc.sub(barcodes[t], [(3 * k) % 12]))
        c = len(barcodes) - 1
        m.add(c, 0, [k]); m.add(c, 1, [k])
        want[c] = t
    case = MergeCase("all_F%d" % n_filtered, barcodes, m.mol, 8, 1, [Run("all", 2, 0)])
    assert len(case.filtered) == n_filtered == len(barcodes)
    for base, t in want.items():
        assert case.filtered.index(t) == (t if t < block else n_filtered - 1)
        assert case.answers(0)[base].targets == {t}
    assert all(case.answers(0)[c].targets == {c} for c in case.filtered if c not in want)
    case.target_positions = sorted(case.filtered.index(t) for t in want.values())
    return case


def all_rules_case():
    """Five neighbourhoods of barcodes of 12 bases, far from each other; in each, cell B and its candidates (UMIs, edits from B):
      equal     B 5 UMIs; E 5 UMIs at 1: equal counts are never a target -- B stays
      counts    B 5; P 8 at 1, Q 9 at 1: the same distance, Q has more UMIs
      order     B 5; P 8 at 1, Q 8 at 1: the same distance and count -- the earlier in the filtered order
      nearer    B 5; P 6 at 1, Q 30 at 2: the nearer one although it has fewer UMIs
      far       B 5; P 9 at 3
    Runs with max_ed = 0 (nobody merges), 1, 2 and 12, the barcode length."""
    centres = far_barcodes(5, 12, 300, 7)
    m = Mol(8)
    barcodes, cells = [], {}

    def cell(name, barcode, umis):
        barcodes.append(barcode)
        cells[name] = len(barcodes) - 1
        m.add(cells[name], 0, range(umis))

    cell("equal.B", centres[0], 5); cell("equal.E", pc.sub(centres[0], [2]), 5)
    cell("counts.B", centres[1], 5); cell("counts.P", pc.sub(centres[1], [2]), 8); cell("counts.Q", pc.sub(centres[1], [7]), 9)
    cell("order.B", centres[2], 5); cell("order.P", pc.sub(centres[2], [2]), 8); cell("order.Q", pc.sub(centres[2], [7]), 8)
    cell("nearer.B", centres[3], 5); cell("nearer.P", pc.sub(centres[3], [2]), 6); cell("nearer.Q", pc.sub(centres[3], [5, 9]), 30)
    cell("far.B", centres[4], 5); cell("far.P", pc.sub(centres[4], [1, 5, 9]), 9)
    case = MergeCase("all_rules", barcodes, m.mol, 8, 1, [Run("all", e, 0) for e in (0, 1, 2, 12)])
    case.cells = cells
    t = lambda i, name: case.answers(i)[cells[name]].target
    assert all(a.target == b for b, a in case.answers(0).items())
    first = min(cells["order.P"], cells["order.Q"], key=case.filtered.index)
    for i in (1, 2):
        assert t(i, "equal.B") == cells["equal.B"] and t(i, "counts.B") == cells["counts.Q"] and t(i, "order.B") == first
        assert t(i, "nearer.B") == cells["nearer.P"] and t(i, "far.B") == cells["far.B"]
    assert t(3, "far.B") == cells["far.P"]
    return case


BANDED_PAIR = ("CTTCGCCTGA", "CTGTCGCACTGA")


def all_two_lengths_case():
    """Barcodes of 10 and of 12 bases: the host's route, with the reference's banded distance.  Beside pairs one substitution and one
    insertion apart it holds BANDED_PAIR, filled in from a search: the banded distance (band 2) and the plain Levenshtein distance of
    that pair differ, so restating the plain distance on the host would show."""
    rng = random.Random(401)
    centres = far_barcodes(4, 10, 400, 5)
    m = Mol(8)
    barcodes = []
    for k, c in enumerate(centres):
        at = 3 + k
        barcodes += [c, pc.sub(c, [k]), c[:at] + "GT"[c[at] == "G"] + c[at:] + "ACGT"[k]]         # 10, 10 and 12 bases
        for j, umis in enumerate((5, 9 + k, 14)):
            m.add(3 * k + j, 0, rng.sample(range(60000), umis))
    barcodes += list(BANDED_PAIR)
    m.add(len(barcodes) - 2, 0, range(3)); m.add(len(barcodes) - 1, 0, range(40))
    case = MergeCase("all_two_lengths", barcodes, m.mol, 8, 1, [Run("all", 2, 0), Run("all", 1, 0)])
    assert {len(b) for b in barcodes} == {10, 12}
    base, other = len(barcodes) - 2, len(barcodes) - 1
    assert smm.banded_edit_distance(BANDED_PAIR[0], BANDED_PAIR[1], False, 2) == 3 and wm.edit_distance(*BANDED_PAIR) == 2
    assert case.answers(0)[base].targets == {base}                            # (the plain distance, 2, would merge it into `other`)
    case.banded_pair = (base, other)
    return case


def all_with_n_case():
    """Barcodes of one length, one of them with an N: the host's route again.  N is no wildcard here (skip_n = false): the cell with the N is
    one edit from its clean twin and merges into it, a cell two substitutions from the twin merges into the twin, not into the N."""
    c = far_barcodes(3, 12, 500, 6)
    barcodes = [c[0], c[0][:6] + "N" + c[0][7:], pc.sub(c[0], [1, 9]), c[1], pc.sub(c[1], [3]), c[2]]
    m = Mol(8)
    for cell, umis in enumerate((30, 12, 4, 8, 3, 50)):
        m.add(cell, 0, range(umis))
    case = MergeCase("all_with_n", barcodes, m.mol, 8, 1, [Run("all", 2, 0)])
    assert [case.answers(0)[b].target for b in range(6)] == [0, 0, 0, 3, 3, 5] and len(case.side) == 1
    return case


# ---- random containers --------------------------------------------------------------------------------------------------------
RANDOM_SEEDS = list(range(12))
UNDECIDED_CAP = 0.02                                      # of the filtered bases of a random container


def random_case(seed):
    """20 to 60 cells, 5 to 40 genes, UMIs of 6 to 9 bases; a third of the cells are real, the others error barcodes one or two
    substitutions from a real one that hold a share of its molecules and a few of their own."""
    rng = random.Random(7000 + seed)
    umi_len = 6 + seed % 4
    n_cells, n_genes = rng.randint(20, 60), rng.randint(5, 40)
    n_real = max(3, n_cells // 3)
    real = far_barcodes(n_real, 12, 7100 + seed, 5)
    m = Mol(umi_len)
    barcodes = list(real)
    pool = 4 ** umi_len
    for c in range(n_real):
        for g in rng.sample(range(n_genes), rng.randint(max(2, n_genes // 2), n_genes)):
            m.add(c, g, rng.sample(range(pool), rng.randint(2, 14)))
    while len(barcodes) < n_cells:
        src = rng.randrange(n_real)
        t = pc.sub(real[src], rng.sample(range(12), rng.randint(1, 2)))
        if t in barcodes:
            continue
        barcodes.append(t)
        c = len(barcodes) - 1
        share = rng.choice((0.05, 0.15, 0.3, 0.6))
        for _, g, u in sorted(x for x in m.mol if x[0] == src):
            if rng.random() < share:
                m.add(c, g, [u])
        for g in rng.sample(range(n_genes), rng.randint(1, 3)):
            m.add(c, g, rng.sample(range(pool), rng.randint(1, 3)))
    used = sorted({g for _, g, _ in m.mol})
    relabel = {g: i for i, g in enumerate(used)}
    mol = {(c, relabel[g], u) for c, g, u in m.mol}
    return MergeCase("random_%d" % seed, barcodes, mol, umi_len, 2, [Run("simple", 3, 0.1), Run("simple", 2, 0.2), Run("all", 2, 0)],
                     hand_built=False)


_CASES = {
    "pair_runs": pair_runs_case,
    "high_cell_ids": partial(pair_runs_case, "high_cell_ids", 5000),
    "hot_600": hot_600_case,
    "tiles": tiles_case,
    "shared_counts": shared_counts_case,
    "barcode_lengths": lengths_case,
    "barcode_long": long_case,
    "exact_fractions": exact_fractions_case,
    "tie_unique_genes": tie_unique_case,
    "tie_shared_genes": tie_shared_case,
    "tie_chain": tie_chain_case,
    "tie_band_genes": tie_band_case,
    "hot_umig": hot_umig_case,
    "nobody_admissible": nobody_admissible_case,
    "second_loop": second_loop_case,
    "all_rules": all_rules_case,
    "all_two_lengths": all_two_lengths_case,
    "all_with_n": all_with_n_case,
}
for _end in (255, 256, 257):
    _CASES["run_end_%d" % _end] = partial(run_end_case, _end)
for _width in KEY_WIDTHS:
    _CASES["key_width_%d" % _width] = partial(key_width_case, _width)
for _ed in DISTANCE_MAX_EDS:
    _CASES["distance_ed%d" % _ed] = partial(distance_case, _ed)
for _d in (1, 3, 5):
    _CASES["eps_band_%d" % _d] = partial(eps_band_case, _d)
for _f in ALL_SIZES:
    _CASES["all_F%d" % _f] = partial(all_size_case, _f)
HAND_BUILT = sorted(_CASES)
for _seed in RANDOM_SEEDS:
    _CASES["random_%d" % _seed] = partial(random_case, _seed)
RANDOM = ["random_%d" % s for s in RANDOM_SEEDS]
NAMES = HAND_BUILT + RANDOM
ORDER_DEPENDENT = ("tie_shared_genes", "tie_chain")
DISTANCE_CASES = ["distance_ed%d" % e for e in DISTANCE_MAX_EDS] + ["barcode_lengths", "barcode_long"]
KEY_WIDTH_CASES = ["key_width_%d" % w for w in KEY_WIDTHS]

_built = {}


def case(name):
    """the case of that name, built once per process (its model results are cached on it)"""
    if name not in _built:
        _built[name] = _CASES[name]()
        assert _built[name].name == name
    return _built[name]


def runs_of(names=None, kinds=("simple", "poisson", "all")):
    """[(case name, run index)] for parametrised tests, without building a case"""
    counts = {"exact_fractions": ["simple"] * 4, "all_rules": ["all"] * 4, "all_two_lengths": ["all"] * 2}
    out = []
    for name in (NAMES if names is None else names):
        if name in counts:
            kinds_of = counts[name]
        elif name.startswith("all_"):
            kinds_of = ["all"]
        elif name.startswith("random_"):
            kinds_of = ["simple", "simple", "all"]
        elif name in DISTANCE_CASES or name in ("pair_runs", "high_cell_ids"):
            kinds_of = ["simple", "poisson"]
        else:
            kinds_of = ["simple"]
        out += [(name, i) for i, k in enumerate(kinds_of) if k in kinds]
    return out
