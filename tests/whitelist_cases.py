"""The whitelists, universes and bases of the whitelist search tests (test_whitelist_model_cpu.py runs them through
whitelist_model.py and the oracle, test_gpu_whitelist_search.py through both device routes).

A case is a whitelist (kind + parts), a merge kind, min_genes_before_merge, a universe of cells (barcode text, gene
count, TOTAL_UMIS) and the bases to search for.  Every cell has 1 <= n_genes <= total_umis, so that a plain stream
of reads gives the oracle exactly these cells.  What a case claims about itself -- stop levels, candidate counts --
is asserted here from the model when the case is built: a case that no longer reaches its edge fails on any machine.

Routes.  With neighbour tables (every part of one length of at most 9 clean bases, at most four parts) a base is
decided from 128-byte rows that hold the counts at distance 0..3 and list at most 60 entries, closest groups first;
`takes_full_search` restates from those documented limits which bases are handed on to the full search.
"""
import itertools
import random
from functools import lru_cache, partial

import whitelist_model as wm
from whitelist_model import CONST, INDROP, Universe

TAB_MAX_LEN, TAB_MAX_DIST, TAB_LIST, TAB_FOUND, MAX_PARTS, CAND_CAP = 9, 3, 60, 12, 4, 128
ACGT = "ACGT"


class Case:
    def __init__(self, name, kind, parts, poisson, min_genes, universe, bases, error=None):
        self.name, self.kind, self.parts, self.poisson, self.min_genes = name, kind, parts, poisson, min_genes
        self.universe, self.bases, self.error = universe, list(bases), error
        self._searches = None

    @property
    def has_tables(self):
        return len(self.parts) <= MAX_PARTS and all(
            1 <= len(part[0]) <= TAB_MAX_LEN and all(len(e) == len(part[0]) and set(e) <= set(ACGT) for e in part) for part in self.parts)

    def searches(self):
        """the model's result per base, computed once"""
        if self._searches is None:
            self._searches = [wm.search(self.kind, self.parts, self.poisson, self.min_genes, self.universe, b) for b in self.bases]
        return self._searches

    def pairs(self):
        return {b: sorted(wm.pairs(b, s.candidates, self.poisson)) for b, s in zip(self.bases, self.searches())}

    def takes_full_search(self, base, s):
        """whether the table search hands this base on (the case has tables)"""
        pieces = wm.split_barcode(self.kind, self.parts, self.universe.barcode[base])
        if any(len(x) != len(part[0]) or "N" in x for x, part in zip(pieces, self.parts)):
            return True                                                  # a part of another length or with an N
        counts = [c[:TAB_MAX_DIST + 1] for c in s.part_counts]
        if any(sum(c) == 0 for c in counts):
            return True                                                  # no entry within 3 in some part
        if s.horizon > TAB_MAX_DIST or len(s.candidates) > TAB_FOUND:
            return True                                                  # a level beyond 3; more than 12 candidates
        first = sum(min(d for d in range(TAB_MAX_DIST + 1) if c[d]) for c in counts)
        for tup in itertools.product(range(TAB_MAX_DIST + 1), repeat=len(counts)):
            if first <= sum(tup) <= s.horizon and all(c[d] for c, d in zip(counts, tup)):
                if any(sum(c[:d + 1]) > TAB_LIST for c, d in zip(counts, tup)):
                    return True                                          # a needed distance group is not listed in its row
        return False

    def n_full_search(self):
        """The device reports the route only as a count over a search, so two opposite mistakes of takes_full_search on single bases
        would cancel.  The cases whose count is 0 or every base (dense_12 / dense_13 / dense_5_at_level ...) pin the rule at both ends."""
        return sum(self.takes_full_search(b, s) for b, s in zip(self.bases, self.searches()))


# ---- helpers ------------------------------------------------------------------------------------------------------------
def rnd_seq(rng, n):
    return "".join(rng.choice(ACGT) for _ in range(n))


def distinct_seqs(rng, count, n):
    out = []
    while len(out) < count:
        s = rnd_seq(rng, n)
        if s not in out:
            out.append(s)
    return out


def substitute(rng, s, k, lo=0, hi=None):
    """k substitutions at distinct places of s[lo:hi]"""
    hi = len(s) if hi is None else hi
    t = list(s)
    for i in rng.sample(range(lo, hi), k):
        t[i] = rng.choice([c for c in ACGT if c != t[i]])
    return "".join(t)


def all_combinations(parts):
    return ["".join(t) for t in itertools.product(*parts)]


class Cells:
    """a universe under construction: first writer of a barcode wins"""

    def __init__(self):
        self.barcode, self.n_genes, self.total_umis, self.index = [], [], [], {}

    def add(self, barcode, n_genes, total_umis):
        assert 1 <= n_genes <= total_umis
        if barcode in self.index:
            return None
        self.index[barcode] = len(self.barcode)
        self.barcode.append(barcode); self.n_genes.append(n_genes); self.total_umis.append(total_umis)
        return self.index[barcode]

    def universe(self):
        return Universe(self.barcode, self.n_genes, self.total_umis)


# ---- dense whitelist: all 256 4-mers in each of two parts ------------------------------------------------------------------
FOUR_MERS = ["".join(t) for t in itertools.product(ACGT, repeat=4)]
DENSE = [FOUR_MERS, FOUR_MERS]
DENSE_MIN_GENES, BASE_UMIS = 3, 5


def dense_neighbours(barcode, level):
    """whitelist barcodes whose per-part distances to `barcode` sum to `level` (with repeats never: the entries are distinct)"""
    a, b = barcode[:4], barcode[4:]
    da = {e: wm.edit_distance(a, e) for e in FOUR_MERS}
    db = {e: wm.edit_distance(b, e) for e in FOUR_MERS}
    return [x + y for x in FOUR_MERS for y in FOUR_MERS if da[x] + db[y] == level]


# the 4-mers with 1 / 12 / 72 / 130 entries at distance 0 / 1 / 2 / 3 (48 of the 256: a repeated letter brings fewer distinct
# neighbours).  Every 4-mer has at least 1 + 12 + 54 = 67 entries within 2, so no row lists its group 2.
FULL_ROWS = [v for v in FOUR_MERS if [sum(1 for e in FOUR_MERS if wm.edit_distance(v, e) == d) for d in range(4)] == [1, 12, 72, 130]]


def far_apart_bases(rng, count, min_dist):
    """8-mers of two FULL_ROWS parts whose pairwise whitelist distance (sum over the two parts) is at least min_dist"""
    out = []
    for _ in range(100000):
        if len(out) == count:
            break
        s = rng.choice(FULL_ROWS) + rng.choice(FULL_ROWS)
        if all(wm.edit_distance(s[:4], t[:4]) + wm.edit_distance(s[4:], t[4:]) >= min_dist for t in out):
            out.append(s)
    assert len(out) == count
    return out


def dense_case(name, n_l1, n_l2, poisson=False, n_bases=4, base_genes=DENSE_MIN_GENES - 1, seed=1, error=None, all_l1=False):
    """Every base is a whitelist barcode (every 8-mer is).  Per base the universe holds n_l1 qualifying cells at level 1 and n_l2 at
    level 2; the other level-1 barcodes are there too, half of them one gene short and half one UMI short of qualifying."""
    rng = random.Random(seed)
    cells, bases = Cells(), []
    texts = far_apart_bases(rng, n_bases, 3 if all_l1 else 5)     # 5: the cells within 2 of one base lie 3 or more from any other
    for t in texts:
        bases.append(cells.add(t, base_genes, BASE_UMIS))
    for t in texts:
        l1, l2 = dense_neighbours(t, 1), dense_neighbours(t, 2)
        assert len(l1) == 24 and len(l2) == 288
        rng.shuffle(l1); rng.shuffle(l2)
        for k, x in enumerate(l1):
            if k < n_l1:
                got = cells.add(x, DENSE_MIN_GENES + k % 2, BASE_UMIS + k % 3)           # equality passes both tests
            elif k % 2:
                got = cells.add(x, DENSE_MIN_GENES - 1, BASE_UMIS + 4)                   # one gene short
            else:
                got = cells.add(x, DENSE_MIN_GENES, BASE_UMIS - 1)                       # one UMI short
            assert got is not None
        for x in l2[:n_l2]:
            assert cells.add(x, DENSE_MIN_GENES + 1, BASE_UMIS + 1) is not None
    return Case(name, CONST, DENSE, poisson, DENSE_MIN_GENES, cells.universe(), bases, error=error)


@lru_cache(maxsize=None)
def dense_cases():
    out = {}
    # (a) 12 of the 24 level-1 neighbours qualify: as many candidates as the table search keeps
    c = out["dense_12_at_level_1"] = dense_case("dense_12_at_level_1", 12, 10)
    assert all(len(s.candidates) == 12 and s.level_found == {1: 12} for s in c.searches()) and c.n_full_search() == 0
    # (b) 13: one more than it keeps
    c = out["dense_13_at_level_1"] = dense_case("dense_13_at_level_1", 13, 10, seed=2)
    assert all(len(s.candidates) == 13 and s.level_found == {1: 13} for s in c.searches()) and c.n_full_search() == len(c.bases)
    # (c) nothing at level 1, a handful at level 2: the tuple (2, 0) needs a group no row lists (1 + 12 + 72 > 60)
    c = out["dense_5_at_level_2"] = dense_case("dense_5_at_level_2", 0, 5, seed=3)
    assert all(s.part_counts[p][:4] == [1, 12, 72, 130] for s in c.searches() for p in (0, 1))
    assert all(s.level_found == {2: 5} and s.horizon == 2 for s in c.searches()) and c.n_full_search() == len(c.bases)
    # (d) exactly as many candidates as a base may have, (e) one more
    c = out["dense_128_at_level_2"] = dense_case("dense_128_at_level_2", 0, CAND_CAP, n_bases=2, seed=4)
    assert all(s.level_found == {2: CAND_CAP} for s in c.searches())
    c = out["dense_129_at_level_2"] = dense_case("dense_129_at_level_2", 0, CAND_CAP + 1, n_bases=2, seed=5,
                                                 error="more than 128 merge candidates")
    assert all(s.level_found == {2: CAND_CAP + 1} for s in c.searches())
    # (f) Poisson, the base a qualifying whitelist barcode: levels 0, 1 and 2 are all taken (1 + 24 + 288 = 313 combinations)
    c = out["dense_poisson_levels_0_to_2"] = dense_case("dense_poisson_levels_0_to_2", 10, 100, poisson=True, n_bases=2,
                                                        base_genes=DENSE_MIN_GENES, seed=6)
    assert all(s.level_found == {0: 1, 1: 10, 2: 100} and s.candidates[0] == b for b, s in zip(c.bases, c.searches()))
    assert all(len(p) == 110 and b not in p for b, p in c.pairs().items())
    # (g) 50 bases x 24 candidates = 1200: more than the flat lists hold at first (max(2 * 50, 1024))
    c = out["dense_1200_candidates"] = dense_case("dense_1200_candidates", 24, 0, n_bases=50, seed=7, all_l1=True)
    assert all(s.level_found == {1: 24} for s in c.searches()) and len(c.bases) == 50
    return out


# ---- sparse whitelists: at most 60 entries per part, every row lists all four groups ------------------------------------------
def sparse_case(name, n_entries, length, poisson, seed, n_bases):
    rng = random.Random(seed)
    parts = [distinct_seqs(rng, n_entries, length), distinct_seqs(rng, n_entries, length)]
    cells = Cells()
    for t in rng.sample(all_combinations(parts), 300):
        g = rng.randint(1, 4)
        cells.add(t, g, rng.randint(max(g, 3), 8))
    real = list(cells.barcode)
    bases, tries = [], 0
    while len(bases) < n_bases:
        k, one_part, second = 1 + tries % 6, (tries // 6) % 3 == 0, (tries // 18) % 2
        tries += 1
        t = rng.choice(real)
        # the substitutions over the whole barcode, or (every third round) all of them in one part
        t = substitute(rng, t, k, second * length, (second + 1) * length) if one_part else substitute(rng, t, k)
        g = rng.randint(1, 3)
        b = cells.add(t, g, rng.randint(max(g, 3), 6))
        if b is not None:
            bases.append(b)
    return Case(name, CONST, parts, poisson, 2, cells.universe(), bases)


def far_part_case():
    """Tables, and bases with a part farther than 5 from every entry: the entries have no A, the part is all A (or all but one)."""
    rng = random.Random(13)
    def no_a(n):
        out = []
        while len(out) < n:
            e = "".join(rng.choice("CGT") for _ in range(7))
            if e not in out:
                out.append(e)
        return out
    parts = [no_a(40), no_a(40)]
    cells = Cells()
    for t in rng.sample(all_combinations(parts), 120):
        g = rng.randint(1, 3)
        cells.add(t, g, rng.randint(max(g, 3), 6))
    real = list(cells.barcode)
    far = []
    for k in range(6):
        t = real[k]
        far.append(cells.add(("AAAAAAA" + t[7:], t[:7] + "AAAAAAA", "AAAAAAA" + substitute(rng, t, 1, 7, 14)[7:],
                              t[:1] + "AAAAAA" + t[7:], t[:7] + "AAAAAA" + t[13:], "AAAAAAAAAAAAAA")[k], 1, 3))
    bases = list(far)
    while len(bases) < 30:
        b = cells.add(substitute(rng, rng.choice(real), 1 + len(bases) % 3), 1, 3)
        if b is not None:
            bases.append(b)
    c = Case("sparse_far_part", CONST, parts, False, 2, cells.universe(), sorted(bases))
    by_base = dict(zip(c.bases, c.searches()))
    assert all(by_base[b].min_level is None and any(sum(x) == 0 for x in by_base[b].part_counts) for b in far)
    assert all(c.takes_full_search(b, by_base[b]) for b in far)
    return c


@lru_cache(maxsize=None)
def sparse_cases():
    out = {}
    for poisson in (False, True):
        tag = "_poisson" if poisson else ""
        out["sparse_40x7" + tag] = sparse_case("sparse_40x7" + tag, 40, 7, poisson, 11, 240)
        out["sparse_60x9" + tag] = sparse_case("sparse_60x9" + tag, 60, 9, poisson, 12, 150)
    out["sparse_far_part"] = far_part_case()
    plain = out["sparse_40x7"].searches() + out["sparse_60x9"].searches()
    assert {s.horizon for s in plain if s.candidates} >= {1, 2, 3, 4, 5}
    assert any(not s.candidates and s.min_level is not None for s in plain)                       # combinations, none of them a qualifying cell
    assert any(any(sum(c[:4]) == 0 for c in s.part_counts) for s in plain)                        # a part with nothing within 3 (long_case: none within 5)
    for c in out.values():
        assert c.has_tables and all(sum(x[:4]) <= TAB_LIST for s in c.searches() for x in s.part_counts)
        assert 0 < c.n_full_search() < len(c.bases)
    return out


# ---- small random whitelists ---------------------------------------------------------------------------------------------------
def small_whitelist(rng, lengths, n_entries=8):
    return [distinct_seqs(rng, n_entries, n) for n in lengths]


def boundary_case(poisson):
    """Candidate test at its boundaries; a base that is its own only candidate."""
    rng = random.Random(21)
    parts = small_whitelist(rng, (5, 5))
    combos = all_combinations(parts)
    cells, bases = Cells(), []
    min_genes = 2
    targets = {                                                   # whitelist cells (n_genes, total_umis)
        combos[0]: (2, 5), combos[9]: (1, 5), combos[18]: (2, 7), combos[27]: (3, 3), combos[36]: (2, 9),
    }
    for t, (g, u) in targets.items():
        cells.add(t, g, u)
    origin = {}
    for t in targets:
        for k, u in enumerate((4, 5, 6, 7, 8)):                   # around every target's UMI count: one fewer, equal, one more
            for n_sub in (1, 2):
                b = cells.add(substitute(rng, t, n_sub), 1 + k % 2, u)
                if b is not None:
                    bases.append(b)
                    origin[b] = cells.index[t]
    bases += [cells.index[t] for t in targets]                    # the whitelist cells themselves: combos[27] is far from all others
    name = "boundaries_poisson" if poisson else "boundaries"
    c = Case(name, CONST, parts, poisson, min_genes, cells.universe(), sorted(bases))
    by_base = dict(zip(c.bases, c.searches()))
    own = [b for b in c.bases if by_base[b].candidates == [b]]
    assert own and all(c.pairs()[b] == [] for b in own)           # its own only candidate: no pair under either merge kind
    u = c.universe
    flat = [(b, x) for b in c.bases for x in by_base[b].candidates if x != b]
    assert any(u.total_umis[x] == u.total_umis[b] for b, x in flat) and any(u.n_genes[x] == min_genes for b, x in flat)
    # ... and the failing side: the whitelist cell a base was made from lies at the first level the scan looks at, and is turned down
    # only for being one UMI, or one gene, short
    def nearest(b, x):
        pieces, entry = wm.split_barcode(CONST, parts, u.barcode[b]), wm.split_barcode(CONST, parts, u.barcode[x])
        return sum(wm.edit_distance(p, e) for p, e in zip(pieces, entry)) == by_base[b].min_level
    turned_down = [(b, x) for b, x in origin.items() if nearest(b, x) and x not in by_base[b].candidates]
    assert any(u.total_umis[x] == u.total_umis[b] - 1 and u.n_genes[x] >= min_genes for b, x in turned_down)
    assert any(u.n_genes[x] == min_genes - 1 and u.total_umis[x] >= u.total_umis[b] for b, x in turned_down)
    return c


def parts_case(lengths, poisson, seed):
    rng = random.Random(seed)
    parts = small_whitelist(rng, lengths, 40 if len(lengths) == 1 else 7)
    cells = Cells()
    combos = all_combinations(parts)
    for t in rng.sample(combos, min(150, len(combos) * 3 // 4)):
        g = rng.randint(1, 3)
        cells.add(t, g, rng.randint(max(g, 2), 6))
    real = list(cells.barcode)
    bases = rng.sample(range(len(real)), 10)                       # whitelist cells
    while len(bases) < 70:
        g = rng.randint(1, 2)
        b = cells.add(substitute(rng, rng.choice(real), 1 + len(bases) % 4), g, rng.randint(max(g, 2), 5))
        if b is not None:
            bases.append(b)
    name = "parts_%d%s" % (len(lengths), "_poisson" if poisson else "")
    return Case(name, CONST, parts, poisson, 2, cells.universe(), bases)         # (bases in no particular order)


def with_n(s, places):
    t = list(s)
    for i in places:
        t[i] = "N"
    return "".join(t)


def n_case(poisson):
    """Bases with N: inside a part, at its ends, two of them, a whole part of N."""
    rng = random.Random(31)
    parts = small_whitelist(rng, (6, 6), 20)
    cells = Cells()
    for t in rng.sample(all_combinations(parts), 200):
        g = rng.randint(1, 3)
        cells.add(t, g, rng.randint(max(g, 2), 6))
    real = list(cells.barcode)
    bases = []
    places = [(2,), (0,), (5,), (6,), (11,), (8,), (1, 3), (0, 5), (5, 6), (2, 9), tuple(range(6)), tuple(range(6, 12))]
    for k, where in enumerate(places * 3):
        t = rng.choice(real)
        if k >= len(places):
            t = substitute(rng, t, 1 + k % 2)                    # an N beside one or two substitutions
        b = cells.add(with_n(t, where), 1, 2 + k % 3)
        if b is not None:
            bases.append(b)
    n_with_n = len(bases)
    while len(bases) < n_with_n + 12:                            # clean bases beside them: these stay in the table route
        b = cells.add(substitute(rng, rng.choice(real), 1), 1, 2)
        if b is not None:
            bases.append(b)
    c = Case("n_bases_poisson" if poisson else "n_bases", CONST, parts, poisson, 2, cells.universe(), bases)
    texts = [c.universe.barcode[b] for b in c.bases]
    assert any("NNNNNN" in t for t in texts) and any(t.count("N") == 2 for t in texts)
    assert n_with_n <= c.n_full_search() < len(c.bases)
    assert any(s.level_found.get(0, 0) > 1 for s in c.searches())   # a wildcard matches several entries at distance 0
    return c


def indrop_case(poisson):
    """inDrop whitelist with first-part entries of two lengths: insertions and deletions in the first part, an empty first part."""
    rng = random.Random(41)
    parts = [distinct_seqs(rng, 6, 5) + distinct_seqs(rng, 6, 6), distinct_seqs(rng, 10, 6)]
    cells = Cells()
    for t in all_combinations(parts):
        if rng.random() < 0.8:
            g = rng.randint(1, 3)
            cells.add(t, g, rng.randint(max(g, 2), 6))
    real = list(cells.barcode)
    bases = rng.sample(range(len(real)), 6)
    tries = 0
    while len(bases) < 60:
        t = rng.choice(real)
        n1 = len(t) - 6
        i = rng.randrange(n1)
        how = tries % 4
        tries += 1
        if how == 0:
            t = t[:i] + rng.choice(ACGT) + t[i:]                   # insertion in the first part
        elif how == 1:
            t = t[:i] + t[i + 1:]                                  # deletion in the first part
        elif how == 2:
            t = substitute(rng, t, 2)
        else:
            t = t[:i] + t[i + 2:] if n1 == 6 else substitute(rng, t[:i] + rng.choice(ACGT) + t[i:], 1, n1 + 1)
        b = cells.add(t, 1, rng.randint(2, 4))
        if b is not None:
            bases.append(b)
    for e in parts[1][:3]:                                        # exactly as long as part 2: the first part is empty
        bases.append(cells.add(e, 1, 2))
    c = Case("indrop_poisson" if poisson else "indrop", INDROP, parts, poisson, 2, cells.universe(), sorted(bases))
    assert not c.has_tables
    empty_first = [s for b, s in zip(c.bases, c.searches()) if len(c.universe.barcode[b]) == 6]
    assert len(empty_first) == 3 and all(s.min_level == 5 for s in empty_first) and any(s.candidates for s in empty_first)
    return c


def long_case(lengths, seed):
    """Parts of up to 31 bases; the entries are relatives of one root, so that neighbours lie at several small distances."""
    rng = random.Random(seed)
    parts = []
    for n in lengths:
        root = rnd_seq(rng, n)
        part = [root]
        while len(part) < 12:
            e = substitute(rng, rng.choice(part), rng.randint(1, 2))
            if e not in part:
                part.append(e)
        parts.append(part)
    cells = Cells()
    for t in all_combinations(parts)[:200]:
        g = rng.randint(1, 3)
        cells.add(t, g, rng.randint(max(g, 2), 6))
    real = list(cells.barcode)
    bases = rng.sample(range(len(real)), 8)                        # distance 0
    while len(bases) < 40:
        b = cells.add(substitute(rng, rng.choice(real), 1 + len(bases) % 2), 1, rng.randint(2, 4))
        if b is not None:
            bases.append(b)
    bases.append(cells.add(rnd_seq(rng, sum(lengths)), 1, 2))      # a stranger: no entry within 5 of its parts
    c = Case("long_" + "_".join(map(str, lengths)), CONST, parts, False, 2, cells.universe(), sorted(bases))
    assert not c.has_tables and {0, 1, 2} <= {s.min_level for s in c.searches()}
    assert any(s.min_level is None and any(sum(x) == 0 for x in s.part_counts) for s in c.searches())
    return c


def repeated_entry_case(poisson):
    """One entry twice in the first part: the reference walks both copies, a candidate that holds it comes twice."""
    rng = random.Random(51)
    parts = small_whitelist(rng, (5, 5), 9)
    twice = parts[0][3]
    parts[0].insert(7, twice)
    cells = Cells()
    for t in all_combinations(parts):
        if t.startswith(twice) or rng.random() < 0.5:
            cells.add(t, 2, rng.randint(3, 6))
    real = list(cells.barcode)
    bases = [cells.index[t] for t in real if t.startswith(twice)][:4]   # a base that is itself twice on the whitelist
    while len(bases) < 40:
        t = rng.choice(real)
        t = substitute(rng, t, 1, 5, 10) if len(bases) % 2 else substitute(rng, t, 1 + len(bases) % 3)
        b = cells.add(t, 1, rng.randint(2, 4))
        if b is not None:
            bases.append(b)
    c = Case("repeated_entry_poisson" if poisson else "repeated_entry", CONST, parts, poisson, 2, cells.universe(), sorted(bases))
    by_base = dict(zip(c.bases, c.searches()))
    assert sum(1 for b in c.bases if by_base[b].candidates[:2] == [b, b]) == 4
    assert any(x != b and s.candidates.count(x) == 2 for b, s in by_base.items() for x in s.candidates)
    assert c.has_tables
    return c


@lru_cache(maxsize=None)
def error_cases():
    """Bases that split_barcode refuses.  Const length: the reference's text (ConstLengthBarcodesParser::split_barcode).  inDrop: the
    reference has no text of its own there -- its substr throws std::out_of_range -- so the expected text is this project's (whitelist.h)."""
    rng = random.Random(61)
    parts = small_whitelist(rng, (5, 5))
    cells = Cells()
    for t in all_combinations(parts)[:20]:
        cells.add(t, 2, 3)
    good = cells.add(substitute(rng, cells.barcode[0], 1), 1, 2)
    long_one = cells.add(cells.barcode[1] + "A", 1, 2)
    const = Case("error_const_wrong_length", CONST, parts, False, 2, cells.universe(), [good, long_one],
                 error="Barcode '%s' has wrong length (10 expected)" % cells.barcode[long_one])
    parts = [distinct_seqs(rng, 6, 5) + distinct_seqs(rng, 6, 6), distinct_seqs(rng, 8, 6)]
    cells = Cells()
    for t in all_combinations(parts)[:20]:
        cells.add(t, 2, 3)
    good = cells.add(substitute(rng, cells.barcode[0], 1), 1, 2)
    short = cells.add(parts[1][0][:5], 1, 2)
    indrop = Case("error_indrop_too_short", INDROP, parts, False, 2, cells.universe(), [good, short],
                  error="Barcode '%s' is shorter than the second whitelist part" % cells.barcode[short])
    return {c.name: c for c in (const, indrop)}


def _from(group, name):
    return lambda: group()[name]


# name -> builder; the dense, sparse and error groups build their cases together (functools.lru_cache: once per process)
_BUILDERS = {
    "dense_12_at_level_1": _from(dense_cases, "dense_12_at_level_1"),
    "dense_13_at_level_1": _from(dense_cases, "dense_13_at_level_1"),
    "dense_5_at_level_2": _from(dense_cases, "dense_5_at_level_2"),
    "dense_128_at_level_2": _from(dense_cases, "dense_128_at_level_2"),
    "dense_129_at_level_2": _from(dense_cases, "dense_129_at_level_2"),
    "dense_poisson_levels_0_to_2": _from(dense_cases, "dense_poisson_levels_0_to_2"),
    "dense_1200_candidates": _from(dense_cases, "dense_1200_candidates"),
    "sparse_40x7": _from(sparse_cases, "sparse_40x7"),
    "sparse_40x7_poisson": _from(sparse_cases, "sparse_40x7_poisson"),
    "sparse_60x9": _from(sparse_cases, "sparse_60x9"),
    "sparse_60x9_poisson": _from(sparse_cases, "sparse_60x9_poisson"),
    "sparse_far_part": _from(sparse_cases, "sparse_far_part"),
    "boundaries": partial(boundary_case, False),
    "boundaries_poisson": partial(boundary_case, True),
    "parts_1": partial(parts_case, (6,), False, 70),
    "parts_1_poisson": partial(parts_case, (6,), True, 70),
    "parts_3": partial(parts_case, (4, 5, 3), False, 71),
    "parts_3_poisson": partial(parts_case, (4, 5, 3), True, 71),
    "parts_4": partial(parts_case, (3, 4, 3, 4), False, 72),
    "parts_4_poisson": partial(parts_case, (3, 4, 3, 4), True, 72),
    "parts_5": partial(parts_case, (3, 3, 3, 3, 3), False, 73),
    "parts_5_poisson": partial(parts_case, (3, 3, 3, 3, 3), True, 73),
    "n_bases": partial(n_case, False),
    "n_bases_poisson": partial(n_case, True),
    "indrop": partial(indrop_case, False),
    "indrop_poisson": partial(indrop_case, True),
    "long_29": partial(long_case, (29,), 80),
    "long_30": partial(long_case, (30,), 81),
    "long_31": partial(long_case, (31,), 82),
    "long_15_16": partial(long_case, (15, 16), 83),
    "repeated_entry": partial(repeated_entry_case, False),
    "repeated_entry_poisson": partial(repeated_entry_case, True),
    "error_const_wrong_length": _from(error_cases, "error_const_wrong_length"),
    "error_indrop_too_short": _from(error_cases, "error_indrop_too_short"),
}
CASE_NAMES = sorted(_BUILDERS)
_built = {}


def case(name):
    """the case of that name, built (and its model run) once per process"""
    if name not in _built:
        _built[name] = _BUILDERS[name]()
        assert _built[name].name == name
    return _built[name]
