"""A plain model of the directional UMI correction (-u): MergeUMIsStrategyDirectional::merge / find_targets / find_target
(Estimation/Merge/UMIs/MergeUMIsStrategyDirectional.cpp:18-116) with the two library behaviours its answer hangs on restated in the open:
libstdc++'s std::sort (bits/stl_algo.h, bits/stl_heap.h), whose arrangement of equal read counts decides which of two equally-read UMIs
survives, and the banded edit distance of Tools/UtilFunctions.cpp:32-65.  Pure Python: integers, strings, and Python floats (IEEE doubles,
as in the reference) in the multiplier test.  test_directional_model_cpu.py pins every piece on the oracle; test_gpu_directional.py holds
the device against it.

Groups with an N-UMI or with UMIs of several lengths are not decided here (find_targets raises): their answer hangs on rand() and on the
iteration order of an unordered map, and the library replays them on the host.

VARIANTS names the ways a kernel could be subtly wrong; every function takes `variant`, a set of those names, and test_directional_model_cpu.py
asserts that each of them changes the expected answer of a named case."""
from collections import namedtuple
from functools import cmp_to_key

VARIANTS = ("stable_sort",        # (reads, first occurrence) at every size, not only up to 16
            "no_heap_fallback",   # the ranges that reach the depth limit are sorted stably instead of by the heapsort
            "hamming",            # Hamming in place of the edit distance
            "local_index",        # UMI-index order of the group's own first occurrences, not of the stream's
            "geneless_indexed",   # reads without a gene take part in the UMI index
            "mult_ge",            # reads(src) * mult >= reads(dst) breaks the search
            "ed_le",              # ed <= min_ed takes the later hit
            "no_chain")           # no chain shortening
THRESHOLD = 16                    # libstdc++ _S_threshold
FAST_FROM = 512                   # groups from this size on, at max_ed = 1, find their neighbours by lookup (_find_target_by_lookup)


# ---- std::sort ------------------------------------------------------------------------------------------------------------------
class _Sort:
    """std::sort over the index vector a, comparing through less(x, y) on the elements (positions of the input)"""

    def __init__(self, n, less, no_heap=False):
        self.a, self.less, self.no_heap, self.fallbacks = list(range(n)), less, no_heap, 0

    def push_heap(self, first, hole, top, value):
        a = self.a
        parent = (hole - 1) // 2
        while hole > top and self.less(a[first + parent], value):
            a[first + hole] = a[first + parent]
            hole = parent
            parent = (hole - 1) // 2
        a[first + hole] = value

    def adjust_heap(self, first, hole, length, value):
        a = self.a
        top = hole
        child = hole
        while child < (length - 1) // 2:
            child = 2 * (child + 1)
            if self.less(a[first + child], a[first + child - 1]):
                child -= 1
            a[first + hole] = a[first + child]
            hole = child
        if length % 2 == 0 and child == (length - 2) // 2:
            child = 2 * (child + 1)
            a[first + hole] = a[first + child - 1]
            hole = child - 1
        self.push_heap(first, hole, top, value)

    def heap_sort(self, first, last):
        """__partial_sort(first, last, last): __make_heap, then __pop_heap from the back"""
        a = self.a
        self.fallbacks += 1
        if self.no_heap:
            a[first:last] = _stable(a[first:last], self.less)
            return
        length = last - first
        if length >= 2:
            parent = (length - 2) // 2
            while True:
                self.adjust_heap(first, parent, length, a[first + parent])
                if parent == 0:
                    break
                parent -= 1
        while last - first > 1:
            last -= 1
            value = a[last]
            a[last] = a[first]
            self.adjust_heap(first, 0, last - first, value)

    def swap(self, i, j):
        self.a[i], self.a[j] = self.a[j], self.a[i]

    def move_median_to_first(self, result, x, y, z):
        a, less = self.a, self.less
        if less(a[x], a[y]):
            if less(a[y], a[z]):
                self.swap(result, y)
            elif less(a[x], a[z]):
                self.swap(result, z)
            else:
                self.swap(result, x)
        elif less(a[x], a[z]):
            self.swap(result, x)
        elif less(a[y], a[z]):
            self.swap(result, z)
        else:
            self.swap(result, y)

    def unguarded_partition(self, first, last, pivot):
        a, less = self.a, self.less
        while True:
            while less(a[first], a[pivot]):
                first += 1
            last -= 1
            while less(a[pivot], a[last]):
                last -= 1
            if not first < last:
                return first
            self.swap(first, last)
            first += 1

    def introsort_loop(self, first, last, depth):
        while last - first > THRESHOLD:
            if depth == 0:
                self.heap_sort(first, last)
                return
            depth -= 1
            mid = first + (last - first) // 2
            self.move_median_to_first(first, first + 1, mid, last - 1)
            cut = self.unguarded_partition(first + 1, last, first)
            self.introsort_loop(cut, last, depth)
            last = cut

    def unguarded_linear_insert(self, last):
        a = self.a
        value = a[last]
        nxt = last - 1
        while self.less(value, a[nxt]):
            a[last] = a[nxt]
            last = nxt
            nxt -= 1
        a[last] = value

    def insertion_sort(self, first, last):
        a = self.a
        for i in range(first + 1, last):
            if self.less(a[i], a[first]):
                value = a[i]
                a[first + 1:i + 1] = a[first:i]
                a[first] = value
            else:
                self.unguarded_linear_insert(i)

    def sort(self):
        n = len(self.a)
        if n == 0:
            return
        self.introsort_loop(0, n, 2 * (n.bit_length() - 1))
        if n > THRESHOLD:
            self.insertion_sort(0, THRESHOLD)
            for i in range(THRESHOLD, n):
                self.unguarded_linear_insert(i)
        else:
            self.insertion_sort(0, n)


def _stable(items, less):
    return sorted(items, key=cmp_to_key(lambda x, y: -1 if less(x, y) else 1 if less(y, x) else 0))   # (sorted() is stable)


def sort_with(n, less, variant=()):
    """(order, fallbacks) of std::sort on n elements under the comparison less(x, y) of two positions of the input"""
    if "stable_sort" in variant:
        return _stable(range(n), less), 0
    s = _Sort(n, less, "no_heap_fallback" in variant)
    s.sort()
    return s.a, s.fallbacks


def std_sort_order(reads, variant=()):
    """The positions of `reads` (a vector in UMI-index order) after libstdc++'s std::sort comparing read counts only -- up to 16 elements
    an insertion sort, hence stable; beyond that introsort -- and how many times the heapsort fallback ran."""
    return sort_with(len(reads), lambda x, y: reads[x] < reads[y], variant)


def killer(n):
    """McIlroy's adversary ("A killer adversary for quicksort", 1999) run against std_sort_order: a permutation of 0 .. n-1, in index
    order, on which the median-of-three partitions stay lopsided until the depth limit is reached.  Every value starts as "gas" (larger
    than anything solid); a comparison of two gas values freezes one of them to the next solid number."""
    gas = n
    val = [gas] * n
    state = {"solid": 0, "candidate": 0}

    def less(x, y):
        if val[x] == gas and val[y] == gas:
            frozen = x if x == state["candidate"] else y
            val[frozen] = state["solid"]
            state["solid"] += 1
        if val[x] == gas:
            state["candidate"] = x
        elif val[y] == gas:
            state["candidate"] = y
        return val[x] < val[y]

    sort_with(n, less)
    for x in range(n):                                         # what never met another gas value is larger than everything else
        if val[x] == gas:
            val[x] = state["solid"]
            state["solid"] += 1
    assert sorted(val) == list(range(n))
    return val


# ---- distances ------------------------------------------------------------------------------------------------------------------
def edit_distance(a, b, max_ed):
    """Tools::edit_distance for N-free strings: a column of the Levenshtein table is updated inside the band [j - max_ed, j + max_ed] only
    -- the cell under the band is set to j, the cell above it keeps what an earlier column left there (stale) -- and the function returns
    early with a lower bound once every cell of a column, plus its distance from the diagonal, exceeds max_ed."""
    la, lb = len(a), len(b)
    column = list(range(la + 1))
    for j in range(1, lb + 1):
        lower, upper = max(0, j - max_ed), min(la, j + max_ed)
        last_diag = column[lower]
        column[lower] = j
        best = j
        for i in range(lower + 1, upper + 1):
            old_diag = column[i]
            v = min(column[i] + 1, column[i - 1] + 1, last_diag + (a[i - 1] != b[j - 1]))
            best = min(best, v + abs(i - j))
            column[i] = v
            last_diag = old_diag
        if best > max_ed:
            return best
    return column[la]


def levenshtein(a, b):
    row = list(range(len(a) + 1))
    for j in range(1, len(b) + 1):
        new = [j]
        for i in range(1, len(a) + 1):
            new.append(min(row[i] + 1, new[i - 1] + 1, row[i - 1] + (a[i - 1] != b[j - 1])))
        row = new
    return row[len(a)]


def hamming(a, b):
    return sum(x != y for x, y in zip(a, b))


# ---- find_target / find_targets -------------------------------------------------------------------------------------------------
def _find_target(s, v, mult, max_ed, variant):
    """find_target (:83-116) of the UMI at sorted position s: from the most-read UMI downwards, while reads(s) * mult <= reads(d)"""
    seq, reads = v[s]
    target, min_ed = None, None
    for d in range(len(v) - 1, s, -1):
        scaled = reads * mult                                               # double arithmetic: 50 * 1.1 is 55.00000000000001
        if scaled >= v[d][1] if "mult_ge" in variant else scaled > v[d][1]:
            break
        ed = hamming(seq, v[d][0]) if "hamming" in variant else edit_distance(seq, v[d][0], max_ed)
        if ed > max_ed:
            continue
        if min_ed is None or (ed <= min_ed if "ed_le" in variant else ed < min_ed):
            target = v[d][0]
            if ed <= 1:
                break
            min_ed = ed
    return target


def _find_target_by_lookup(s, v, position, mult):
    """The same answer at max_ed = 1, where a hit ends the search: the highest position within the multiplier's reach that holds a
    Hamming-1 neighbour (two strings of one length are one edit apart exactly if they differ in one base).  Groups of thousands of UMIs
    only; test_directional_model_cpu.py holds it against _find_target and, on the large groups, against the oracle."""
    seq, reads = v[s]
    best = s
    for i in range(len(seq)):
        for base in "ACGT":
            if base != seq[i]:
                d = position.get(seq[:i] + base + seq[i + 1:], -1)
                if d > best and not reads * mult > v[d][1]:
                    best = d
    return v[best][0] if best > s else None


def find_targets(umis, mult, max_ed, variant=(), by_lookup=None):
    """find_targets (:55-81) of one (cell, gene) group: `umis` is [(sequence, reads)] in UMI-index order; returns {source: target} after
    the chain shortening.  Raises on an N and on sequences of several lengths."""
    if any("N" in s for s, _ in umis):
        raise ValueError("a group with an N-UMI is decided with rand(): not the model's")
    if len({len(s) for s, _ in umis}) > 1:
        raise ValueError("UMIs of several lengths: the banded distance is no Levenshtein distance there, not the model's")
    assert len({s for s, _ in umis}) == len(umis)
    order, _ = std_sort_order([r for _, r in umis], variant)
    v = [umis[i] for i in order]
    if by_lookup is None:
        by_lookup = len(v) >= FAST_FROM and max_ed == 1 and not set(variant) - {"stable_sort", "no_heap_fallback", "no_chain"}
    assert not by_lookup or max_ed == 1
    position = {s: i for i, (s, _) in enumerate(v)} if by_lookup else None
    out = {}
    for s in range(len(v)):
        t = _find_target_by_lookup(s, v, position, mult) if by_lookup else _find_target(s, v, mult, max_ed, variant)
        if t is not None:
            out[v[s][0]] = t
    if "no_chain" not in variant:
        for s in range(len(v) - 1, -1, -1):                                  # (:66-78) once, from the most-read UMI downwards
            t = out.get(v[s][0])
            if t is not None and t in out:
                out[v[s][0]] = out[t]
    return out


# ---- a whole stream -------------------------------------------------------------------------------------------------------------
Result = namedtuple("Result", "targets molecules removed total_umis stream")
Stream = namedtuple("Stream", "cells genes molecules groups")


def first_seen(values):
    ids = {}
    for x in values:
        ids.setdefault(x, len(ids))
    return ids


def stream_of(case, variant=(), seen_by=None):
    """What the container holds before the correction: case.reads is [(barcode, gene or None, UMI)] in stream order.
      cells, genes  {barcode: id}, {gene: id} by first occurrence (cells over all reads, genes over gene-bearing reads)
      molecules     {(cell, gene, umi): reads} of the gene-bearing reads
      groups        {(cell, gene): [(sequence, reads)]} of the real cells -- those with at least case.min_genes genes -- in UMI-index order:
                    the order of the UMIs' first occurrences among the gene-bearing reads of the WHOLE stream (StringIndexer)
    seen_by (positions of reads) is another way to be wrong: first occurrences taken among those reads only -- what a shard of a sharded run
    knows by itself -- and the UMIs they lack behind them."""
    cells = first_seen(b for b, _, _ in case.reads)
    genes = first_seen(g for _, g, _ in case.reads if g is not None)
    known = [case.reads[i] for i in sorted(seen_by)] if seen_by is not None else []
    index = first_seen(u for _, g, u in known + case.reads if g is not None or "geneless_indexed" in variant)
    local = first_seen((cells[b], genes[g], u) for b, g, u in case.reads if g is not None)
    molecules = {}
    for b, g, u in case.reads:
        if g is not None:
            key = (cells[b], genes[g], u)
            molecules[key] = molecules.get(key, 0) + 1
    by_group = {}
    for (c, g, u), r in molecules.items():
        by_group.setdefault((c, g), []).append((u, r))
    n_genes = {}
    for c, g in by_group:
        n_genes[c] = n_genes.get(c, 0) + 1
    groups = {}
    for (c, g), umis in sorted(by_group.items()):
        if n_genes[c] >= case.min_genes:
            groups[c, g] = sorted(umis, key=(lambda x: local[c, g, x[0]]) if "local_index" in variant else (lambda x: index[x[0]]))
    return Stream(cells, genes, molecules, groups)


def run(case, variant=(), seen_by=None):
    """The correction over a whole stream (case.reads, case.mult, case.max_ed, case.min_genes):
      targets     {(cell, gene): {source: target}} of the groups that re-key something
      molecules   {(cell, gene, umi): reads} after the fold
      removed     {cell: decrement of total_umis}, one per re-keyed UMI (Cell::merge_umis)
      total_umis  {cell: molecules before the correction - removed}"""
    st = stream_of(case, variant, seen_by)
    molecules = dict(st.molecules)
    targets, removed = {}, {}
    for (c, g), umis in st.groups.items():
        t = find_targets(umis, case.mult, case.max_ed, variant)
        if not t:
            continue
        targets[c, g] = t
        for src in t:
            root = t[src]
            while root in t:                                                 # (only without the chain shortening)
                root = t[root]
            molecules[c, g, root] += molecules.pop((c, g, src))
            removed[c] = removed.get(c, 0) + 1
    total = {c: 0 for c in st.cells.values()}
    for c, _, _ in st.molecules:
        total[c] += 1
    return Result(targets, molecules, removed, {c: n - removed.get(c, 0) for c, n in total.items()}, st)


def written_umis(case, result):
    """Per read, the UMI it is written under once corrected (-F): its group's target, or its own; None for a read without a gene and for
    one of a cell with fewer than case.min_genes genes (min_genes serves as both thresholds of the container)."""
    st = result.stream
    out = []
    for b, g, u in case.reads:
        key = (st.cells[b], st.genes[g]) if g is not None else None
        out.append(result.targets.get(key, {}).get(u, u) if key in st.groups else None)
    return out
