"""The reference's whitelist neighbour search, restated in plain Python for the tests (whitelist_cases.py,
test_whitelist_model_cpu.py, test_gpu_whitelist_search.py).

It follows the reference's own steps, one list at a time, and shares nothing with the device code: no packed
barcodes, no bit-parallel distances, no neighbour tables.

  whitelist file   BarcodesParser::read_line: whitespace separated tokens, stored reverse-complemented.
                   InDropBarcodesParser: exactly two lines.  ConstLengthBarcodesParser: one part per line, one
                   length per line.
  split_barcode    inDrop: the second part has the length of the second line's first entry, the first part is
                   the rest (possibly empty).  Const length: the lengths of every line's first entry, in turn.
  edit_distance    Tools::edit_distance with its defaults (skip_n, max_ed = 10000: the band is never active).
  combinations     BarcodesParser::get_real_neighbour_cbs: per part the entries sorted by distance, walked depth
                   first in part order; a running distance beyond 5 ends the walk of that list.
  search           RealBarcodesMergeStrategy::get_real_neighbour_cbs (:63-109) and
                   PoissonRealBarcodesMergeStrategy::get_max_merge_dist.
  pairs            what is left of a base's candidates for the target estimators (RealBarcodesMergeStrategy.cpp:34-35,
                   PoissonTargetEstimator.cpp:26-29).
"""

INDROP, CONST = 0, 1
MAX_DIST = 5                      # BarcodesParser::MAX_REAL_MERGE_EDIT_DISTANCE

_COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


class BarcodeLengthError(ValueError):
    """split_barcode refused the barcode; str() is the reference's message where it has one."""


def reverse_complement(s):
    return "".join(_COMPLEMENT[c] for c in reversed(s))


def whitelist_text(parts):
    """The file that loads as `parts`: one line per part, every entry reverse-complemented."""
    return "".join(" ".join(reverse_complement(e) for e in part) + "\n" for part in parts)


def parse_whitelist(text, kind):
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    parts = []
    for line in (lines[:2] if kind == INDROP else lines):
        tokens = line.split()
        if not tokens:
            raise ValueError("File with barcodes has wrong format")
        if kind == CONST and len({len(t) for t in tokens}) != 1:
            raise ValueError("All barcodes in one line must have the same length")
        parts.append([reverse_complement(t) for t in tokens])
    if kind == INDROP and len(parts) != 2:
        raise ValueError("File with barcodes has wrong format")
    if not parts:
        raise ValueError("ERROR: empty barcodes list")
    return parts


def split_barcode(kind, parts, barcode):
    if kind == INDROP:
        l2 = len(parts[1][0])
        if len(barcode) < l2:
            raise BarcodeLengthError("Barcode '%s' is shorter than the second whitelist part" % barcode)
        return [barcode[:len(barcode) - l2], barcode[len(barcode) - l2:]]
    lengths = [len(part[0]) for part in parts]
    if len(barcode) != sum(lengths):
        raise BarcodeLengthError("Barcode '%s' has wrong length (%d expected)" % (barcode, sum(lengths)))
    out, at = [], 0
    for n in lengths:
        out.append(barcode[at:at + n])
        at += n
    return out


def edit_distance(a, b):
    """Levenshtein distance; an N on either side matches anything."""
    column = list(range(len(a) + 1))
    for j in range(1, len(b) + 1):
        diagonal = column[0]
        column[0] = j
        for i in range(1, len(a) + 1):
            match = a[i - 1] == b[j - 1] or a[i - 1] == "N" or b[j - 1] == "N"
            value = min(column[i] + 1, column[i - 1] + 1, diagonal + (0 if match else 1))
            diagonal = column[i]
            column[i] = value
    return column[len(a)]


def part_distances(parts, pieces):
    """per part: [(distance, entry index)] sorted by distance"""
    out = []
    for part, piece in zip(parts, pieces):
        cache = {}
        row = []
        for i, entry in enumerate(part):
            d = cache.get(entry)
            if d is None:
                d = cache[entry] = edit_distance(piece, entry)
            row.append((d, i))
        row.sort()
        out.append(row)
    return out


def combinations(dists):
    """[(total distance, (entry index per part))] of every combination within MAX_DIST, in the walk's order"""
    out = []
    chosen = [0] * len(dists)

    def walk(part, so_far):
        if part == len(dists):
            out.append((so_far, tuple(chosen)))
            return
        for d, i in dists[part]:
            if so_far + d > MAX_DIST:
                return
            chosen[part] = i
            walk(part + 1, so_far + d)

    walk(0, 0)
    return out


class Search:
    """The result for one base.

    candidates   universe indices in the reference's order up to ties of the distance; a multiset
    min_level    smallest total distance of any combination, None when no combination lies within MAX_DIST
    level_found  total distance -> candidates taken at it (only levels that gave one)
    horizon      the largest total distance at which a combination was, or would have been, taken: the last value of
                 max_dist when something was found, MAX_DIST when the scan ran to its end without a candidate
    part_counts  per part: entries at distance 0 .. MAX_DIST
    """

    def __init__(self):
        self.candidates, self.min_level, self.level_found, self.horizon, self.part_counts = [], None, {}, MAX_DIST, []


def search(kind, parts, poisson, min_genes, universe, base):
    """universe: a Universe; base: index of the base cell in it"""
    res = Search()
    dists = part_distances(parts, split_barcode(kind, parts, universe.barcode[base]))
    res.part_counts = [[sum(1 for d, _ in row if d == k) for k in range(MAX_DIST + 1)] for row in dists]
    combos = combinations(dists)
    if not combos:
        return res
    combos.sort(key=lambda c: c[0])                      # stable; the reference's order inside a level is not modelled
    res.min_level = combos[0][0]
    max_dist = res.min_level
    if poisson:
        max_dist = 2 if max_dist == 0 else max_dist + 1
    for ed, picks in combos:
        if ed > max_dist and res.candidates:
            break
        cell = universe.by_barcode.get("".join(parts[p][i] for p, i in enumerate(picks)))
        if cell is not None and universe.n_genes[cell] >= min_genes and universe.total_umis[cell] >= universe.total_umis[base]:
            res.candidates.append(cell)
            res.level_found[ed] = res.level_found.get(ed, 0) + 1
        max_dist = max(max_dist, ed)
    if res.candidates:
        res.horizon = min(max_dist, MAX_DIST)
    return res


class Universe:
    """The cells a search sees: barcode text, gene count and TOTAL_UMIS of each; barcodes are distinct."""

    def __init__(self, barcode, n_genes, total_umis):
        assert len(barcode) == len(n_genes) == len(total_umis)
        self.barcode, self.n_genes, self.total_umis = list(barcode), list(n_genes), list(total_umis)
        self.by_barcode = {b: i for i, b in enumerate(self.barcode)}
        assert len(self.by_barcode) == len(self.barcode), "a barcode occurs twice"

    def __len__(self):
        return len(self.barcode)


def pairs(base, candidates, poisson):
    """The candidates a target estimator compares the base with.  A base that leads its own candidate list is a real
    barcode: RealBarcodesMergeStrategy returns it at once (no pair), the Poisson estimator skips it and goes on."""
    if candidates and candidates[0] == base and not poisson:
        return []
    return [c for c in candidates if c != base]
