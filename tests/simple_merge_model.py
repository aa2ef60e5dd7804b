"""The reference's barcode merges that run without a whitelist, restated in plain Python for the tests (simple_merge_cases.py,
test_simple_merge_model_cpu.py, test_gpu_simple_merge.py).

Written from the reference's text, one container at a time; it shares nothing with the device code or the oracle: no sorted
tables, no packed barcodes, no bit-parallel distances.  A case is a poisson_cases.ContainerCase: `container` (cell -> gene -> set
of UMIs), `n_genes`, `total_umis`, `barcodes`, and `filtered` in the order of compare_cells.

  common_umigs               SimpleMergeStrategy::get_cells_with_common_umigs (SimpleMergeStrategy.cpp:16-40)
  simple_target              SimpleMergeStrategy::get_merge_target (:47-86) in exact rationals.  The reference walks an unordered
                             container, so what it returns can hang on the order: the answer is the SET of cells it can return
  poisson_simple_neighbours  the neighbour list of PoissonSimpleMergeStrategy::get_merge_target (PoissonSimpleMergeStrategy.cpp:15-43)
  banded_edit_distance       Tools::edit_distance(s1, s2, skip_n, max_ed) (Tools/UtilFunctions.cpp:32-65), line by line
  merge_all_target           MergeAllMergeStrategy::get_merge_target (MergeAllMergeStrategy.h:16-50)
  final_targets              MergeStrategyBase::merge_inited's second loop over the targets of the filtered cells
"""
from fractions import Fraction
from itertools import permutations

import poisson_model as pm
import whitelist_model as wm

EPS = Fraction(0.00001)            # SimpleMergeStrategy::EPS, the double itself
MARGIN = Fraction(1, 10 ** 9)      # a compared difference nearer than this to its boundary: the reference's doubles could fall either way
LITERAL_MAX = 6                    # up to this many admissible candidates the loop is run over every order


class TooClose(ArithmeticError):
    """a comparison of the reference lies within MARGIN of its boundary: the model does not answer"""


class Answer:
    """targets: the cells get_merge_target can return, or None where the model cannot tell (undecided)"""

    def __init__(self, targets, fractions):
        self.targets, self.fractions = (None if targets is None else frozenset(targets)), fractions

    @property
    def decided(self):
        return self.targets is not None and len(self.targets) == 1

    @property
    def target(self):
        assert self.decided
        return next(iter(self.targets))


def _above(x, boundary, exact_ok=False):
    """x > boundary, refusing the neighbourhood of the boundary (exact equality passes where both sides are exact in double)"""
    d = x - boundary
    if abs(d) < MARGIN and not (exact_ok and d == 0):
        raise TooClose("%s against %s" % (float(x), float(boundary)))
    return d > 0


def umig_index(case):
    """SimpleMergeStrategy::init (:88-102): (UMI, gene) -> the filtered cells that hold it"""
    index = getattr(case, "_umig_index", None)
    if index is None:
        index = {}
        for cell in case.filtered:
            for gene, umis in case.container[cell].items():
                for umi in umis:
                    index.setdefault((umi, gene), []).append(cell)
        case._umig_index = index
    return index


def common_umigs(case, base):
    """{other: number of UMI-genes of `base` that `other` holds too}; other is filtered, not the base, and has at least as many genes"""
    index = umig_index(case)
    common = {}
    for gene, umis in case.container[base].items():
        for umi in umis:
            for other in index.get((umi, gene), ()):          # (a base that is not filtered has UMI-genes outside the index)
                if other == base:
                    continue
                if case.n_genes[other] >= case.n_genes[base]:
                    common[other] = common.get(other, 0) + 1
    return common


def distance(case, a, b):
    """Tools::edit_distance of two cells' barcodes with its default arguments (kept per case: every pair is asked for from both sides)"""
    memo = case.__dict__.setdefault("_distances", {})
    key = (a, b) if a < b else (b, a)
    if key not in memo:
        memo[key] = wm.edit_distance(case.barcodes[key[0]], case.barcodes[key[1]])
    return memo[key]


def fraction_of(case, base, other, shared):
    return Fraction(shared, 2) * (Fraction(1, case.total_umis[base]) + Fraction(1, case.total_umis[other]))


def _power_of_two(n):
    return n > 0 and n & (n - 1) == 0


def _walk(case, base, order, fractions):
    """the loop of :53-80 over the admissible candidates in one order -> (top cell, top fraction)"""
    top, top_fraction, top_genes = -1, Fraction(-1), -1
    for cell in order:
        d = fractions[cell] - top_fraction
        if _above(d, EPS) or (_above(d, -EPS) and not _above(d, EPS) and case.n_genes[cell] > top_genes):
            top, top_fraction, top_genes = cell, fractions[cell], case.n_genes[cell]
    return top, top_fraction


def simple_target(case, base, max_ed, min_fraction):
    """Answer of SimpleMergeStrategy::get_merge_target.  A candidate beyond the edit distance never changes the loop's state (:67-71), so the
    loop runs over the admissible ones (distance < max_ed) alone."""
    common = common_umigs(case, base)
    admissible = sorted(c for c in common if distance(case, base, c) < max_ed)
    fractions = {c: fraction_of(case, base, c, common[c]) for c in admissible}
    min_fraction = Fraction(min_fraction)

    def closing(top, top_fraction):                            # :82-85
        exact = top >= 0 and _power_of_two(case.total_umis[base]) and _power_of_two(case.total_umis[top])
        return top if _above(top_fraction, min_fraction, exact) or top_fraction == min_fraction else base

    if len(admissible) <= LITERAL_MAX:
        return Answer({closing(*_walk(case, base, order, fractions)) for order in permutations(admissible)}, fractions)
    # more candidates: only what can be proved from the loop.  A candidate more than EPS above all others is taken when it is met and
    # never given up.  So is, of a group of exactly equal best fractions with everybody else more than EPS below, the one member with the
    # most genes: outsiders never replace a member, and among members only a larger gene count replaces.
    best = max(fractions.values())
    group = [c for c in admissible if fractions[c] == best]
    if all(_above(best - fractions[c], EPS) for c in admissible if c not in group):
        most = max(case.n_genes[c] for c in group)
        winners = [c for c in group if case.n_genes[c] == most]
        if len(winners) == 1:
            return Answer({closing(winners[0], best)}, fractions)
    return Answer(None, fractions)


def poisson_simple_neighbours(case, base, max_ed):
    """the cells with common UMI-genes within the edit distance (<=, where Simple has <), in the filtered order (the reference's own
    order is an unordered_map's)"""
    common = common_umigs(case, base)
    return [c for c in case.filtered if c in common and distance(case, base, c) <= max_ed]


def banded_edit_distance(s1, s2, skip_n, max_ed):
    """Tools::edit_distance, line by line: the row minimum's early return, and the cells outside the band that keep what an earlier row
    left in them.  The reference's column is a C array; where it would be read beyond its end the model refuses."""
    s1len, s2len = len(s1), len(s2)
    column = list(range(s1len + 1))
    for s2_ind in range(1, s2len + 1):
        lower_index = max(0, s2_ind - max_ed)
        upper_index = min(s1len, s2_ind + max_ed)
        if lower_index > s1len:
            raise IndexError("the reference reads beyond its column")
        lastdiag = column[lower_index]
        column[lower_index] = s2_ind
        min_ed = s2_ind
        for s1_ind in range(lower_index + 1, upper_index + 1):
            olddiag = column[s1_ind]
            is_match = s1[s1_ind - 1] == s2[s2_ind - 1] or (skip_n and (s1[s1_ind - 1] == "N" or s2[s2_ind - 1] == "N"))
            new_ed = min(column[s1_ind] + 1, column[s1_ind - 1] + 1, lastdiag + (0 if is_match else 1))
            min_ed = min(min_ed, new_ed + abs(s1_ind - s2_ind))
            column[s1_ind] = new_ed
            lastdiag = olddiag
        if min_ed > max_ed:
            return min_ed
    return column[s1len]


def merge_all_target(case, base, max_ed):
    """the nearest filtered cell with more UMIs; of several the one with the most UMIs, of those the first in the filtered order"""
    min_ed, max_umi_num, target = None, 0, None
    for cell in case.filtered:
        target_umi_num = case.total_umis[cell]
        if target_umi_num <= case.total_umis[base]:
            continue
        ed = banded_edit_distance(case.barcodes[base], case.barcodes[cell], False, max_ed)
        if ed > max_ed:
            continue
        if min_ed is None or min_ed > ed:
            min_ed, max_umi_num, target = ed, target_umi_num, cell
        elif min_ed == ed and max_umi_num < target_umi_num:
            max_umi_num, target = target_umi_num, cell
    return base if target is None else target


def final_targets(case, targets):
    """merge_targets() after the merge; targets: {filtered cell: its get_merge_target}"""
    return pm.merge_targets(len(case.barcodes), case.filtered, [targets[c] for c in case.filtered])[0]
