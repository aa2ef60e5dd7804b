"""`dropest -S` in plain Python, written from the reference's text, for test_validation_model_cpu.py and test_gpu_validation.py.

  edit_distance    Tools::edit_distance(s1, s2, skip_n, max_ed), Tools/UtilFunctions.cpp:32-65, line by line: ONE column that is a plain
                   array, so a cell outside a row's band keeps what an earlier row left there; a row whose minimum (over the band, each
                   cell plus its distance from the diagonal, and the row number itself) exceeds the band ends the function with that
                   minimum.  Under a narrow band the result is not the Levenshtein distance, and it is what -S tests and records.
  run_validation   MergeProbabilityValidator::run_validation, MergeProbabilityValidator.cpp:8-46, over libc's srand(42) / rand(): two
                   values per candidate, cell1 == cell2 rejected before any distance, the band is min_ed.  The reference never ends when
                   no pair qualifies; `max_draws` caps the candidates tested so that the model does.
  evaluate         the estimator's numbers of the recorded pairs from poisson_model.Estimator (exact).
"""
import ctypes

import poisson_model as pm

_libc = ctypes.CDLL("libc.so.6")
_libc.rand.restype = ctypes.c_int


def edit_distance(s1, s2, skip_n=True, max_ed=10000):
    n1, n2 = len(s1), len(s2)
    column = list(range(n1 + 1))
    for j in range(1, n2 + 1):
        lower, upper = max(0, j - max_ed), min(n1, j + max_ed)
        lastdiag = column[lower]
        column[lower] = j
        min_ed = j
        for i in range(lower + 1, upper + 1):
            olddiag = column[i]
            match = s1[i - 1] == s2[j - 1] or (skip_n and (s1[i - 1] == "N" or s2[j - 1] == "N"))
            new_ed = min(column[i] + 1, column[i - 1] + 1, lastdiag + (0 if match else 1))
            min_ed = min(min_ed, new_ed + abs(i - j))
            column[i] = new_ed
            lastdiag = olddiag
        if min_ed > max_ed:
            return min_ed
    return column[n1]


def levenshtein(s1, s2, skip_n=True):
    """the full table, for the cases that show where the band departs from it"""
    prev = list(range(len(s1) + 1))
    for j in range(1, len(s2) + 1):
        cur = [j]
        for i in range(1, len(s1) + 1):
            match = s1[i - 1] == s2[j - 1] or (skip_n and "N" in (s1[i - 1], s2[j - 1]))
            cur.append(min(prev[i] + 1, cur[i - 1] + 1, prev[i - 1] + (0 if match else 1)))
        prev = cur
    return prev[len(s1)]


class Sample:
    def __init__(self):
        self.cell1, self.cell2, self.edit_distance = [], [], []
        self.draws_used, self.complete = 0, False

    @property
    def n_found(self):
        return len(self.cell1)

    def pairs(self):
        return list(zip(self.cell1, self.cell2))


def run_validation(filtered, barcode_of, min_ed, max_ed, n_pairs, max_draws):
    """filtered: cell ids in filtered_cells() order; barcode_of: cell id -> text.  draws_used: candidates tested up to and including
    the one that gave the last pair of a complete sample; every candidate tested (max_draws) of one that the cap ended."""
    s = Sample()
    f = len(filtered)
    if f == 0 or n_pairs == 0:
        s.complete = n_pairs == 0
        return s
    if f == 1:                                   # (the reference spins on cell1 == cell2; the library returns at once)
        return s
    _libc.srand(42)
    draws = 0
    while s.n_found < n_pairs and draws < max_draws:
        c1 = filtered[_libc.rand() % f]
        c2 = filtered[_libc.rand() % f]
        draws += 1
        if c1 == c2:
            continue
        ed = edit_distance(barcode_of(c1), barcode_of(c2), True, min_ed)
        if min_ed <= ed <= max_ed:
            s.cell1.append(c1); s.cell2.append(c2); s.edit_distance.append(ed)
    s.draws_used = draws
    s.complete = s.n_found == n_pairs
    return s


def evaluate(estimator, pairs):
    """[(intersection size, expected, probability)]: PoissonTargetEstimator::estimate_intersection_prob, exact (-1 and 1 when empty)"""
    cache = {}
    out = []
    for pair in pairs:
        if pair not in cache:
            cache[pair] = estimator.intersection_prob(*pair)
        out.append(cache[pair])
    return out


def container_of(cells, genes, umis):
    """{cell: {gene: set(umi)}} from molecule arrays (Context.molecules())"""
    container = {}
    for c, g, u in zip(cells, genes, umis):
        container.setdefault(int(c), {}).setdefault(int(g), set()).add(int(u))
    return container


def estimator_of(container, filtered):
    """the one estimator of save_validation_stats: tables from the filtered cells (only they are ever paired)"""
    filtered = [int(c) for c in filtered]
    return pm.Estimator({c: container.get(c, {}) for c in filtered}, filtered)
