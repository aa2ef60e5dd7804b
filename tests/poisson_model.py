"""The -M estimator (Tools::CollisionsAdjuster + Estimation::Merge::PoissonTargetEstimator) in exact arithmetic, for the tests
(poisson_cases.py, test_poisson_model_cpu.py, test_gpu_poisson_estimator.py).

Plain Python on decimal.Decimal at PRECISION digits.  Every probability that enters is the double the reference and the device
work on (count / total rounded once), converted exactly; from there on nothing is rounded to double again, so against a double
evaluation (2^-53 = 1.1e-16 per operation) the results below are exact.  The order of a sum does not matter here, so UMIs that
were seen equally often are summed as one class (probability x how many): that is what makes 65 537 UMIs affordable.

  umi_distribution      CellsDataContainer::umi_distribution: molecules per UMI over the filtered cells' genes.
  adjusted_sizes        CollisionsAdjuster::update_adjusted_sizes: for s = 1, 2, ...: the total size is s plus the whole collisions
                        so far; every UMI's chance of not having been drawn goes down by (1 - p) per drawn molecule; the chance that
                        the next molecule repeats a UMI is new_prob = SUM p (1 - not drawn); 1 / (1 - new_prob) - 1 more collisions
                        are expected; the adjusted size is s plus the collisions, rounded half away from zero (lround).
  gene_intersection     estimate_genes_intersection_size: SUM over UMIs of (1 - (1-p)^a1) (1 - (1-p)^a2) for the ADJUSTED sizes.
  expected_intersection estimate_intersection_prob's loop: the sum of gene_intersection over the genes the two cells share.
  upper_tail            Rcpp::ppois(k - 1, lam, lower = false) = P(X >= k), X ~ Poisson(lam).
  intersection_prob     estimate_intersection_prob: an empty intersection gives expected -1 and probability 1.
  best_target           get_best_merge_target.
  merge_targets         MergeStrategyBase::merge_inited's second loop on the targets of the filtered cells.
"""
from collections import Counter
from decimal import Context, Decimal, localcontext, MAX_EMAX, MIN_EMIN, ROUND_FLOOR, ROUND_HALF_UP

PRECISION = 80
MIN_NORMAL = Decimal(2) ** -1022              # below it a double keeps an absolute precision (2^-1074), not a relative one
HALF = Decimal("0.5")
TOTAL_LIMIT = 1 << 32


class CollisionsDiverged(ArithmeticError):
    """The recurrence left its domain at entry `at` (1-based): nothing is left of 1 - new_prob, or the total size of the next
    step passes 2^32.  `table` and `margins` hold the entries before it."""

    def __init__(self, at, table, margins):
        super().__init__("collisions adjustment diverged at size %d" % at)
        self.at, self.table, self.margins = at, table, margins


def _ctx():
    return localcontext(Context(prec=PRECISION, Emax=MAX_EMAX, Emin=MIN_EMIN))


def exact(x):
    """a double (or int, or Decimal) as the number it is"""
    return x if isinstance(x, Decimal) else Decimal(x)


def classes_of(probs):
    """[(probability, how many UMIs have it)], ascending"""
    return sorted(Counter(exact(p) for p in probs).items())


def probabilities(counts):
    """PoissonTargetEstimator::init: count / sum, one rounding to double each"""
    total = sum(int(c) for c in counts)
    return [int(c) / total for c in counts]                       # int / int is correctly rounded, as double(c) / double(total) is


def _classes(probs):
    """probs: doubles, or classes_of(...) already"""
    probs = list(probs)
    return probs if probs and isinstance(probs[0], tuple) else classes_of(probs)


def adjusted_sizes(probs, max_expression):
    """-> (table, margins): table[s - 1] the adjusted size of s; margins[s - 1] = (distance of sum_collisions to the nearest
    integer, distance of s + sum_collisions to the nearest half) -- how far the two roundings of step s are from tipping over.
    Raises CollisionsDiverged."""
    with _ctx():
        cls = _classes(probs)
        q = [1 - p for p, _ in cls]
        not_drawn = [Decimal(1)] * len(cls)
        sum_collisions, last_total = Decimal(0), 0
        table, margins = [], []
        for s in range(1, max_expression + 1):
            total = s + int(sum_collisions.to_integral_value(ROUND_FLOOR))
            delta = total - last_total
            last_total = total
            new_prob = Decimal(0)
            for i, (p, m) in enumerate(cls):
                not_drawn[i] *= q[i] ** delta
                new_prob += m * (p * (1 - not_drawn[i]))
            left = 1 - new_prob
            if not left > 0:
                raise CollisionsDiverged(s, table, margins)
            sum_collisions += 1 / left - 1
            if s + 1 + int(sum_collisions.to_integral_value(ROUND_FLOOR)) > TOTAL_LIMIT:
                raise CollisionsDiverged(s, table, margins)
            value = s + sum_collisions
            table.append(int(value.to_integral_value(ROUND_HALF_UP)))         # value > 0: half up is half away from zero
            to_integer = abs(sum_collisions - sum_collisions.to_integral_value(ROUND_HALF_UP))
            to_half = abs(abs(value - value.to_integral_value(ROUND_FLOOR)) - HALF)
            margins.append((to_integer, to_half))
        return table, margins


def gene_intersection(probs, a1, a2):
    """est(a1, a2) for ADJUSTED sizes"""
    with _ctx():
        cls = _classes(probs)
        if a1 > a2:
            a1, a2 = a2, a1
        out = Decimal(0)
        for p, m in cls:
            q = 1 - p
            low = q ** a1
            out += m * ((1 - low) * (1 - low * q ** (a2 - a1)))
        return out


def upper_tail(k, lam):
    """P(X >= k), X ~ Poisson(lam).  The terms t(j) = e^-lam lam^j / j! follow from t(j + 1) = t(j) lam / (j + 1); for k above lam
    the tail itself is summed, else the k terms below it are and taken from 1 (the smaller side, so nothing cancels)."""
    with _ctx():
        lam = exact(lam)
        if k <= 0:
            return Decimal(1)
        if not lam > 0:
            return Decimal(0)
        t = (-lam).exp()
        if k > lam:
            for j in range(1, k + 1):
                t = t * lam / j
            total, j = t, k
            eps = Decimal(10) ** -(PRECISION + 5)
            while True:
                j += 1
                t = t * lam / j
                total += t
                if t <= total * eps:
                    return total
        below = t
        for j in range(1, k):
            t = t * lam / j
            below += t
        return 1 - below


def relative_deviation(got, want):
    """|got - want| / want for a double `got` and an exact `want` >= 0; below the normal range of double (where it keeps an
    absolute precision) the scale is the smallest normal number, so a result that underflowed to 0 deviates by next to nothing"""
    with _ctx():
        return abs(exact(got) - want) / max(abs(want), MIN_NORMAL)


def umi_distribution(container, filtered):
    """container: {cell: {gene: set(umi)}} -> Counter umi -> molecules over the filtered cells"""
    out = Counter()
    for cell in filtered:
        for umis in container.get(cell, {}).values():
            out.update(umis)
    return out


def intersection_size(container, c1, c2):
    g1, g2 = container.get(c1, {}), container.get(c2, {})
    return sum(len(u & g2[g]) for g, u in g1.items() if g in g2)


class Estimator:
    """PoissonTargetEstimator after init(container.umi_distribution())."""

    def __init__(self, container, filtered):
        self.container = container
        self.distribution = umi_distribution(container, filtered)
        self.classes = classes_of(probabilities(self.distribution.values())) if self.distribution else []
        self.max_size = max((len(u) for genes in container.values() for u in genes.values()), default=0)
        self.table, self.margins = adjusted_sizes(self.classes, self.max_size) if self.distribution else ([], [])
        self._est = {}

    def adjusted(self, size):
        return self.table[size - 1]

    def gene_intersection(self, size1, size2):
        """for RAW sizes"""
        key = tuple(sorted((self.adjusted(size1), self.adjusted(size2))))
        if key not in self._est:
            self._est[key] = gene_intersection(self.classes, *key)
        return self._est[key]

    def common_genes(self, c1, c2):
        g1, g2 = self.container.get(c1, {}), self.container.get(c2, {})
        return sorted(g for g in g1 if g in g2)

    def expected_intersection(self, c1, c2):
        with _ctx():
            g1, g2 = self.container[c1], self.container[c2]
            return sum((self.gene_intersection(len(g1[g]), len(g2[g])) for g in self.common_genes(c1, c2)), Decimal(0))

    def intersection_prob(self, c1, c2):
        """-> (intersection size, expected, probability); expected and probability exact, or -1 and 1"""
        n = intersection_size(self.container, c1, c2)
        if n == 0:
            return 0, Decimal(-1), Decimal(1)
        expected = self.expected_intersection(c1, c2)
        return n, expected, upper_tail(n, expected)


class Decision:
    """target: what get_best_merge_target returns.  margin: the smallest relative distance that the decision hangs on -- of the
    smallest probability to its limit, and, where that probability is accepted, to the next larger one; 0 when the answer
    hangs on an order that is not known.  Neighbours whose probabilities are exactly equal (same genes, same sizes, same
    intersection) do not enter the margin otherwise: the first of them in the reference's order wins."""

    def __init__(self, target, margin, limit, probs):
        self.target, self.margin, self.limit, self.probs = target, margin, limit, probs


def best_target(estimator, base, neighbours, max_merge_prob, max_real_merge_prob, levels=None):
    """neighbours: cells in the reference's order (the base itself may be among them: first, when it is a real barcode).
    levels: where that order is known only level by level (whitelist_model.search), the level of each neighbour; None when the
    order is known throughout."""
    with _ctx():
        base_real = neighbours[0] == base
        limit = exact((max_merge_prob if base_real else max_real_merge_prob) / len(neighbours))     # a double division there too
        levels = list(range(len(neighbours))) if levels is None else levels
        probs = [(estimator.intersection_prob(base, c)[2], c, lv) for c, lv in zip(neighbours, levels) if c != base]
        if not probs:
            return Decision(base if base_real else -1, Decimal(1), limit, probs)                    # min_prob stays 2 > limit
        low = min(p for p, _, _ in probs)
        scale = lambda a, b: abs(a - b) / max(a, b, MIN_NORMAL)
        margin = scale(low, limit)
        if low > limit:
            return Decision(base if base_real else -1, margin, limit, probs)
        tied = [(lv, c) for p, c, lv in probs if p == low]
        first_level = min(lv for lv, _ in tied)
        winners = {c for lv, c in tied if lv == first_level}
        if len(winners) > 1:
            margin = Decimal(0)
        above = [p for p, _, _ in probs if p != low]
        if above:
            margin = min(margin, scale(low, min(above)))
        return Decision(sorted(winners)[0], margin, limit, probs)


def merge_targets(n_cells, filtered, targets):
    """MergeStrategyBase::merge_inited (:29-57) -> (cb_reassign_targets, excluded cells); targets[i] belongs to filtered[i]"""
    reassign = list(range(n_cells))
    moved_to = {}
    excluded = []
    for base, target in zip(filtered, targets):
        if target < 0:
            excluded.append(base)
            continue
        target = reassign[target]
        if target == base:
            continue
        reassign[base] = target
        moved_to.setdefault(target, set()).add(base)
        for other in moved_to.pop(base, ()):
            reassign[other] = target
            moved_to[target].add(other)
    return reassign, excluded
