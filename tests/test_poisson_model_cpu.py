"""Pins the exact model of the -M estimator (poisson_model.py) and proves what poisson_cases.py claims about its cases.  No GPU.

  known answers   the reference's own (Tests/TestEstimationMergeProbs.cpp) at its tolerances
  oracle          on every case the oracle -- the reference's formulas in double, left to right -- gives the model's integer
                  adjuster table, its `expected` and probability to rounding, and its merge targets wherever the model can tell
  tail            the oracle's and the library's Poisson tail on a grid of (k, lambda) against the exact series
  conditions      every committed table keeps 1e-5 from a rounding boundary; no base of a hand-built case is undecidable, at
                  most 2 % of the bases of a random one

The scale D of a case (poisson_cases.oracle_scale) is printed per case: run with -s to see it."""
import math
import os

import numpy as np
import pytest

from dropest_amd import capi
from oracle import binding as ob

import poisson_cases as pc
import poisson_model as pm
import whitelist_model as wm
from poisson_model import Decimal

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dropest_amd", "data", "barcodes")
TABLE_MARGIN = Decimal("1e-5")
U = 2.0 ** -53


# ---- known answers ----------------------------------------------------------------------------------------------------------
def reference_fixture():
    from test_gpu_parity import POISSON_FIXTURE
    cells, genes, umis = {}, {}, {}
    container = {}
    for cb, umi, gene in POISSON_FIXTURE:
        c, g = cells.setdefault(cb, len(cells)), genes.setdefault(gene, len(genes))
        container.setdefault(c, {}).setdefault(g, set()).add(umis.setdefault(umi, len(umis)))
    return list(cells), container


def test_reference_known_answers():
    """testPoissonMergeInit (:93-111), testPoissonMergeProbs (:127-134) and testPoissonMergeRejections (:136-140).  The fourth
    probability, (5, 6), and testIntersectionSizeEstimation's values are not what the reference's code computes (see
    test_oracle_reference_kat.py, where they are kept as strict expected failures): the model gives the code's 0.105 there."""
    barcodes, container = reference_fixture()
    n = len(barcodes)
    e = pm.Estimator(container, list(range(n)))                                       # min_genes_before_merge = 0: every cell
    assert len(e.distribution) == 8 and len(container[5]) == 2 and len(container[6]) == 2
    assert e.intersection_prob(0, 1) == (0, Decimal(-1), Decimal(1))
    assert abs(e.intersection_prob(1, 2)[2] - Decimal("0.16")) <= Decimal("0.05")
    assert abs(e.intersection_prob(3, 4)[2] - Decimal("0.15")) <= Decimal("0.05")
    assert Decimal("0.04") <= e.intersection_prob(5, 6)[2] <= Decimal("0.12")
    assert e.gene_intersection(1, 3) == e.gene_intersection(3, 1)
    parts = wm.parse_whitelist(open(os.path.join(DATA, "test_est")).read(), wm.INDROP)
    n_genes = [len(container[c]) for c in range(n)]
    total = [sum(len(u) for u in container[c].values()) for c in range(n)]
    s = wm.search(wm.INDROP, parts, True, 0, wm.Universe(barcodes, n_genes, total), 7)
    target = pm.best_target(e, 7, s.candidates, 1e-4, 1e-7).target if s.candidates else -1
    assert target == -1


def test_model_equals_the_oracle_on_the_reference_fixture():
    from oracle import Oracle
    barcodes, container = reference_fixture()
    from test_oracle_reference_kat import _poisson_fixture
    o = _poisson_fixture()
    o.poisson_init()
    e = pm.Estimator(container, list(range(len(barcodes))))
    for i in range(len(barcodes)):
        for j in range(len(barcodes)):
            if i != j:
                n, expected, prob = e.intersection_prob(i, j)
                assert pm.relative_deviation(o.poisson_intersection_prob(i, j), prob) < 1e-13
                assert n == 0 or pm.relative_deviation(o.poisson_expected_intersection(i, j), expected) < 1e-14


# ---- the adjuster table -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.ADJUSTER_NAMES)
def test_adjuster_table_equals_the_oracle_and_keeps_its_margin(name):
    c = pc.adjuster_case(name)
    table, margins, diverged_at = c.model()
    good = len(table)
    assert (diverged_at is None and good == c.max_expression) or good == diverged_at - 1
    if good:
        assert list(ob.collisions_table(np.array(c.probs), good)) == table
        assert min(min(m) for m in margins) >= TABLE_MARGIN, (name, float(min(min(m) for m in margins)))
    assert all(b > a for a, b in zip(table, table[1:]))


def test_adjuster_cases_reach_their_edges():
    assert {len(pc.adjuster_case(n).counts) for n in pc.ADJUSTER_NAMES} >= {1, 63, 64, 65, 255, 256, 257, 65535, 65536, 65537, 131073}
    table, _, at = pc.adjuster_case("adj_16_diverges").model()
    assert at == 19 and table[-1] == 423                       # 16 equally likely UMIs: 18 good entries, then the total passes 2^32
    # floor(sum_collisions) steps by more than 1 somewhere: the exponent of a step is larger than 2
    table, _, at = pc.adjuster_case("adj_40_steps").model()
    assert at is None and max(b - a for a, b in zip(table, table[1:])) >= 3
    # one distribution in three orders: one table
    tables = [pc.adjuster_case("adj_257_distinct_%s" % o).model()[0] for o in ("random", "ascending", "descending")]
    assert tables[0] == tables[1] == tables[2]
    for n in pc.ADJUSTER_NAMES:
        c = pc.adjuster_case(n)
        assert c.max_expression <= (300 if len(c.counts) <= 1000 else 20)


def test_adjuster_entry_without_umis_or_sizes():
    """n = 0: nothing can collide, adjusted_size[s - 1] = s (the reference's loop over no UMI leaves new_prob = 0); max_expression = 0:
    nothing is written.  Neither touches a device, so both answer on a machine without one."""
    assert list(capi.collisions_adjusted_sizes(np.zeros(0), 7)) == [1, 2, 3, 4, 5, 6, 7] == pm.adjusted_sizes([], 7)[0]
    assert list(ob.collisions_table(np.zeros(0), 7)) == [1, 2, 3, 4, 5, 6, 7]
    assert len(capi.collisions_adjusted_sizes(np.array([0.5, 0.5]), 0)) == 0 and len(capi.collisions_adjusted_sizes(np.zeros(0), 0)) == 0


# ---- containers: expected, probability, decisions ---------------------------------------------------------------------------
def expected_cap(c):
    """What a double evaluation of the reference's formulas may lose on `expected`, relative: 1 - p is rounded once (u, relative
    to 1), which is u / p relative to p, and 1 - (1 - p)^a ~ a p inherits it; two such factors per term, then a sum of n terms
    and the powers' own multiplications.  With p >= 1 / total: (4 total + 2 n + 64) u, doubled for slack."""
    e = c.estimator()
    return 2 * (4 * sum(e.distribution.values()) + 2 * len(e.distribution) + 64) * U


@pytest.mark.parametrize("name", pc.CONTAINER_NAMES)
def test_expected_and_probability_equal_the_oracle(name):
    c = pc.case(name)
    o = pc.oracle_of(c)
    names, counts = o.umi_distribution()
    e = c.estimator()
    assert sorted(int(x) for x in counts) == sorted(e.distribution.values())
    assert {pc.pack(t) & ((1 << 2 * c.umi_len) - 1): int(k) for t, k in zip(names, counts)} == dict(e.distribution)
    assert [int(x) for x in o.filtered_cells()] == c.filtered
    assert min(min(m) for m in e.margins) >= TABLE_MARGIN
    for (a, b), (n, expected, prob) in zip(c.pairs, c.pair_results()):
        if n == 0:
            assert o.poisson_expected_intersection(a, b) == -1 and o.poisson_intersection_prob(a, b) == 1
    d_expected, d_prob = pc.oracle_scale(c, o)
    print("%-24s D(expected) = %.3g  D(probability) = %.3g" % (name, d_expected, d_prob))
    assert d_expected <= expected_cap(c), (float(d_expected), expected_cap(c))
    # the tail turns a relative error of lambda into (k - lambda) times as much, and adds its own: exp() of an argument of
    # magnitude lambda + k ln(lambda) + lgamma(k), each term rounded
    worst = max((abs(n - float(ex)) + 1 for n, ex, _ in c.pair_results() if n), default=1)
    size = max((float(ex) + n * abs(math.log(float(ex))) + math.lgamma(n + 1) for n, ex, _ in c.pair_results() if n), default=1)
    assert d_prob <= worst * expected_cap(c) + 8 * U * size + 64 * U, (float(d_prob), worst, size)


def test_cases_reach_their_edges():
    for name, n in pc.CLASS_COUNTS.items():
        assert pc.case(name).n_classes == n, name
    c = pc.case("multiplicity_thousands")
    assert min(m for _, m in c.estimator().classes) >= 1000
    for name in pc.CLASS_COUNTS:                                           # UMIs of 8 bases or more, and the table did not diverge
        assert pc.case(name).umi_len >= 8 and len(pc.case(name).estimator().table) == pc.case(name).estimator().max_size
    t = pc.case("tail_regimes")
    r = dict(zip(t.pairs, t.pair_results()))
    assert r[0, 1][0] == 1 and r[0, 1][1] > 10 and r[0, 1][2] > Decimal("0.9999")
    assert r[2, 3][2] < Decimal("1e-100") and r[2, 3][2] > pm.MIN_NORMAL
    assert r[4, 5][2] < Decimal(2) ** -1075 and float(r[4, 5][2]) == 0.0       # rounds to 0 in double
    near = [r[6, 7], r[8, 9], r[10, 11]]
    assert [n for n, _, _ in near] == list(pc.TAIL_OVERLAPS)
    assert all(abs(ex - n) < 2 for n, ex, _ in near) and sum(abs(ex - n) <= 1 for n, ex, _ in near) >= 2
    assert {bool(ex < n + 1) for n, ex, _ in near} == {True, False}          # both branches of the library's tail
    for name in pc.CONTAINER_NAMES:
        assert len(pc.case(name).pairs) <= 40 and len(pc.case(name).molecules) <= 200000
    for seed in pc.RANDOM_SEEDS:
        c = pc.case("random_%d" % seed)
        assert len(c.barcodes) <= 40 and len({g for _, g, _ in c.molecules}) <= 61 and 5 <= c.umi_len <= 8 and len(c.molecules) <= 30000
    assert {pc.case("random_%d" % s).umi_len for s in pc.RANDOM_SEEDS} == {5, 6, 7, 8}


def undecidable(c, kind, thresholds, d_prob):
    t = pc.threshold_of(d_prob)
    return [b for b, d in c.decisions(kind, thresholds).items() if d.margin < t]


@pytest.mark.parametrize("kind", [pc.MERGE_POISSON_REAL, pc.MERGE_POISSON_SIMPLE], ids=["real", "simple"])
@pytest.mark.parametrize("name", pc.DECISION_NAMES)
def test_merge_targets_equal_the_oracle(name, kind, tmp_path):
    c = pc.case(name)
    path = pc.write_whitelist(c, tmp_path)
    for thresholds in c.thresholds:
        o = pc.oracle_of(c, kind, thresholds, path)
        _, d_prob = pc.oracle_scale(c, o)
        skipped = undecidable(c, kind, thresholds, d_prob)
        print("%-12s kind %d thresholds %s: %d bases, %d undecidable (T = %.3g)" % (name, kind, thresholds, len(c.filtered), len(skipped),
                                                                                     pc.threshold_of(d_prob)))
        if c.hand_built:
            assert not skipped, skipped
        else:
            assert len(skipped) <= 0.02 * len(c.filtered), skipped
        decisions = c.decisions(kind, thresholds)
        if kind == pc.MERGE_POISSON_REAL:
            for base in c.filtered:
                if base not in skipped:
                    assert o.poisson_merge_target(base) == decisions[base].target, (name, base, c.barcodes[base])
        if not skipped:
            want, excluded = pm.merge_targets(len(c.barcodes), c.filtered, [decisions[b].target for b in c.filtered])
            o.merge_and_filter()
            assert [int(x) for x in o.merge_targets()] == want
            assert sorted(int(i) for i in np.nonzero(o.cell_rows()[:, 1])[0]) == sorted(excluded)


def test_hand_built_decisions_are_the_intended_ones():
    c = pc.case("decisions")
    n = c.names
    strict, loose = (c.decisions(pc.MERGE_POISSON_REAL, t) for t in (pc.STRICT, pc.LOOSE))
    target = lambda d, x: d[n[x]].target
    assert target(strict, "B0") == n["R0"] == target(loose, "B0") and len(c.neighbours(pc.MERGE_POISSON_REAL, n["B0"])[0]) == 1
    assert target(strict, "B1") == n["R1"] and sorted(c.neighbours(pc.MERGE_POISSON_REAL, n["B1"])[0]) == sorted([n["R1"], n["R2"]])
    assert target(strict, "B2") == -1 == target(loose, "B2")
    assert target(strict, "R3") == n["R3"] and target(loose, "R3") == n["R4"]          # a real base: max_merge_prob, and its own id
    nb, levels = c.neighbours(pc.MERGE_POISSON_REAL, n["B4"])
    assert dict(zip(nb, levels)) == {n["R5"]: 1, n["R6"]: 2}
    tie = strict[n["B4"]]
    assert tie.probs[0][0] == tie.probs[1][0] and tie.target == n["R5"]                # exactly equal: the first in the order
    assert target(strict, "B5") == -1 and target(loose, "B5") == n["R1"]
    simple = c.decisions(pc.MERGE_POISSON_SIMPLE, pc.LOOSE)
    assert simple[n["B4"]].target == n["R5"] and simple[n["B2"]].target == n["B2"]


# ---- the Poisson tail -------------------------------------------------------------------------------------------------------
def tail_grid():
    grid = set()
    for exponent in (-8, -6, -4, -2, -1, 0, 0.5, 1, 1.5, 2, 2.5, 3, 3.5, 4):
        lam = 10.0 ** exponent
        sigma = math.sqrt(lam)
        ks = {1, 2, 3, 5, 10, 20, 40, 60}
        ks |= {int(round(lam + z * sigma)) for z in (-4, -2, -1, 0, 1, 2, 4)}
        ks |= {int(2 * lam) + 10, int(10 * lam) + 50 if lam <= 1000 else int(1.5 * lam)}
        grid |= {(k, lam) for k in ks if k >= 1}
    for k in (1, 2, 3, 10, 100, 1000):                                     # around the library's switch, lambda = k + 1
        grid |= {(k, k + 1 + d) for d in (-1, -1e-9, 0, 1e-9, 1)}
    return sorted(grid)


def test_poisson_tails_against_the_exact_series():
    """The bound: both functions form exp(-lambda + k ln(lambda) - lgamma(k)) (or the pmf the same way); each of the three terms
    is rounded, the library's lgamma and log are good to a few ulp, so the exponent is off by up to 4 * 2^-53 of the terms'
    magnitude and the result by that much relatively; the sums and the continued fraction add a few dozen roundings."""
    worst = {"oracle": (0, None), "library": (0, None)}
    for k, lam in tail_grid():
        want = pm.upper_tail(k, lam)
        bound = 4 * U * (lam + k * abs(math.log(lam)) + abs(math.lgamma(k + 1))) + 64 * U
        for who, got in (("oracle", ob.poisson_upper_tail(k, lam)), ("library", capi.poisson_upper_tail(k, lam))):
            dev = float(pm.relative_deviation(got, want))
            if dev > worst[who][0]:
                worst[who] = (dev, (k, lam))
            assert dev <= bound, (who, k, lam, got, float(want), dev, bound)
            assert (got == 0) == (want < Decimal(2) ** -1075) or want < pm.MIN_NORMAL, (who, k, lam, got)   # no underflow mismatch
    print("worst relative deviation of the Poisson tail:", worst)
    assert capi.poisson_upper_tail(0, 3.0) == 1 == pm.upper_tail(0, 3.0) and capi.poisson_upper_tail(-2, 3.0) == 1
    assert capi.poisson_upper_tail(4, 0.0) == 0 == pm.upper_tail(4, 0.0)
