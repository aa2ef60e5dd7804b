"""The -M estimator on the device (poisson_merge.h, k_collisions.h and their callers) against the exact model (poisson_model.py, pinned
by test_poisson_model_cpu.py), on the cases of poisson_cases.py.

  the stand-alone adjuster entry    capi.collisions_adjusted_sizes equals the model's integer table on every adjuster case; where the
                                    recurrence diverges, the entries before that point are the model's and the rest are marked
  the estimator through a context   per listed pair: the intersection size, `expected` and the probability against the exact values,
                                    expected(i, j) == expected(j, i) bit for bit, -1 and 1 on an empty intersection; the UMI
                                    distribution; the route (collisions_table and genes_intersection ran, over the case's classes)
  decisions                         merge_target(cell) of every filtered cell and the merge_targets() of a whole merge_and_filter(),
                                    -M with and without a whitelist, on every base the model can decide

Bounds.  D of a case is the largest relative deviation of the oracle -- the reference's formulas in double, left to right -- from
the exact model over that case's pairs, at least 2^-52, measured here again (poisson_cases.oracle_scale).  The device sums per class
of equally frequent UMIs (one product for m additions) and in tree order: a small multiple of the reference's own rounding, so its
bound is 16 D, for `expected` and for the probability each.  A base whose decision margin is under T = max(100 D, 1e-10) is skipped
and counted; test_poisson_model_cpu.py establishes that no hand-built case and at most 2 % of a random case's bases are."""
from functools import lru_cache

import numpy as np
import pytest

from dropest_amd import capi

import poisson_cases as pc
import poisson_model as pm

pytestmark = pytest.mark.gpu

DEVICE_FACTOR = 16
# poisson_merge.h: "`expected` agrees with the reference's to rounding (measured <= ... relative)"
HEADER_EXPECTED_AGREEMENT = 1e-12


# ---- the stand-alone adjuster entry -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.ADJUSTER_NAMES)
def test_adjuster_entry_equals_the_model(name):
    c = pc.adjuster_case(name)
    table, _, diverged_at = c.model()
    got = [int(x) for x in capi.collisions_adjusted_sizes(np.array(c.probs), c.max_expression)]
    assert got[:len(table)] == table, (name, got, table)
    if diverged_at is None:
        assert len(table) == c.max_expression
    else:                                                          # marked from the model's point of divergence on, not garbage
        assert len(table) == diverged_at - 1 < c.max_expression
        assert got[len(table):] == [capi.COLLISIONS_DIVERGED] * (c.max_expression - len(table)), (name, got)


def test_adjuster_entry_without_umis_or_sizes():
    assert list(capi.collisions_adjusted_sizes(np.zeros(0), 5)) == [1, 2, 3, 4, 5]
    assert len(capi.collisions_adjusted_sizes(np.array([0.25, 0.75]), 0)) == 0


def test_diverging_container_is_refused():
    """16 equally likely UMIs again, through -M: the filtered cells hold them, a cell that is not filtered holds a gene of 25 UMIs,
    and the table has to reach that size.  The class table diverges where the model does and the estimator says so."""
    molecules = {(c, g, u) for c in range(2) for g in range(2) for u in range(16)} | {(2, 0, u) for u in range(25)}
    c = pc.ContainerCase("diverges", pc.barcodes_plain(3), molecules, 3, 2, [(0, 1)])
    assert c.filtered == [0, 1]
    with pytest.raises(pm.CollisionsDiverged) as e:
        c.estimator()
    assert e.value.at == 19
    ctx = context_of(c, pc.MERGE_POISSON_SIMPLE)
    try:
        with pytest.raises(capi.DropestError) as e:
            ctx.poisson_intersection_prob(0, 1)
        assert e.value.status == 4 and "diverged" in str(e.value)
    finally:
        ctx.close()


# ---- the estimator through a context ----------------------------------------------------------------------------------------
def context_of(c, kind, thresholds=pc.STRICT, whitelist=None):
    ctx = capi.Context(merge_kind=kind, barcodes_kind=capi.BARCODES_CONST, barcodes_file=whitelist, min_genes_before_merge=c.min_genes,
                       min_genes_after_merge=c.min_genes, max_cb_merge_edit_distance=c.max_ed, max_merge_prob=thresholds[0],
                       max_real_merge_prob=thresholds[1])
    ctx.set_profiling(True)
    ctx.push_reads(*c.arrays())
    ctx.set_initialized()
    return ctx


@lru_cache(maxsize=None)
def device_run(name):
    """One context per case -> what the device says about its pairs, both ways round, its distribution and its kernel statistics"""
    c = pc.case(name)
    ctx = context_of(c, pc.MERGE_POISSON_SIMPLE)
    try:
        assert [int(x) for x in ctx.filtered_cells()] == c.filtered
        codes, counts = ctx.umi_distribution()
        sentinel = 1 << (2 * c.umi_len)
        distribution = {int(u) ^ sentinel: int(k) for u, k in zip(codes, counts)}
        forward = [ctx.poisson_intersection_prob(a, b) for a, b in c.pairs]
        backward = [ctx.poisson_intersection_prob(b, a) for a, b in c.pairs]
        return distribution, forward, backward, ctx.kernel_stats()
    finally:
        ctx.close()


@lru_cache(maxsize=None)
def scale_of(name):
    c = pc.case(name)
    return pc.oracle_scale(c, pc.oracle_of(c))


@lru_cache(maxsize=None)
def deviations(name):
    """(device from exact, device from oracle) for `expected`, (device from exact) for the probability: the largest over the pairs"""
    c = pc.case(name)
    o = pc.oracle_of(c)
    _, forward, _, _ = device_run(name)
    exact_e = oracle_e = exact_p = pm.Decimal(0)
    for (a, b), (n, expected, prob), got in zip(c.pairs, c.pair_results(), forward):
        if n:
            exact_e = max(exact_e, pm.relative_deviation(got[1], expected))
            oracle_e = max(oracle_e, pm.relative_deviation(got[1], pm.exact(o.poisson_expected_intersection(a, b))))
            exact_p = max(exact_p, pm.relative_deviation(got[2], prob))
    return exact_e, oracle_e, exact_p


@pytest.mark.parametrize("name", pc.CONTAINER_NAMES)
def test_estimator_equals_the_model(name):
    c = pc.case(name)
    e = c.estimator()
    distribution, forward, backward, stats = device_run(name)
    assert distribution == dict(e.distribution)
    d_expected, d_prob = scale_of(name)
    dev_e, _, dev_p = deviations(name)
    figures = "%s: D(expected) %.3g, device %.3g; D(probability) %.3g, device %.3g" % (name, d_expected, dev_e, d_prob, dev_p)
    print(figures)
    for (a, b), (n, expected, prob), got, back in zip(c.pairs, c.pair_results(), forward, backward):
        assert got[0] == n == back[0], (name, a, b, got, n)
        if n == 0:
            assert got[1] == -1 and got[2] == 1 and back[1] == -1 and back[2] == 1, (name, a, b, got, back)
            continue
        assert got[1] == back[1] and got[2] == back[2], (name, a, b, got, back)          # the sum runs in gene order either way
        assert pm.relative_deviation(got[1], expected) <= DEVICE_FACTOR * d_expected, (a, b, got[1], float(expected), figures)
        assert pm.relative_deviation(got[2], prob) <= DEVICE_FACTOR * d_prob, (a, b, got[2], float(prob) if prob > pm.MIN_NORMAL else prob, figures)
    # the route: one table and one est() launch per estimated pair with a non-empty intersection, over the case's classes and sizes
    calls = 2 * sum(1 for n, _, _ in c.pair_results() if n)
    if calls:
        assert stats["collisions_table"]["launches"] == calls and stats["genes_intersection"]["launches"] == calls
        assert stats["collisions_table"]["bytes"] == calls * float(e.max_size) * c.n_classes * 24, (name, stats["collisions_table"], e.max_size, c.n_classes)
    if name in pc.CLASS_COUNTS:
        assert c.n_classes == pc.CLASS_COUNTS[name]


def test_expected_agrees_with_the_reference_as_the_header_says():
    """poisson_merge.h states how far `expected` is from the reference's own double evaluation; here the oracle stands for the
    reference.  The table this prints (run with -s) is every case's D, and the device's deviation from the exact value."""
    worst_exact = worst_oracle = pm.Decimal(0)
    for name in pc.CONTAINER_NAMES:
        d_expected, d_prob = scale_of(name)
        dev_e, dev_o, dev_p = deviations(name)
        print("%-24s D(expected) %.3g device-exact %.3g device-oracle %.3g | D(probability) %.3g device-exact %.3g"
              % (name, d_expected, dev_e, dev_o, d_prob, dev_p))
        worst_exact, worst_oracle = max(worst_exact, dev_e), max(worst_oracle, dev_o)
    print("largest relative deviation of the device's expected: from the exact value %.3g, from the oracle %.3g" % (worst_exact, worst_oracle))
    assert worst_oracle <= HEADER_EXPECTED_AGREEMENT, float(worst_oracle)


# ---- decisions --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [pc.MERGE_POISSON_REAL, pc.MERGE_POISSON_SIMPLE], ids=["real", "simple"])
@pytest.mark.parametrize("name", pc.DECISION_NAMES)
def test_merge_targets_equal_the_model(name, kind, tmp_path):
    c = pc.case(name)
    path = pc.write_whitelist(c, tmp_path)
    _, d_prob = scale_of(name)
    threshold = pc.threshold_of(d_prob)
    for thresholds in c.thresholds:
        decisions = c.decisions(kind, thresholds)
        skipped = [b for b in c.filtered if decisions[b].margin < threshold]
        allowed = 0 if c.hand_built else int(0.02 * len(c.filtered))
        assert len(skipped) <= allowed, (name, kind, thresholds, skipped, float(threshold))
        ctx = context_of(c, kind, thresholds, path if kind == pc.MERGE_POISSON_REAL else None)
        try:
            if kind == pc.MERGE_POISSON_REAL:                      # (dropest_merge_target answers for the whitelist merges only)
                for base in c.filtered:
                    if base not in skipped:
                        assert ctx.merge_target(base) == decisions[base].target, (name, thresholds, base, c.barcodes[base])
            stats = ctx.kernel_stats() if kind == pc.MERGE_POISSON_REAL else None
            ctx.merge_and_filter()
            if not skipped:
                want, excluded = pm.merge_targets(len(c.barcodes), c.filtered, [decisions[b].target for b in c.filtered])
                assert [int(x) for x in ctx.merge_targets()] == want, (name, kind, thresholds)
                assert sorted(int(i) for i in np.nonzero(ctx.cell_rows()["is_excluded"])[0]) == sorted(excluded)
            stats = stats or ctx.kernel_stats()
            if any(d.probs and any(p < 1 for p, _, _ in d.probs) for d in decisions.values()):
                assert stats["collisions_table"]["launches"] >= 1 and stats["genes_intersection"]["launches"] >= 1
        finally:
            ctx.close()
