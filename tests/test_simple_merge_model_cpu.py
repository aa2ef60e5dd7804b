"""The model of the whitelist-free barcode merges (simple_merge_model.py) and the oracle, pinned on each other on the CPU over the cases
of simple_merge_cases.py -- the device is compared with the model in test_gpu_simple_merge.py.

  common UMI-genes   the oracle's cells_with_common_umigs of every filtered base equals the model's dict
  targets            the oracle's per-base target lies in the model's set and is its one element where the model is decided; the bases
                     that hang on an iteration order are exactly the ones their cases name, with the sets they name
  final targets      merge_targets() after the oracle's merge_and_filter equals the model's second loop over the model's targets (over
                     the oracle's own target for a base that hangs on the order)
  caps               no hand-built case leaves a base undecided beside the named ones; a random container leaves at most 2 % -- counted
                     from the model alone, before anything is compared
  banded distance    the transcription against the oracle's on random pairs, where the reference does not read beyond its column
"""
import random

import numpy as np
import pytest

from oracle import Oracle
from oracle.binding import edit_distance as oracle_edit_distance

import poisson_cases as pc
import poisson_model as pm
import simple_merge_cases as sc
import simple_merge_model as smm
import whitelist_model as wm

ORACLE_KIND = {"simple": 2, "poisson": 4, "all": 5}
POISSON_MARGIN = pm.Decimal("1e-10")                       # poisson_cases.threshold_of at the oracle's smallest scale


def oracle_of(c, run):
    o = Oracle(merge_kind=ORACLE_KIND[run.kind], min_genes_before=c.min_genes, min_genes_after=c.min_genes, max_cb_merge_ed=run.max_ed,
               min_merge_fraction=run.min_fraction, max_merge_prob=pc.LOOSE[0], max_real_merge_prob=pc.LOOSE[1])
    o.add_packed(*c.arrays(), c.side)
    o.set_initialized()
    assert [int(x) for x in o.filtered_cells()] == c.filtered
    return o


def undecided_within_cap(c, i):
    """the bases of run i the model leaves open, checked against the case's claims and the caps -- from the model alone"""
    named = c.order_dependent.get(i, {})
    open_bases = c.undecided(i)
    if c.hand_built:
        assert set(open_bases) == set(named), (c.name, open_bases)
        for base, targets in named.items():
            assert c.answers(i)[base].targets == targets
    else:
        assert len(open_bases) <= sc.UNDECIDED_CAP * len(c.filtered), (c.name, open_bases)
    return open_bases


def test_the_run_list_is_the_cases():
    assert sc.runs_of() == [(name, i) for name in sc.NAMES for i in range(len(sc.case(name).runs))]
    for kind in ("simple", "poisson", "all"):
        assert all(sc.case(name).runs[i].kind == kind for name, i in sc.runs_of(kinds=(kind,)))
    assert set(sc.ORDER_DEPENDENT) == {name for name in sc.HAND_BUILT if sc.case(name).order_dependent}


def test_cases_are_what_the_issue_asks_for():
    assert [sc.case("all_F%d" % f).target_positions for f in sc.ALL_SIZES] == \
        [[], [0], [0, 62], [0, 63], [0, 64], [0, 63, 64, 254], [0, 63, 64, 255], [0, 63, 64, 256], [0, 63, 64, 255, 256, 512]]
    for seed in sc.RANDOM_SEEDS:
        c = sc.case("random_%d" % seed)
        assert 20 <= len(c.barcodes) <= 60 and 5 <= len({g for _, g, _ in c.molecules}) <= 40 and c.umi_len >= 6 and not c.hand_built
        moved = [a.target != b for b, a in c.answers(0).items() if a.decided]
        assert sum(moved) >= 3                                                  # the random containers do merge
    assert all(sc.case(name).hand_built for name in sc.HAND_BUILT)


@pytest.mark.parametrize("name", sorted({n for n, _ in sc.runs_of(kinds=("simple",))}))
def test_common_umigs_equal_the_oracle(name):
    c = sc.case(name)
    o = oracle_of(c, c.runs[0])
    for base in c.filtered:
        assert o.common_umigs(base) == smm.common_umigs(c, base), (name, base)


@pytest.mark.parametrize("name,i", sc.runs_of(kinds=("simple", "all")))
def test_targets_equal_the_oracle(name, i):
    c = sc.case(name)
    open_bases = undecided_within_cap(c, i)
    print("%-18s run %d %s: %d bases, %d not decided" % (name, i, tuple(c.runs[i]), len(c.filtered), len(open_bases)))
    o = oracle_of(c, c.runs[i])
    targets = {}
    for base, answer in c.answers(i).items():
        targets[base] = o.strategy_merge_target(base)
        if answer.decided:
            assert targets[base] == answer.target, (name, base)
        elif answer.targets is not None:
            assert targets[base] in answer.targets, (name, base)
    want = smm.final_targets(c, targets)
    o.merge_and_filter()
    assert [int(x) for x in o.merge_targets()] == want
    assert not o.cell_rows()[:, 1].any()                                        # these strategies never exclude


@pytest.mark.parametrize("name,i", sc.runs_of(kinds=("poisson",)))
def test_poisson_simple_targets_equal_the_oracle(name, i):
    """-M without a whitelist: the neighbour list is this model's, the decision poisson_model's"""
    c = sc.case(name)
    decisions = c.decisions(pc.MERGE_POISSON_SIMPLE, pc.LOOSE)
    assert not [b for b, d in decisions.items() if d.margin < POISSON_MARGIN]
    o = oracle_of(c, c.runs[i])
    for base in c.filtered:
        assert o.strategy_merge_target(base) == decisions[base].target, (name, base)
    for base, other, d, _ in getattr(c, "distance_pairs", ()):                  # `<=` against `<`: the pair at exactly max_ed
        assert decisions[base].target == (other if d <= c.max_ed else base)
        assert c.answers(0)[base].target == (other if d < c.max_ed else base)
    o.merge_and_filter()
    assert [int(x) for x in o.merge_targets()] == smm.final_targets(c, {b: d.target for b, d in decisions.items()})


def test_the_proof_rules_alone_decide_the_hand_built_cases():
    """The proof rules alone (no literal walk), as the issue measured them on the suite's streams: a clear best, or an exact tie with a
    unique largest gene count.  On the hand-built cases they decide every base the cases do not name."""
    for name, i in sc.runs_of(sc.HAND_BUILT, kinds=("simple",)):
        c = sc.case(name)
        for base, answer in c.answers(i).items():
            f = answer.fractions
            if not f or base in c.order_dependent.get(i, {}):
                continue
            best = max(f.values())
            group = [x for x in f if f[x] == best]
            clear = all(best - f[x] > smm.EPS for x in f if x not in group)
            most = max(c.n_genes[x] for x in group)
            if clear and sum(c.n_genes[x] == most for x in group) == 1:
                continue
            assert name in ("eps_band_1", "tie_band_genes"), (name, base)       # a near tie that the gene count decides needs the walk


def test_banded_distance_equals_the_oracle():
    rng = random.Random(5)
    differs = 0
    for _ in range(3000):
        a = "".join(rng.choice("ACGTN") for _ in range(rng.randint(6, 14)))
        b = list(a)
        for _ in range(rng.randint(0, 4)):
            at = rng.randrange(len(b) + 1)
            b[at:at + rng.randint(0, 1)] = rng.choice(["", "A", "C", "G", "T"])
        b = "".join(b) or "A"
        for max_ed in (0, 1, 2, 3, 12):
            if max(0, len(b) - max_ed) > len(a):
                continue                                                        # (the reference would read beyond its column)
            for skip_n in (False, True):
                got = smm.banded_edit_distance(a, b, skip_n, max_ed)
                assert got == oracle_edit_distance(a, b, skip_n, max_ed), (a, b, skip_n, max_ed)
                differs += skip_n and (got <= max_ed) != (wm.edit_distance(a, b) <= max_ed)
        assert smm.banded_edit_distance(a, b, True, 10000) == wm.edit_distance(a, b)
    assert differs > 0                                                          # the band does change answers
    base, other = sc.case("all_two_lengths").banded_pair
    bc = sc.case("all_two_lengths").barcodes
    assert oracle_edit_distance(bc[base], bc[other], False, 2) == 3 and oracle_edit_distance(bc[base], bc[other]) == 2
