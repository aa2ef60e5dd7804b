"""The whitelist-free barcode merges on the device (simple_merge.h, merge_all.h and their callers) against the plain model
(simple_merge_model.py, pinned on the oracle by test_simple_merge_model_cpu.py), piece by piece, on the cases of simple_merge_cases.py.

  pair table     dropest_simple_merge_pairs as {(base, other): shared} equals the model's common_umigs of every filtered base -- the pairs
                 that must be absent included
  distances      the device's distance of every pair equals the model's plain Levenshtein distance (N matches anything); it is left to the
                 host (0xFFFFFFFF) exactly where a barcode is escaped (an N, more than 31 bases)
  targets        dropest_merge_target of every filtered base, before the merge -- computed by the steps the merge itself runs -- equals the
                 model's answer where the model is decided; where the reference's answer hangs on an iteration order it lies in the
                 model's set and equals the oracle's
  after          merge_targets() after merge_and_filter equals the model's second loop over those targets; every observable equals the oracle's
  routes         which kernels and host stages ran, from kernel_stats()
  shards         every hand-built Simple and merge-all case through 2 and 3 in-process shards: the oracle's matrices and merges, and the
                 merges of the one context

Everything compared is an integer or a set: nothing here has a tolerance."""
import copy
from functools import lru_cache

import pytest

from dropest_amd import capi
import parity
import poisson_cases as pc
import simple_merge_cases as sc
import simple_merge_model as smm
from test_gpu_multi_oracle import check_vs_oracle, even_bounds, run_shards
from test_simple_merge_model_cpu import POISSON_MARGIN, oracle_of, undecided_within_cap

pytestmark = pytest.mark.gpu

CAPI_KIND = {"simple": capi.MERGE_SIMPLE, "poisson": capi.MERGE_POISSON_SIMPLE, "all": capi.MERGE_ALL}
SIMPLE_KERNELS = ("simple:umig_keys", "simple:umig_pairs", "seg_count:simple:pair_runs", "seg_reduce:simple:pair_runs", "simple:pair_distance")
UNSUPPORTED = 4


def context_kw(c, run):
    return dict(merge_kind=CAPI_KIND[run.kind], min_genes_before_merge=c.min_genes, min_genes_after_merge=c.min_genes,
                max_cb_merge_edit_distance=run.max_ed, min_merge_fraction=run.min_fraction, max_merge_prob=pc.LOOSE[0],
                max_real_merge_prob=pc.LOOSE[1])


@lru_cache(maxsize=None)
def device_run(name, i):
    """One fresh context per (case, run), profiling on: the pair table and the targets before the merge, then merge_and_filter and the
    comparison of every observable with the oracle.  A width the library refuses is recorded, not answered."""
    c = sc.case(name)
    run = c.runs[i]
    ctx = capi.Context(**context_kw(c, run))
    out = {"refused": None}
    try:
        ctx.set_profiling(True)
        if c.side:
            ctx.set_side_strings(c.side)
        try:
            ctx.push_reads(*c.arrays())
            ctx.set_initialized()
            assert [int(x) for x in ctx.filtered_cells()] == c.filtered
            if run.kind != "all":
                base, other, shared, distance = ctx.simple_merge_pairs()
                out["pairs"] = {(int(b), int(o)): (int(s), int(d)) for b, o, s, d in zip(base, other, shared, distance)}
                assert len(out["pairs"]) == len(base)
                assert list(zip(base.tolist(), other.tolist())) == sorted(out["pairs"])               # ascending (base, other)
            out["targets"] = {b: ctx.merge_target(b) for b in c.filtered}
            out["stats_before"] = set(ctx.kernel_stats())
            ctx.merge_and_filter()
        except capi.DropestError as e:
            if name not in sc.KEY_WIDTH_CASES or e.status != UNSUPPORTED:
                raise
            out["refused"] = str(e)
            return out
        out["merge_targets"] = [int(x) for x in ctx.merge_targets()]
        out["stats"] = set(ctx.kernel_stats())
        src, tgt = ctx.merge_target_pairs()
        out["merged"] = {c.barcodes[int(a)]: c.barcodes[int(b)] for a, b in zip(src, tgt)}
        o = oracle_of(c, run)
        out["oracle_targets"] = {b: o.strategy_merge_target(b) for b in c.filtered}
        o.merge_and_filter()
        parity.compare(o, ctx, c.side)
    finally:
        ctx.close()
    return out


def refused(name, got):
    """a width the library refuses (UnsupportedError) is one the case records as refused"""
    if got["refused"] is None:
        assert name not in ["key_width_%d" % w for w in sc.KEY_WIDTH_REFUSED["one context"]]
        return False
    print("%s: the library refuses this width: %s" % (name, got["refused"]))
    assert name in ["key_width_%d" % w for w in sc.KEY_WIDTH_REFUSED["one context"]]
    return True


# ---- the pair table and the distances ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted({n for n, _ in sc.runs_of(kinds=("simple",))}))
def test_pair_table_equals_the_model(name):
    c = sc.case(name)
    got = device_run(name, 0)
    if refused(name, got):
        return
    want = {(base, other): shared for base in c.filtered for other, shared in smm.common_umigs(c, base).items()}
    have = {pair: shared for pair, (shared, _) in got["pairs"].items()}
    assert have == want, (name, sorted(set(have) ^ set(want))[:10], [(p, have[p], want[p]) for p in have if p in want and have[p] != want[p]][:10])
    for (base, other), (_, distance) in got["pairs"].items():
        if c.on_device(base, other):
            assert distance == smm.distance(c, base, other), (name, c.barcodes[base], c.barcodes[other])
        else:
            assert distance == sc.NOT_ON_DEVICE, (name, c.barcodes[base], c.barcodes[other])
    for base, other, d, _ in getattr(c, "distance_pairs", ()):
        assert got["pairs"][base, other][1] == (d if c.on_device(base, other) else sc.NOT_ON_DEVICE)


def test_pair_table_edges_reach_the_device():
    """what the cases are made for arrives in the table: the counts around 256 and the large one, both orders of equal sizes, ids beyond 2^12"""
    pairs = device_run("shared_counts", 0)["pairs"]
    assert sorted(s for s, _ in pairs.values()) == sorted(2 * list(sc.SHARED_COUNTS))
    c = sc.case("high_cell_ids")
    assert min(b for b, _ in device_run("high_cell_ids", 0)["pairs"]) >= 1 << 12 and len(c.barcodes) > 5000
    assert len(device_run("hot_600", 0)["pairs"]) == sum(len(smm.common_umigs(sc.case("hot_600"), b)) for b in range(600)) > 200000
    assert any(d == sc.NOT_ON_DEVICE for _, d in device_run("barcode_long", 0)["pairs"].values())


def test_handles_refuse_what_they_do_not_cover():
    c = sc.case("pair_runs")
    for kind in ("simple", "all"):
        ctx = capi.Context(**context_kw(c, sc.Run(kind, 2, 0.2)))
        try:
            ctx.push_reads(*c.arrays())
            ctx.set_initialized()
            with pytest.raises(capi.DropestError) as e:
                ctx.merge_target(4)                                        # cell 4 is not filtered
            assert e.value.status == 1
            if kind == "all":
                with pytest.raises(capi.DropestError) as e:
                    ctx.simple_merge_pairs()
                assert e.value.status == 1
            assert ctx.merge_target(c.filtered[0]) in c.filtered
            ctx.merge_and_filter()
            with pytest.raises(capi.DropestError) as e:                    # the un-merged state is gone
                ctx.merge_target(c.filtered[0])
            assert e.value.status == 1
        finally:
            ctx.close()


def test_kept_targets_follow_a_change_of_the_container():
    """The targets are kept from the first call until the container changes: with cell 1 of second_loop excluded -- the one candidate of
    cell 0 -- the answers are the model's over the filtered cells that are left, and the merge applies those."""
    c = sc.case("second_loop")
    ctx = capi.Context(**context_kw(c, c.runs[0]))
    try:
        ctx.push_reads(*c.arrays())
        ctx.set_initialized()
        assert ctx.merge_target(0) == 1 and ctx.merge_target(1) == 2
        ctx.exclude_cell(1)
        left = copy.copy(c)
        left.filtered = [b for b in c.filtered if b != 1]
        left._umig_index, left._answers = None, {}
        assert [int(x) for x in ctx.filtered_cells()] == left.filtered
        targets = {b: ctx.merge_target(b) for b in left.filtered}
        assert targets == {b: a.target for b, a in left.answers(0).items()} and targets[0] == 0
        with pytest.raises(capi.DropestError) as e:
            ctx.merge_target(1)
        assert e.value.status == 1
        assert {(int(b), int(o)) for b, o in zip(*ctx.simple_merge_pairs()[:2])} == \
            {(b, o) for b in left.filtered for o in smm.common_umigs(left, b)}
        ctx.merge_and_filter()
        assert [int(x) for x in ctx.merge_targets()] == smm.final_targets(left, targets)
    finally:
        ctx.close()


# ---- targets, and the state after the merge ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,i", sc.runs_of(kinds=("simple", "all")))
def test_targets_equal_the_model(name, i):
    c = sc.case(name)
    open_bases = undecided_within_cap(c, i)
    got = device_run(name, i)
    if refused(name, got):
        return
    for base, answer in c.answers(i).items():
        if answer.decided:
            assert got["targets"][base] == answer.target, (name, base, c.barcodes[base])
        else:
            assert answer.targets is None or got["targets"][base] in answer.targets, (name, base)
            assert got["targets"][base] == got["oracle_targets"][base], (name, base)
    assert got["merge_targets"] == smm.final_targets(c, got["targets"])
    assert len(open_bases) <= (len(c.order_dependent.get(i, {})) if c.hand_built else sc.UNDECIDED_CAP * len(c.filtered))


@pytest.mark.parametrize("name,i", sc.runs_of(kinds=("poisson",)))
def test_poisson_simple_targets_equal_the_model(name, i):
    """-M without a whitelist takes its neighbours with `<=` where Simple has `<`: the other at exactly max_ed is the target under -M (the
    thresholds are loose) and not under Simple"""
    c = sc.case(name)
    decisions = c.decisions(pc.MERGE_POISSON_SIMPLE, pc.LOOSE)
    assert not [b for b, d in decisions.items() if d.margin < POISSON_MARGIN]
    got, simple = device_run(name, i), device_run(name, 0)
    assert c.runs[0].kind == "simple" and got["pairs"] == simple["pairs"]
    assert got["targets"] == {b: d.target for b, d in decisions.items()}
    assert got["merge_targets"] == smm.final_targets(c, got["targets"])
    at_max = [(base, other) for base, other, d, _ in getattr(c, "distance_pairs", ()) if d == c.max_ed]
    assert at_max or not hasattr(c, "distance_pairs") or name == "barcode_long"
    for base, other in at_max:
        assert got["targets"][base] == other and simple["targets"][base] == base


# ---- routes -------------------------------------------------------------------------------------------------------------------
def test_routes():
    for name, i in sc.runs_of(sc.HAND_BUILT, kinds=("simple", "poisson")):
        got = device_run(name, i)
        if refused(name, got):
            continue
        assert set(SIMPLE_KERNELS) <= got["stats_before"] and set(SIMPLE_KERNELS) <= got["stats"], name
        assert "merge_all" not in got["stats"]
    replayed = {name for name, i in sc.runs_of(sc.HAND_BUILT, kinds=("simple",)) if "host:cb_merge:replay" in (device_run(name, i).get("stats") or ())}
    assert {"eps_band_3", "tie_unique_genes", "tie_shared_genes", "tie_chain", "tie_band_genes"} <= replayed
    # every base of these is more than 2 EPS clear of its other candidates
    clear = ["eps_band_5", "pair_runs", "high_cell_ids", "hot_600", "tiles", "shared_counts", "second_loop", "hot_umig", "nobody_admissible",
             "exact_fractions", "run_end_255", "run_end_256", "run_end_257"] + ["distance_ed%d" % e for e in sc.DISTANCE_MAX_EDS]
    for name in clear:
        c = sc.case(name)
        for a in c.answers(0).values():
            f = sorted(a.fractions.values())
            assert len(f) < 2 or f[-1] - f[-2] > 2 * smm.EPS
        assert name not in replayed, name
    for name, i in sc.runs_of(sc.HAND_BUILT, kinds=("all",)):
        stats = device_run(name, i)["stats"]
        on_host = name in ("all_two_lengths", "all_with_n")
        assert ("merge_all" in stats) == (not on_host) and ("host:cb_merge:targets_host" in stats) == on_host, name
        assert not set(SIMPLE_KERNELS) & stats


# ---- shards -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name,i", sc.runs_of(sc.HAND_BUILT, kinds=("simple", "all")))
def test_shards_equal_the_oracle_and_the_one_context(name, i, world):
    """The stream is cut evenly: a cell's molecules, the 300 holders of one UMI-gene (tiles) and the 70 000 UMI-genes two cells share
    (shared_counts) lie on both sides of a cut, so the partial counts of the index shards have to add up."""
    c = sc.case(name)
    one = device_run(name, i)
    arrays = c.arrays()
    refusing = name in ["key_width_%d" % w for w in sc.KEY_WIDTH_REFUSED["shards"]]
    try:
        got = run_shards(arrays, context_kw(c, c.runs[i]), even_bounds(len(arrays[0]), world), side=tuple(c.side))
    except capi.DropestError as e:
        if not refusing or e.status != UNSUPPORTED:
            raise
        print("%s over %d shards: the library refuses this width: %s" % (name, world, e))
        return
    assert not refusing, name
    o = oracle_of(c, c.runs[i])
    o.merge_and_filter()
    merged = check_vs_oracle(got, o, tuple(c.side))
    if not refused(name, one):
        assert merged == one["merged"]
