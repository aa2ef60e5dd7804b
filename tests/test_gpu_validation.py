"""`dropest -S` on the device (k_validation.h, validation.h, dropest_merge_validation) against the model (validation_model.py, pinned by
test_validation_model_cpu.py) on the cases of validation_cases.py.

Comparison.  The model runs on what the SAME context reports: filtered_cells(), the barcodes and TOTAL_UMIS of cell_rows() and the
{cell: {gene: set(umi)}} dict of molecules() -- after merge_and_filter where the case merges.  Cells, UMI counts, distances, intersection
sizes, n_found, draws_used and complete must be equal.  `expected` and the probability are compared with the exact model within
DEVICE_FACTOR x D (the 16 of test_gpu_poisson_estimator.py, for the reason given there); D is measured in the same run as there: the
largest relative deviation, at least 2^-52, of the CPU checker's double evaluation from the exact value over the sample's pairs -- the
checker being fed the context's current molecules as one read each, no merge, thresholds 1."""
import numpy as np
import pytest

from dropest_amd import capi
from dropest_amd.multi import ShardGroup

import poisson_model as pm
import validation_cases as vc
import validation_model as vm
from test_gpu_poisson_estimator import DEVICE_FACTOR

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -52
INT_KEYS = ("cell1", "cell2", "umis1", "umis2", "edit_distance", "intersection")
ALL_KEYS = INT_KEYS + ("expected", "probability")


class State:
    """one case on the device, merged where the case says so, with what the model needs read back"""

    def __init__(self, name, tmp, merge=None):
        c = self.case = vc.case(name)
        cb, umi, gene, aux, side = c.arrays()
        self.side = side
        self.ctx = capi.Context(barcodes_file=c.whitelist(tmp), **c.ctx)
        if side:
            self.ctx.set_side_strings(side)
        self.ctx.push_reads(cb, umi, gene, aux)
        self.ctx.set_initialized()
        if c.merge if merge is None else merge:
            self.ctx.merge_and_filter()
        self.refresh()

    def refresh(self):
        ctx = self.ctx
        self.filtered = [int(x) for x in ctx.filtered_cells()]
        self.rows = ctx.cell_rows()
        self.barcode = {i: capi.unpack_code(self.rows["barcode"][i], self.side) for i in self.filtered}
        self.molecules = ctx.molecules()
        self.container = vm.container_of(*self.molecules[:3])

    def close(self):
        self.ctx.close()

    def model_sample(self, lo, hi, n, cap):
        return vm.run_validation(self.filtered, self.barcode.get, lo, hi, n, cap)

    def scale(self, pairs, exact):
        """D of `expected` and of the probability over `pairs` (see the module's docstring)"""
        from oracle import Oracle
        cell, gene, umi = self.molecules[:3]
        keep = np.isin(cell, self.filtered)
        o = Oracle(merge_kind=0, min_genes_before=1, min_genes_after=1)
        o.add_packed(self.rows["barcode"][cell[keep]], umi[keep], gene[keep], np.full(int(keep.sum()), 2 << 16, np.uint32), self.side)
        o.set_initialized()
        o.poisson_init()
        ids = {}
        d_expected = d_prob = pm.Decimal(ULP)
        for (a, b), (k, expected, prob) in zip(pairs, exact):
            if not k:
                continue
            for c in (a, b):
                if c not in ids:
                    ids[c] = o.cell_id_by_cb(self.barcode[c])
            d_expected = max(d_expected, pm.relative_deviation(o.poisson_expected_intersection(ids[a], ids[b]), expected))
            d_prob = max(d_prob, pm.relative_deviation(o.poisson_intersection_prob(ids[a], ids[b]), prob))
        return d_expected, d_prob

    def check(self, got, lo, hi, n, cap):
        """every output of one sample against the model"""
        s = self.model_sample(lo, hi, n, cap)
        assert (got["n_found"], got["draws_used"], bool(got["complete"])) == (s.n_found, s.draws_used, s.complete), (self.case.name, lo, hi, n)
        assert [int(x) for x in got["cell1"]] == s.cell1 and [int(x) for x in got["cell2"]] == s.cell2
        assert [int(x) for x in got["edit_distance"]] == s.edit_distance
        assert [int(x) for x in got["umis1"]] == [int(self.rows["total_umis"][c]) for c in s.cell1]
        assert [int(x) for x in got["umis2"]] == [int(self.rows["total_umis"][c]) for c in s.cell2]
        exact = vm.evaluate(vm.estimator_of(self.container, self.filtered), s.pairs())
        d_expected, d_prob = self.scale(s.pairs(), exact)
        worst_e = worst_p = pm.Decimal(0)
        for p, (k, expected, prob) in enumerate(exact):
            assert int(got["intersection"][p]) == k, (self.case.name, p, s.pairs()[p])
            if k == 0:
                assert got["expected"][p] == -1 and got["probability"][p] == 1
                continue
            worst_e = max(worst_e, pm.relative_deviation(float(got["expected"][p]), expected))
            worst_p = max(worst_p, pm.relative_deviation(float(got["probability"][p]), prob))
        print("%s (%d, %d, %d): %d pairs, %d empty; D(expected) %.3g device %.3g; D(probability) %.3g device %.3g"
              % (self.case.name, lo, hi, n, s.n_found, sum(1 for k, _, _ in exact if not k), d_expected, worst_e, d_prob, worst_p))
        assert worst_e <= DEVICE_FACTOR * d_expected and worst_p <= DEVICE_FACTOR * d_prob
        return s, exact


@pytest.fixture(scope="module")
def states(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("validation")
    made = {}

    def get(name, merge=None):
        if (name, merge) not in made:
            made[(name, merge)] = State(name, tmp, merge)
        return made[(name, merge)]

    yield get
    for s in made.values():
        s.close()


def same_bits(a, b):
    for k in ALL_KEYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k
    assert (a["n_found"], a["draws_used"], a["complete"]) == (b["n_found"], b["draws_used"], b["complete"])


# ---- the samples against the model -----------------------------------------------------------------------------------------------------
def test_planted_barcodes(states):
    st = states("planted")
    (lo, hi, n, cap, _), (lo2, hi2, n2, cap2, _) = st.case.samples
    both = st.ctx.merge_validation((lo, hi, n), (lo2, hi2, n2), max_draws=cap)
    distant, exact_far = st.check(both[0], lo, hi, n, cap)
    adjacent, exact = st.check(both[1], lo2, hi2, n2, cap2)
    assert both[0]["rounds"] == 1                                   # a little over n candidates were enough
    # (what the barcodes were planted for: test_validation_model_cpu.py shows it on the model, which the samples equal)
    assert any(e != vm.levenshtein(st.barcode[a], st.barcode[b]) for (a, b), e in zip(distant.pairs(), distant.edit_distance))
    for e in (exact, exact_far):                                    # empty and non-empty intersections in both samples
        assert any(k == 0 for k, _, _ in e) and any(k > 0 for k, _, _ in e)
    # one sample through dropest_merge_validation gives what the two-sample call gave
    one = st.ctx.merge_validation(lo2, hi2, n2, max_draws=cap2)
    same_bits(one, both[1])


def test_before_merge_and_filter(states):
    st = states("planted", merge=False)
    lo, hi, n, cap, _ = st.case.samples[1]
    st.check(st.ctx.merge_validation(lo, hi, n, max_draws=cap), lo, hi, n, cap)


@pytest.mark.parametrize("name", ["whitelist", "simple"])
def test_after_a_barcode_merge(states, name):
    st = states(name)
    src, _ = st.ctx.merge_target_pairs()
    assert len(src) >= 3                                            # the merge folded cells
    for lo, hi, n, cap, _ in st.case.samples:
        got = st.ctx.merge_validation(lo, hi, n, max_draws=cap)
        st.check(got, lo, hi, n, cap)
        assert not set(int(x) for x in src) & (set(int(x) for x in got["cell1"]) | set(int(x) for x in got["cell2"]))


@pytest.mark.parametrize("name", ["n_umis", "directional"])
def test_with_rewritten_groups(states, name):
    st = states(name)
    plain = {(c, g, capi.pack_seq(u) if "N" not in u else None, r) for c, g, u, r in _summed(st.case.molecules)}
    cell, gene, umi, reads, _ = st.molecules
    now = {(int(c), int(g), int(u), int(r)) for c, g, u, r in zip(cell, gene, umi, reads)}
    assert now - plain, "the UMI merge rewrote nothing"             # a molecule the table built from the reads does not hold
    for lo, hi, n, cap, _ in st.case.samples:
        st.check(st.ctx.merge_validation(lo, hi, n, max_draws=cap), lo, hi, n, cap)


def _summed(molecules):
    out = {}
    for c, g, u, r in molecules:
        out[(c, g, u)] = out.get((c, g, u), 0) + r
    return [(c, g, u, r) for (c, g, u), r in out.items()]


# ---- round and chunk boundaries: no output may depend on them ---------------------------------------------------------------------------
def test_round_boundaries(states):
    st = states("planted")
    for lo, hi, cap in ((5, 100, 1 << 16), (1, 1, 1 << 16)):
        # n such that the n-th acceptance is the LAST candidate of a round of 63, 64 or 65 (not the first round)
        edge = None
        for n in range(8, 200):
            d = st.model_sample(lo, hi, n, cap).draws_used
            hit = [r for r in (63, 64, 65) if d % r == 0 and d > r]
            if hit:
                edge = (n, hit[0], d)
                break
        assert edge is not None, (lo, hi)
        n, r_edge, draws = edge
        base = st.ctx.merge_validation(lo, hi, n, max_draws=cap, round_candidates=1 << 20)
        assert base["draws_used"] == draws and base["complete"] == 1
        st.check(base, lo, hi, n, cap)
        for r in (1, 63, 64, 65, r_edge, draws):
            same_bits(st.ctx.merge_validation(lo, hi, n, max_draws=cap, round_candidates=r), base)
        same_bits(st.ctx.merge_validation(lo, hi, n, max_draws=cap), base)               # the default rounds
        # n reached in the middle of a wave: the following candidates of that wave are accepted ones too in the distant sample
        mid = st.ctx.merge_validation(lo, hi, n + 1, max_draws=cap, round_candidates=64)
        same_bits(mid, st.ctx.merge_validation(lo, hi, n + 1, max_draws=cap, round_candidates=1 << 20))


def test_chunk_boundaries(states):
    st = states("planted")
    lo, hi, n, cap, _ = st.case.samples[0]
    base = st.ctx.merge_validation((lo, hi, n), (1, 1, 16), max_draws=cap)
    assert base[0]["chunks"] == 1
    common = [len(st.container[int(a)].keys() & st.container[int(b)].keys()) for a, b in zip(base[0]["cell1"], base[0]["cell2"])]
    assert max(common) > 1                                           # one pair's keys alone exceed a budget of 1
    for budget in (1, 64):
        got = st.ctx.merge_validation((lo, hi, n), (1, 1, 16), max_draws=cap, max_keys_per_chunk=budget)
        for a, b in zip(got, base):
            same_bits(a, b)
        assert got[0]["chunks"] > 1
        if budget == 1:                                              # a chunk takes pairs while their keys fit; an empty pair rides along
            assert got[0]["chunks"] >= sum(1 for k in common if k)


# ---- termination -----------------------------------------------------------------------------------------------------------------------
def test_cap_ends_a_sample_that_finds_nothing(states):
    st = states("far_apart")
    lo, hi, n, cap, _ = st.case.samples[0]
    assert cap == 10000
    got = st.ctx.merge_validation(lo, hi, n, max_draws=cap)
    assert (got["n_found"], got["complete"], got["draws_used"]) == (0, 0, 10000)
    st.check(got, lo, hi, n, cap)


def test_cap_ends_a_sample_part_way(states):
    st = states("few_adjacent")
    lo, hi, n, cap, _ = st.case.samples[0]
    got = st.ctx.merge_validation(lo, hi, n, max_draws=cap)
    assert 0 < got["n_found"] < n and got["complete"] == 0 and got["draws_used"] == cap
    st.check(got, lo, hi, n, cap)
    same_bits(st.ctx.merge_validation(lo, hi, n, max_draws=cap, round_candidates=777), got)


@pytest.mark.parametrize("name", ["no_cell", "one_cell"])
def test_fewer_than_two_filtered_cells(states, name):
    st = states(name)
    assert len(st.filtered) == (0 if name == "no_cell" else 1)
    for lo, hi, n, cap, _ in st.case.samples:
        got = st.ctx.merge_validation(lo, hi, n, max_draws=cap)
        assert (got["n_found"], got["complete"], got["draws_used"]) == (0, 0, 0)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_shards_and_split_contexts_are_refused():
    c = vc.case("planted")
    cb, umi, gene, aux, side = c.arrays()
    ctx = capi.Context(**c.ctx)
    ctx.set_side_strings(side)
    ctx.push_reads(cb, umi, gene, aux)
    g = ShardGroup.split(ctx, 2)
    try:
        with pytest.raises(capi.DropestError) as e:
            ctx.merge_validation(1, 1, 4)
        assert e.value.status == 4 and "split" in str(e.value)
        with pytest.raises(capi.DropestError) as e:
            g.shards[0].ctx.merge_validation(1, 1, 4)
        assert e.value.status == 4 and "shard" in str(e.value)
    finally:
        g.close()
        ctx.close()
