"""`dropest -S` over the shards of a sharded or split run (csrc/shard_validation.h; dropest_shard_merge_validation_samples and the group
entry) against ONE context on the same reads (test_gpu_validation.State) and, through it, against the model.

All shards share device 0; the reads are dealt in contiguous ranges.  cell1 / cell2 of a sharded sample are columns of the filtered matrix:
they are mapped to barcodes through its col_barcode and from there to the one context's cell ids, then State.check runs on the mapped
sample as it does on the context's own.

Reals.  Where no UMI group was rewritten a pair's numbers depend on its own view keys and on tables made from the same multiset of UMI
codes, and the view keys are the one context's (the global position of a cell is its rank there): `expected` and the probability are
BIT-EQUAL to the one context's.  n_umis / directional: override UMIs above the UMI field are numbered in sorted order here and in map
order on one context, so the tables' classes may be walked in another order; those stay within DEVICE_FACTOR x D of the exact model
(State.check) and are bit-equal between world 2 and world 3."""
import ctypes as C
import threading

import numpy as np
import pytest

from dropest_amd import capi
from dropest_amd.multi import ShardGroup

import validation_cases as vc
from test_gpu_validation import ALL_KEYS, INT_KEYS, State, same_bits, states  # noqa: F401 (states: the module's fixture of one-context runs)

pytestmark = pytest.mark.gpu

CASES = ["planted", "whitelist", "simple", "n_umis", "directional", "far_apart", "few_adjacent", "one_cell", "no_cell"]
PLAIN_VIEW = ("planted", "whitelist", "simple", "far_apart", "few_adjacent")      # no rewritten UMI groups
WORLDS = (2, 3)


def even_bounds(n, world):
    return [n * i // world for i in range(world + 1)]


def make_group(name, world, tmp, options=()):
    """the case's reads dealt to `world` shards on device 0, one step done"""
    c = vc.case(name)
    cb, umi, gene, aux, side = c.arrays()
    g = ShardGroup([0] * world, barcodes_file=c.whitelist(tmp), **c.ctx)
    bounds = even_bounds(len(cb), world)
    for i, s in enumerate(g.shards):
        if side:
            s.set_side_strings(side)
        for k, v in options:
            s.set_option(k, v)
        s.set_reads(capi.DeviceArrays.from_host(0, *[a[bounds[i]:bounds[i + 1]] for a in (cb, umi, gene, aux)]), bounds[i])
    g.step()
    return g


def requests(c):
    return [(lo, hi, n) for lo, hi, n, _, _ in c.samples], max(cap for _, _, _, cap, _ in c.samples)


def debug_keys(shard, which):
    L = capi.lib()
    L.dropest_test_validation_keys.restype = C.c_int
    L.dropest_test_validation_keys.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.c_void_p]
    n = C.c_uint64()
    assert L.dropest_test_validation_keys(shard.h, which, C.byref(n), None) == 0
    out = np.zeros(n.value, np.uint64)
    assert L.dropest_test_validation_keys(shard.h, which, C.byref(n), out.ctypes.data) == 0
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """(case, world) -> what one group call over all the case's samples gave, computed once"""
    tmp = tmp_path_factory.mktemp("validation_sharded")
    made = {}

    def get(name, world):
        if (name, world) not in made:
            c = vc.case(name)
            g = make_group(name, world, tmp, options=(("keep_validation_keys", 1),))
            try:
                samples, cap = requests(c)
                got = g.merge_validation(*samples, max_draws=cap)
                made[(name, world)] = dict(
                    samples=[{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()} for s in got],
                    col_barcode=[capi.unpack_code(int(b), c.arrays()[4]) for b in g.shards[0].matrix(True)[3]],
                    owned=[len(s.ctx.filtered_cells()) for s in g.shards],
                    local_keys=[debug_keys(s, 0) for s in g.shards], placed=[debug_keys(s, 1) for s in g.shards])
            finally:
                g.close()
        return made[(name, world)]

    return get


def one_context(st, samples, cap):
    """the one context's dicts, as a list whatever the number of samples"""
    one = st.ctx.merge_validation(*samples, max_draws=cap)
    return [one] if isinstance(one, dict) else one


def mapped(sample, col_barcode, st):
    """a sharded sample with the one context's cell ids in cell1 / cell2"""
    id_of = {b: i for i, b in st.barcode.items()}
    out = dict(sample)
    for k in ("cell1", "cell2"):
        out[k] = np.array([id_of[col_barcode[int(x)]] for x in sample[k]], np.uint64)
    return out


# ---- every case at worlds 2 and 3 against one context and the model -----------------------------------------------------------------------
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", CASES)
def test_group_equals_one_context(states, runs, name, world):
    st = states(name)
    run = runs(name, world)
    assert run["col_barcode"] == [st.barcode[i] for i in st.filtered]           # the columns are the one context's filtered cells, in its order
    assert sum(run["owned"]) == len(st.filtered)
    samples, cap = requests(st.case)
    one = one_context(st, samples, cap)
    for got, ref, (lo, hi, n) in zip(run["samples"], one, samples):
        m = mapped(got, run["col_barcode"], st)
        for k in INT_KEYS:
            assert np.array_equal(m[k], ref[k]), (name, world, k)
        assert (m["n_found"], m["draws_used"], m["complete"]) == (ref["n_found"], ref["draws_used"], ref["complete"])
        assert m["rounds"] == ref.get("rounds", m["rounds"])                    # (one sample alone goes through the call that does not report them)
        if len(st.filtered) < 2:
            assert (m["n_found"], m["complete"], m["draws_used"]) == (0, 0, 0)
            continue
        if name in PLAIN_VIEW:
            same_bits(m, ref)                                                   # expected / probability included
        st.check(m, lo, hi, n, cap)                                             # integers equal to the model's, reals within DEVICE_FACTOR x D


@pytest.mark.parametrize("name", ["n_umis", "directional"])
def test_rewritten_groups_do_not_depend_on_the_world(runs, name):
    for a, b in zip(runs(name, 2)["samples"], runs(name, 3)["samples"]):
        same_bits(a, b)
    assert runs(name, 2)["col_barcode"] == runs(name, 3)["col_barcode"]


# ---- the partition ------------------------------------------------------------------------------------------------------------------------
def test_a_shard_without_filtered_cells(runs):
    owned = {name: runs(name, 3)["owned"] for name in CASES}
    print(owned)
    assert any(0 in o for o in owned.values())
    assert 0 in owned["one_cell"] and owned["no_cell"] == [0, 0, 0]


def test_a_shard_without_filtered_cells_in_a_full_view(states, tmp_path):
    """few_adjacent has 12 cells: the smallest world at which some shard owns none of them, so that the view is gathered from blocks of which
    one is empty"""
    st = states("few_adjacent")
    codes = [capi.pack_seq(st.barcode[i]) for i in st.filtered]
    assert None not in codes
    world = next((w for w in range(3, 13) if len({capi.lib().dropest_owner_of(c, w) for c in codes}) < w), None)
    assert world is not None
    lo, hi, n, cap, _ = st.case.samples[0]
    g = make_group("few_adjacent", world, tmp_path)
    try:
        assert 0 in [len(s.ctx.filtered_cells()) for s in g.shards]
        got = g.merge_validation(lo, hi, n, max_draws=cap)
        col = [capi.unpack_code(int(b)) for b in g.shards[0].matrix(True)[3]]
    finally:
        g.close()
    same_bits(mapped(got, col, st), st.ctx.merge_validation(lo, hi, n, max_draws=cap))


def test_every_shard_evaluates_pairs_of_planted(states, runs):
    st = states("planted")
    lo, hi, n, cap, _ = st.case.samples[0]
    got = runs("planted", 3)["samples"][0]
    m = mapped(got, runs("planted", 3)["col_barcode"], st)
    common = [len(st.container[int(a)].keys() & st.container[int(b)].keys()) for a, b in zip(m["cell1"], m["cell2"])]
    bounds = capi.validation_cut_pairs(common, 3)
    assert all(b > a for a, b in zip(bounds, bounds[1:])), bounds
    assert got["chunks"] == 3                                                    # one chunk per shard under the default budget


# ---- the chunk budget inside a shard's range ----------------------------------------------------------------------------------------------
def test_chunk_budget(runs, tmp_path):
    c = vc.case("planted")
    samples, cap = requests(c)
    base = runs("planted", 2)["samples"]
    g = make_group("planted", 2, tmp_path)
    try:
        for budget in (1, 64):
            got = g.merge_validation(*samples, max_draws=cap, max_keys_per_chunk=budget)
            for a, b in zip(got, base):
                same_bits(a, b)
            assert got[0]["chunks"] > base[0]["chunks"]
    finally:
        g.close()


# ---- a split context ----------------------------------------------------------------------------------------------------------------------
def test_split_context(states):
    st = states("planted")
    c = st.case
    cb, umi, gene, aux, side = c.arrays()
    samples, cap = requests(c)
    ctx = capi.Context(**c.ctx)
    ctx.set_side_strings(side)
    ctx.push_reads(cb, umi, gene, aux)
    g = ShardGroup.split(ctx, 2)
    try:
        with pytest.raises(capi.DropestError) as e:                              # before a step
            g.merge_validation(*samples, max_draws=cap)
        assert e.value.status == 1 and "initialize" in str(e.value)
        g.step()
        got = g.merge_validation(*samples, max_draws=cap)
        col = [capi.unpack_code(int(b), side) for b in g.shards[0].matrix(True)[3]]
        for a, b in zip(got, one_context(st, samples, cap)):
            same_bits(mapped(a, col, st), b)
        with pytest.raises(capi.DropestError) as e:                              # the context-level calls refuse as before
            ctx.merge_validation(1, 1, 4)
        assert e.value.status == 4 and "split" in str(e.value)
        with pytest.raises(capi.DropestError) as e:
            g.shards[0].ctx.merge_validation(1, 1, 4)
        assert e.value.status == 4 and "shard" in str(e.value)
    finally:
        g.close()
        ctx.close()


# ---- call order and mismatched calls ------------------------------------------------------------------------------------------------------
def test_before_a_step():
    c = vc.case("planted")
    g = ShardGroup([0, 0], **c.ctx)
    try:
        with pytest.raises(capi.DropestError) as e:
            g.merge_validation(1, 1, 4)
        assert e.value.status == 1
        with pytest.raises(capi.DropestError) as e:                              # no collective in front of the refusal: one shard alone returns
            g.shards[1].merge_validation(1, 1, 4)
        assert e.value.status == 1
    finally:
        g.close()


def test_mismatched_calls_are_refused_on_every_shard(runs, tmp_path):
    g = make_group("planted", 2, tmp_path)
    try:
        raised = [None, None]

        def call(i, n_pairs):
            try:
                g.shards[i].merge_validation(1, 1, n_pairs, max_draws=1 << 16)
            except capi.DropestError as e:
                raised[i] = e.status

        threads = [threading.Thread(target=call, args=(i, n)) for i, n in ((0, 8), (1, 9))]
        for t in threads:
            t.start()
        for t in threads:
            t.join(60)
        assert not any(t.is_alive() for t in threads), "a shard is still waiting for its peer"
        assert raised == [1, 1]
        # nobody was left inside a collective: the group still works
        samples, cap = requests(vc.case("planted"))
        for a, b in zip(g.merge_validation(*samples, max_draws=cap), runs("planted", 2)["samples"]):
            same_bits(a, b)
    finally:
        g.close()


# ---- the place kernel alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", WORLDS)
def test_placed_keys_are_the_sorted_union(runs, world):
    run = runs("planted", world)
    union = np.sort(np.concatenate(run["local_keys"]))
    assert len(union) > 500 and sum(1 for k in run["local_keys"] if len(k)) == world
    for placed in run["placed"]:                                                 # every shard holds the same view
        assert np.array_equal(placed, union)
    assert np.all(union[1:] > union[:-1])                                        # a molecule is one (cell, gene, UMI)
    # not one block after the other: the cells of the shards interleave in the global order
    first = np.concatenate(run["local_keys"])
    assert not np.array_equal(first, union)


def test_cells_larger_than_a_piece_of_the_place_kernel(tmp_path):
    """The place kernel cuts a cell's rows into pieces of 4096 (VAL_SEG, k_validation.h) and copies 16 bytes per lane where source and
    destination sit alike in their 16-byte lines, 8 otherwise: two cells of more than two pieces each, with odd row counts in front of
    and inside them, beside small cells -- against one context on the same reads, and the placed keys against the sorted union."""
    import random
    from collections import Counter
    rng = random.Random(23)
    barcodes = vc.planted_barcodes()[0][:7]
    mol = []
    for c in range(len(barcodes)):
        for g in range(6):
            k = {(1, 0): 5001, (1, 3): 4100, (4, 2): 9001}.get((c, g), 19 + c + g)
            seen = set()
            while len(seen) < k:
                seen.add(vc.rnd_seq(rng, 8))
            mol += [(c, g, u, 1) for u in sorted(seen)]
    assert sorted(Counter(c for c, _, _, _ in mol).values())[-2] > 2 * 4096
    case = vc.Case("large_cells", barcodes, mol, vc.PLAIN, [vc.DISTANT + (40, 1 << 14, False), vc.ADJACENT + (8, 1 << 14, False)])
    cb, umi, gene, aux, side = case.arrays()
    samples, cap = requests(case)
    ctx = capi.Context(**case.ctx)
    g = ShardGroup([0, 0, 0], **case.ctx)
    try:
        if side:
            ctx.set_side_strings(side)
        ctx.push_reads(cb, umi, gene, aux)
        ctx.set_initialized()
        ctx.merge_and_filter()
        rows = ctx.cell_rows()
        want = ctx.merge_validation(*samples, max_draws=cap)
        bounds = even_bounds(len(cb), 3)
        for i, s in enumerate(g.shards):
            if side:
                s.set_side_strings(side)
            s.set_option("keep_validation_keys", 1)
            s.set_reads(capi.DeviceArrays.from_host(0, *[a[bounds[i]:bounds[i + 1]] for a in (cb, umi, gene, aux)]), bounds[i])
        g.step()
        got = g.merge_validation(*samples, max_draws=cap)
        col = g.shards[0].matrix(True)[3].copy()
        assert sum(w["n_found"] for w in want) > 0 and any(int(x) for w in want for x in w["intersection"])
        for a, b in zip(got, want):
            a = dict(a)
            for k in ("cell1", "cell2"):                                         # columns -> barcodes <- cell ids
                assert np.array_equal(col[a[k].astype(np.int64)], rows["barcode"][b[k].astype(np.int64)])
                a[k] = b[k]
            same_bits(a, b)
        union = np.sort(np.concatenate([debug_keys(s, 0) for s in g.shards]))
        assert len(union) == len(mol)
        for s in g.shards:
            assert np.array_equal(debug_keys(s, 1), union)
        assert np.all(union[1:] > union[:-1])
    finally:
        g.close()
        ctx.close()
