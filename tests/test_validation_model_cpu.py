"""Pins tests/validation_model.py -- the plain-Python restatement of `dropest -S` that test_gpu_validation.py compares the device with --
on the CPU checker, shows what the planted barcodes are there for, and shows that every sample of validation_cases.py that is meant to
complete does so under the model inside its cap on draws.  No GPU."""
import ctypes
import random

import pytest

from dropest_amd import capi
from oracle import Oracle
from oracle import binding as ob

import validation_cases as vc
import validation_model as vm
import whitelist_cases as wc


# ---- the banded distance -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band", [1, 5])
@pytest.mark.parametrize("n_side", ["none", "first", "second", "both"])
def test_banded_distance_equals_the_checker(band, n_side):
    rng = random.Random(100 * band + ["none", "first", "second", "both"].index(n_side))
    differs = 0
    for k in range(1500):
        la, lb = rng.randint(4, 16), rng.randint(4, 16)
        a = vc.rnd_seq(rng, la)
        if k % 3 == 0:                                              # a relative: substitutions, then an insertion or a deletion
            b = wc.substitute(rng, a, rng.randint(0, 3))
            if k % 2:
                i = rng.randrange(len(b))
                b = b[:i] + b[i + 1:] if k % 4 == 1 else b[:i] + rng.choice("ACGT") + b[i:]
        elif k % 3 == 1:                                            # a shifted copy: the optimal path leaves a narrow band
            s = rng.randint(1, 4)
            b = a[s:] + vc.rnd_seq(rng, s)
        else:
            b = vc.rnd_seq(rng, lb)
        if n_side in ("first", "both"):
            a = wc.with_n(a, rng.sample(range(len(a)), rng.randint(1, 2)))
        if n_side in ("second", "both") and b:
            b = wc.with_n(b, rng.sample(range(len(b)), min(len(b), rng.randint(1, 2))))
        got = vm.edit_distance(a, b, True, band)
        assert got == ob.edit_distance(a, b, True, band), (a, b, band)
        differs += got != vm.levenshtein(a, b)
    assert differs > 100                                            # the band matters on these inputs


def test_unbounded_band_is_levenshtein():
    rng = random.Random(3)
    for _ in range(300):
        a, b = vc.rnd_seq(rng, rng.randint(4, 16)), vc.rnd_seq(rng, rng.randint(4, 16))
        assert vm.edit_distance(a, b, True, 10000) == vm.levenshtein(a, b) == ob.edit_distance(a, b)


@pytest.mark.parametrize("a, b, band, banded, full", [
    # three bases rotated to the end: three deletions and three insertions for Levenshtein; row 1 of a band of 1 already has no
    # cell under 2 -- the function returns that row's minimum
    ("ACGTTGCAAGCT", "TTGCAAGCTACG", 1, 2, 6),
    # the same under a band of 5: the path along the third diagonal fits, the value is Levenshtein's
    ("ACGTTGCAAGCT", "TTGCAAGCTACG", 5, 6, 6),
    # a stranger under a band of 1: the early return reports a row minimum, far below the distance
    ("AAAAAAAAAAAA", "CCCCCCCCCCCC", 1, 2, 12),
    # under a band of 5 the return comes at the row where every cell plus its distance from the diagonal passes 5
    ("AAAAAAAAAAAA", "CCCCCCCCCCCC", 5, 6, 12),
    # N on either side matches anything
    ("ACGTNCGTACGT", "ACGTACGTACGT", 1, 0, 0),
    ("ACGTACGTACGT", "ACNTACGTACGA", 1, 1, 1),
    # unequal lengths.  The last base missing: the path stays on the diagonal until the last row.  A base missing in the middle:
    # from there on the path runs beside the diagonal, where a cell counts with its offset -- 1 + 1 -- and the band of 1 ends it
    ("ACGTACGTACGT", "ACGTACGTACG", 1, 1, 1),
    # ... and the same pair the other way round: the last row has no cell inside the band (the longer string is s2), its minimum is
    # the row number itself, and that is what comes back
    ("ACGTACGTACG", "ACGTACGTACGT", 1, 12, 1),
    ("ACGTACGTACGT", "ACGTAGTACGT", 1, 2, 1),
    ("ACGTAGTACGT", "ACGTACGTACGT", 1, 2, 1),
    ("ACGTACGTACGT", "ACGTAGTACGT", 5, 1, 1),
])
def test_hand_cases_where_the_band_cuts_the_path(a, b, band, banded, full):
    assert vm.levenshtein(a, b) == full
    assert vm.edit_distance(a, b, True, band) == banded == ob.edit_distance(a, b, True, band)


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------
SIX = {0: "AAAAAAAA", 1: "AAAAAAAC", 2: "CCCCCCCC", 3: "CCCCCCCG", 4: "GGGGTTTT", 5: "NGGGTTTT"}


def _rand_pairs(f, count):
    libc = ctypes.CDLL("libc.so.6")
    libc.srand(42)
    return [(libc.rand() % f, libc.rand() % f) for _ in range(count)]


def test_sampler_on_six_cells():
    """Six filtered cells 0 .. 5 (their order is their id): (0, 1) and (2, 3) are one substitution apart, 5 is 4 with an N for its
    first base (distance 0), every other pair is strangers (all eight bases differ; the banded function returns 2 for them under a band
    of 1 and 6 under a band of 5).  So the adjacent sample (1, 1) takes exactly the candidates (0, 1), (1, 0), (2, 3), (3, 2); the distant
    sample (5, 100) takes every candidate of two different cells except those four and (4, 5), (5, 4); a candidate of twice the same
    cell is skipped by both before any distance.  Which candidates come is libc's rand() after srand(42), two values per candidate;
    the test replays that sequence and applies the rule above."""
    order = sorted(SIX)
    adjacent_pairs = {(0, 1), (1, 0), (2, 3), (3, 2)}
    wild = {(4, 5), (5, 4)}
    cand = _rand_pairs(6, 4000)
    want_adj = [p for p in cand if p in adjacent_pairs]
    want_far = [p for p in cand if p[0] != p[1] and p not in adjacent_pairs and p not in wild]
    s = vm.run_validation(order, SIX.get, 1, 1, 20, 4000)
    assert s.complete and s.pairs() == want_adj[:20] and s.edit_distance == [1] * 20
    assert s.draws_used == [i for i, p in enumerate(cand) if p in adjacent_pairs][19] + 1
    d = vm.run_validation(order, SIX.get, 5, 100, 50, 4000)
    assert d.complete and d.pairs() == want_far[:50] and d.edit_distance == [6] * 50
    assert vm.levenshtein(SIX[0], SIX[2]) == 8                      # recorded: the banded function's value, not the distance
    # both samples restart the rand() sequence: the distant one run first, or not at all, does not move the adjacent one
    again = vm.run_validation(order, SIX.get, 1, 1, 20, 4000)
    assert again.pairs() == s.pairs() and again.draws_used == s.draws_used
    # the cap: 30 draws hold fewer than 20 adjacent candidates
    capped = vm.run_validation(order, SIX.get, 1, 1, 20, 30)
    assert not capped.complete and capped.draws_used == 30 and capped.pairs() == [p for p in cand[:30] if p in adjacent_pairs]
    # F < 2
    assert vm.run_validation([3], SIX.get, 1, 1, 5, 100).n_found == 0 and vm.run_validation([], SIX.get, 1, 1, 5, 100).draws_used == 0


def test_library_exports_the_validation_entries():
    L = capi.lib()
    for name in ("dropest_merge_validation", "dropest_merge_validation_samples"):
        assert hasattr(L, name), name
        assert name in capi.EXPORTED_SYMBOLS
    assert hasattr(capi.Context, "merge_validation")


# ---- the cases of the GPU tests under the model --------------------------------------------------------------------------------------
def _checker_state(c, tmp_path):
    cb, umi, gene, aux, side = c.arrays()
    o = Oracle(**c.checker_kw(c.whitelist(tmp_path)))
    o.add_packed(cb, umi, gene, aux, side)
    o.set_initialized()
    if c.merge:
        o.merge_and_filter()
    filtered = [int(x) for x in o.filtered_cells()]
    return o, filtered, {i: o.cell_barcode(i) for i in filtered}


@pytest.mark.parametrize("name", vc.NAMES)
def test_every_case_ends_as_it_is_meant_to_within_its_cap(name, tmp_path):
    c = vc.case(name)
    _, filtered, barcode = _checker_state(c, tmp_path)
    for lo, hi, n, cap, complete in c.samples:
        s = vm.run_validation(filtered, barcode.get, lo, hi, n, cap)
        assert s.complete == complete, (name, lo, hi, n, s.n_found, s.draws_used)
        if complete:
            assert s.draws_used * 4 <= cap                          # nowhere near the cap
    if name == "few_adjacent":
        assert 0 < s.n_found < n
    if name in ("one_cell", "no_cell"):
        assert len(filtered) == (1 if name == "one_cell" else 0)


def test_planted_barcodes_are_what_they_are_planted_for(tmp_path):
    c = vc.case("planted")
    assert sorted(set(len(b) for b in c.barcodes)) == [11, 12] and len(c.barcodes) == 24
    _, filtered, barcode = _checker_state(c, tmp_path)
    assert sorted(filtered) == list(range(24))
    r = c.roles
    band = lambda a, b, k: vm.edit_distance(barcode[a], barcode[b], True, k)
    for k in ("sub0", "sub1", "sub2"):
        a, b = r[k]
        assert band(a, b, 1) == band(b, a, 1) == 1, k
    a, b = r["indel"]                                               # adjacent with the longer barcode first only (see the hand cases)
    assert len(barcode[a]) == 12 and len(barcode[b]) == 11 and band(a, b, 1) == 1 and band(b, a, 1) == 12
    a, b = r["n"]
    assert "N" in barcode[b] and band(a, b, 1) == band(b, a, 1) == 0 and band(a, b, 5) == 0
    rejected = [(r["near"][0], r["near"][1]), (r["near"][0], r["near"][2]), tuple(r["near4"])]
    assert [vm.levenshtein(barcode[a], barcode[b]) for a, b in rejected] == [2, 3, 4]
    for a, b in rejected:                                           # too far for the adjacent sample, too near for the distant one
        assert band(a, b, 1) > 1 and band(a, b, 5) < 5
    a, b = r["rotated"]
    assert band(a, b, 5) >= 5
    (lo, hi, n, cap, _), (lo2, hi2, n2, cap2, _) = c.samples
    distant, adjacent = vm.run_validation(filtered, barcode.get, lo, hi, n, cap), vm.run_validation(filtered, barcode.get, lo2, hi2, n2, cap2)
    seen = {frozenset(p) for p in adjacent.pairs()}
    assert seen == {frozenset(r[k]) for k in ("sub0", "sub1", "sub2", "indel")}
    assert tuple(r["indel"]) in adjacent.pairs() and tuple(reversed(r["indel"])) not in adjacent.pairs()
    far = {frozenset(p) for p in distant.pairs()}
    assert not far & (seen | {frozenset(r["n"])} | {frozenset(p) for p in rejected})
    off = [e for (a, b), e in zip(distant.pairs(), distant.edit_distance) if e != vm.levenshtein(barcode[a], barcode[b])]
    assert len(off) >= 10                                           # recorded values that are not Levenshtein distances
