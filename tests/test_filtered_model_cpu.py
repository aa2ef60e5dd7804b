"""tests/filtered_model.py pinned on literal cases (FilteringBamProcessor.cpp:14-40, :61-96; Gene.cpp:38-58), and the -F calls of the
C-ABI exported and bound."""
import pytest

import filtered_model as fm
from dropest_amd import capi

NEW_CALLS = ["dropest_set_save_umi_merge_targets", "dropest_umi_merge_targets", "dropest_read_corrections",
             "dropest_read_corrections_host", "dropest_read_correction_counts"]


def test_the_filter_calls_are_exported_and_bound():
    L = capi.lib()
    for name in NEW_CALLS:
        assert hasattr(L, name), "missing export: " + name
        assert name in capi.EXPORTED_SYMBOLS
        assert getattr(L, name).argtypes is not None, "not bound: " + name
    for method in ("set_save_umi_merge_targets", "umi_merge_targets", "read_corrections", "read_corrections_device", "read_correction_counts"):
        assert callable(getattr(capi.Context, method))


# cells 0..4: 1 was merged into 0, 3 into 2; filtered = {0, 4}: cell 2 (and with it 3) did not pass the size threshold
MERGE_TARGETS = [0, 0, 2, 2, 4]
FILTERED = [4, 0]
MOLECULES = {(0, 7): {"AAAA": 3, "CCCC": 1}, (0, 8): {"GGGG": 2}, (4, 7): {"TTTT": 1}, (2, 7): {"AAAA": 1}}
UMI_TARGETS = {(0, 7): {"ACGT": "AAAA", "CCCC": "TTGG"}, (4, 8): {"AAAA": "CCCC"}}


def test_merge_cbs_holds_the_cells_whose_target_is_filtered():
    assert fm.merge_cbs(MERGE_TARGETS, FILTERED) == {0: 0, 1: 0, 4: 4}


@pytest.mark.parametrize("read,want", [
    ((0, None, "AAAA"), (fm.NO_GENE, None, "AAAA")),            # :63-64
    ((2, 7, "AAAA"), (fm.CELL_NOT_KEPT, None, "AAAA")),         # own target, not filtered (:66-68)
    ((3, 7, "AAAA"), (fm.CELL_NOT_KEPT, None, "AAAA")),         # merged into a cell that is not filtered
    ((0, 9, "AAAA"), (fm.WRONG_GENE, 0, "AAAA")),               # :70-76
    ((4, 8, "AAAA"), (fm.WRONG_GENE, 4, "AAAA")),               # targets recorded for a gene the cell does not hold: the gene test comes first
    ((0, 7, "AAAA"), (fm.WRITTEN, 0, "AAAA")),                  # a molecule keeps its UMI (:84-87)
    ((1, 7, "AAAA"), (fm.WRITTEN, 0, "AAAA")),                  # ... read of a merged cell: the target's barcode
    ((1, 8, "GGGG"), (fm.WRITTEN, 0, "GGGG")),
    ((0, 7, "ACGT"), (fm.WRITTEN, 0, "AAAA")),                  # a source that is no molecule any more (:79-83)
    ((0, 7, "CCCC"), (fm.WRITTEN, 0, "TTGG")),                  # a source that IS a molecule: the map wins, its target is not looked up
    ((0, 7, "TTGG"), (fm.WRONG_UMI, 0, "TTGG")),                # one hop only: a target that is neither source nor molecule (:88-92)
    ((4, 7, "AAAA"), (fm.WRONG_UMI, 4, "AAAA")),                # a molecule of another cell
    ((4, 7, "TTTT"), (fm.WRITTEN, 4, "TTTT")),
])
def test_decide_read(read, want):
    cbs = fm.merge_cbs(MERGE_TARGETS, FILTERED)
    assert fm.decide_read(read[0], read[1], read[2], cbs, MOLECULES, UMI_TARGETS) == want


def test_decide_reads_without_the_map_drops_the_reads_of_merged_umis():
    v, c, u = fm.decide_reads([0, 0, 1], [7, 7, 7], ["ACGT", "AAAA", "CCCC"], MERGE_TARGETS, FILTERED, MOLECULES, {})
    assert v == [fm.WRONG_UMI, fm.WRITTEN, fm.WRITTEN] and c == [0, 0, 0] and u == ["ACGT", "AAAA", "CCCC"]


def test_record_merges_keeps_the_last_target_and_skips_identity_pairs():
    log = [(5, 1, "AA", "CC"), (2, 9, "GG", "GG"), (5, 1, "TT", "CC"), (5, 0, "AA", "GG"), (5, 1, "AA", "TT"), (2, 9, "CC", "AA")]
    assert fm.record_merges(log) == [(2, 9, "CC", "AA"), (5, 0, "AA", "GG"), (5, 1, "AA", "TT"), (5, 1, "TT", "CC")]


def test_simple_umi_targets():
    assert fm.hamming_n("ACGN", "ACGT") == 0 and fm.hamming_n("ANGT", "CCGA") == 2
    group = {"AAACCT": 2, "AAACCG": 1, "AAACCN": 1, "CCCCCT": 1, "CNCCCT": 4, "TTTTTA": 1}
    assert fm.simple_umi_targets(group, 1) == {"AAACCN": "AAACCT", "CNCCCT": "CCCCCT"}      # more reads among equals; the smallest distance
    with pytest.raises(ValueError):
        fm.simple_umi_targets({"AAACCT": 1, "AAACCG": 1, "AAACCN": 1}, 1)                   # a tie
    with pytest.raises(ValueError):
        fm.simple_umi_targets({"AAACCT": 1, "GGGTTN": 1}, 1)                                # a random fill
