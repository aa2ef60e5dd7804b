"""The filtered-BAM model (tests/bam_filter_model.py) pinned on hand-built records: the expected output bytes stand here literally, worked out by
hand from the rule of DESIGN.md §7 (FilteringBamProcessor::write_alignment, FilteringBamProcessor.cpp:61-96, through
BamProcessorAbstract::save_alignment, BamProcessorAbstract.cpp:65-114).  The GPU tests compare the device's output with this model, so the model
itself is checked against nothing but these bytes.  And the -F calls of the C-ABI are exported."""
import pytest

import bam_filter_model as fm
import bam_model as bm
from dropest_amd import capi
from test_bam_tag_model_cpu import FILLED, NAME, _rec, CB, UB, GX, NH, CR, UR

PLAIN = fm.FilterOutCfg()
TYPED = fm.FilterOutCfg(read_type="RE", exonic=b"E", intronic=b"N", intergenic=b"I")

NEW_CALLS = ["dropest_bam_decoder_set_filtering", "dropest_bam_decoder_filter_window", "dropest_cell_barcodes_device"]


def test_the_filtered_bam_calls_are_exported():
    L = capi.lib()
    for name in NEW_CALLS:
        assert hasattr(L, name), "missing export: " + name
    assert "dropest_cell_barcodes_device" in capi.EXPORTED_SYMBOLS
    assert L.dropest_cell_barcodes_device.argtypes is not None
    assert callable(capi.Context.cell_barcodes_device)


CASES = {
    # -f: the input's CB / UB are the raw strings: they become CR / UR, their entries go, and the corrected pair is appended last
    "CB and UB become CR and UR and are replaced": (FILLED, PLAIN, CB + UB + NH, b"ACGG", b"TTGC",
                                                    NH + CR + UR + b"CBZACGG\x00" + b"UBZTTGC\x00"),
    # an empty corrected UMI edits no UB: the input's entry stays where it is
    "an empty corrected UMI leaves UB alone": (FILLED, PLAIN, CB + UB + GX, b"ACGG", b"",
                                               UB + b"GXZG1\x00" + CR + UR + b"CBZACGG\x00"),
    # ... and so does an empty corrected barcode for CB
    "an empty corrected barcode leaves CB alone": (FILLED, PLAIN, CB + UB, b"", b"TTGC",
                                                   CB + CR + UR + b"UBZTTGC\x00"),
    # the two new tags stand behind the read type
    "behind the read type": (FILLED, TYPED, CB + UB + GX + b"REAE", b"ACGG", b"TTGC",
                             b"GXZG1\x00" + CR + UR + b"REZE\x00" + b"CBZACGG\x00" + b"UBZTTGC\x00"),
    # strings are written as they stand: a side string with N, a barcode longer than a code holds
    "N and a long barcode": (FILLED, PLAIN, CB + UB, b"ACGTNACGTACGTACGTACGTACGTACGTACGTAC", b"TNGA",
                             CR + UR + b"CBZACGTNACGTACGTACGTACGTACGTACGTACGTAC\x00" + b"UBZTNGA\x00"),
    # every CB the walk reaches goes, whatever its type; the one behind the unknown type '?' is not looked at
    "repeated CB and the end of the walk": (FILLED, PLAIN, CB + b"CBi\x01\x00\x00\x00" + UB + b"XX?" + b"CBZyy\x00", b"ACGG", b"TTGC",
                                            b"XX?" + b"CBZyy\x00" + CR + UR + b"CBZACGG\x00" + b"UBZTTGC\x00"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_hand_built_records(case):
    cfg, out_cfg, aux_in, cb, umi, aux_out = CASES[case]
    assert fm.filtered_record(_rec(b"read1", aux_in), cfg, out_cfg, 0, cb, umi) == _rec(b"read1", aux_out)


def test_name_mode_whole_record_literally():
    rec = _rec(b"r!AC#GT", b"")
    assert fm.filtered_record(rec, NAME, TYPED, 0, b"AA", b"GT") == (
        b"\x45\x00\x00\x00" b"\x00\x00\x00\x00\x07\x00\x00\x00\x08\xff\x48\x12\x00\x00\x00\x00\x00\x00\x00\x00\xff\xff\xff\xff\xff\xff\xff\xff\x00\x00\x00\x00"
        b"r!AC#GT\x00" b"CRZAC\x00" b"URZGT\x00" b"REZI\x00" b"CBZAA\x00" b"UBZGT\x00")


@pytest.mark.parametrize("verdict", [1, 2, 3, 4])
def test_a_verdict_that_is_not_written_gives_nothing(verdict):
    assert fm.filtered_record(_rec(b"read1", CB + UB + GX), FILLED, PLAIN, verdict, b"ACGG", b"TTGC") is None


def test_a_record_that_is_not_accepted_gives_nothing():
    assert fm.filtered_record(_rec(b"read1", CB + UB, flag=4), FILLED, PLAIN, 0, b"ACGG", b"TTGC") is None
    assert fm.filtered_record(_rec(b"read1", CB), FILLED, PLAIN, 0, b"ACGG", b"TTGC") is None


def test_other_names_for_the_corrected_tags():
    out = fm.FilterOutCfg(cell_barcode="XC", umi="")                     # a tag without a name is never written and drops nothing
    assert fm.filtered_record(_rec(b"read1", CB + UB), FILLED, out, 0, b"ACGG", b"TTGC") == _rec(b"read1", CB + UB + CR + UR + b"XCZACGG\x00")


def test_codes_are_spelled_first_base_most_significant():
    assert fm.pack_code(b"ACGT") == 0b1_00_01_10_11 and fm.code_string(0b1_00_01_10_11, []) == b"ACGT"
    assert fm.code_string(1, []) == b"" and fm.code_string(0, []) == b""
    assert fm.code_string(fm.pack_code(b"T" * 31), []) == b"T" * 31
    assert fm.code_string((1 << 63) | 1, [b"x", b"ACNT"]) == b"ACNT"


def test_a_stream_takes_its_decisions_by_accepted_record():
    recs = [_rec(b"a", CB + UB), _rec(b"b", CB + UB, flag=4), _rec(b"c", CB + UB), _rec(b"d", CB + UB)]
    decisions = [(0, b"AA", b"CC"), (2, b"", b"TTGA"), (0, b"GG", b"")]
    got, written, used = fm.filtered_stream(recs, FILLED, PLAIN, decisions)
    assert (written, used) == (2, 3)
    assert got == _rec(b"a", CR + UR + b"CBZAA\x00" + b"UBZCC\x00") + _rec(b"d", UB + CR + UR + b"CBZGG\x00")
