"""The tagged-BAM model (tests/bam_tag_model.py) pinned on hand-built records: the expected output bytes stand here literally, worked out by hand
from the edit rule of DESIGN.md §7 (BamProcessorAbstract::save_alignment, BamProcessorAbstract.cpp:65-114).  The GPU tests compare the device's
output with this model, so the model itself is checked against nothing but these bytes."""
import struct

import pytest

import bam_model as bm
import bam_tag_model as tm

# refID 0, pos 7, l_read_name, mapq 255, bin 4680, no CIGAR, flag, no bases, no mate, tlen 0: the 32 fixed bytes of a record
def _fixed(l_read_name, flag=0):
    return (b"\x00\x00\x00\x00" b"\x07\x00\x00\x00" + bytes([l_read_name]) + b"\xff" b"\x48\x12" b"\x00\x00" + struct.pack("<H", flag) + b"\x00\x00\x00\x00"
            b"\xff\xff\xff\xff" b"\xff\xff\xff\xff" b"\x00\x00\x00\x00")


def _rec(name, aux, flag=0):
    body = _fixed(len(name) + 1, flag) + name + b"\x00" + aux
    return struct.pack("<I", len(body)) + body


FILLED = bm.Cfg(tags=("CB", "UB", "CQ", "UQ", "GX", "RE"), filled_bam=True, read_type=True, intronic=b"N", intergenic=b"I", n_refs=1)
NAME = bm.Cfg(tags=("CB", "UB", "CQ", "UQ", "GX", "RE"), filled_bam=False, read_type=True, intronic=b"N", intergenic=b"I", n_refs=1)
TYPED = tm.OutCfg(read_type="RE", exonic=b"E", intronic=b"N", intergenic=b"I")
PLAIN = tm.OutCfg()
CB, UB, GX, NH = b"CBZACGT\x00", b"UBZTTGA\x00", b"GXZG1\x00", b"NHi\x01\x00\x00\x00"
CR, UR = b"CRZACGT\x00", b"URZTTGA\x00"

CASES = {
    # an edited tag first, in the middle, last: the entry goes, the tag is appended (no gene: only CR and UR are edited)
    "edited tag first": (FILLED, PLAIN, b"CRZold\x00" + CB + UB + NH, CB + UB + NH + CR + UR),
    "edited tag in the middle": (FILLED, PLAIN, CB + b"URZxx\x00" + UB + GX, CB + UB + b"GXZG1\x00" + CR + UR),
    "edited tag last": (FILLED, PLAIN, CB + UB + NH + b"URZq\x00", CB + UB + NH + CR + UR),
    # the read type: RE:A:E is an exonic read (neither the intronic N nor the intergenic I); the A entry goes, RE:Z:E is appended last
    "RE:A:E becomes RE:Z:E": (FILLED, TYPED, CB + UB + GX + b"REAE", CB + UB + b"GXZG1\x00" + CR + UR + b"REZE\x00"),
    "RE:A:N is intronic": (FILLED, TYPED, CB + b"REAN" + UB + GX, CB + UB + b"GXZG1\x00" + CR + UR + b"REZN\x00"),
    "no gene is intergenic": (FILLED, TYPED, CB + UB, CB + UB + CR + UR + b"REZI\x00"),
    "no read-type tag configured": (FILLED, PLAIN, CB + UB + GX + b"REAE", CB + UB + b"REAE" + b"GXZG1\x00" + CR + UR),
    # CQ is there but empty: not edited, so it stays where it is; UQ has a value: dropped and appended
    "empty CQ stays in place": (FILLED, PLAIN, CB + UB + b"CQZ\x00" + b"UQZIIII\x00", CB + UB + b"CQZ\x00" + CR + UR + b"UQZIIII\x00"),
    "UQ without CQ": (FILLED, PLAIN, b"UQZ#5\x00" + CB + UB, CB + UB + CR + UR + b"UQZ#5\x00"),
    "both qualities": (FILLED, PLAIN, CB + b"CQZFF\x00" + UB + b"UQZ,,\x00", CB + UB + CR + UR + b"CQZFF\x00" + b"UQZ,,\x00"),
    # every occurrence of an edited name goes, whatever its type
    "repeated CR": (FILLED, PLAIN, b"CRZa\x00" + CB + b"CRi\x01\x00\x00\x00" + UB + b"CRZb\x00", CB + UB + CR + UR),
    # the walk stops at the unknown type '?': what follows is not looked at (the CR behind it stays) and the new tags come after it
    "walk stops at an unknown type": (FILLED, PLAIN, CB + UB + b"CRZzz\x00" + b"XX?" + b"CRZyy\x00", CB + UB + b"XX?" + b"CRZyy\x00" + CR + UR),
    "string without its NUL": (FILLED, PLAIN, CB + UB + b"URZq\x00" + b"CRZnever ends", CB + UB + b"CRZnever ends" + CR + UR),
    # a B array whose payload reads "CRZ\0": the walk goes by type, the array is kept whole
    "CRZ inside a B:C payload": (FILLED, PLAIN, CB + b"XBBC\x04\x00\x00\x00CRZ\x00" + UB, CB + b"XBBC\x04\x00\x00\x00CRZ\x00" + UB + CR + UR),
    "N in the UMI, lower case in the barcode": (FILLED, PLAIN, b"CBZacgN\x00" + b"UBZTNGA\x00", b"CBZacgN\x00" + b"UBZTNGA\x00" + b"CRZacgN\x00" + b"URZTNGA\x00"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_hand_built_records(case):
    cfg, out_cfg, aux_in, aux_out = CASES[case]
    assert tm.tagged_record(_rec(b"read1", aux_in), cfg, out_cfg) == _rec(b"read1", aux_out)


def test_no_aux_data_whole_record_literally():
    """name mode: no '!' .. '#' no record; with them, barcode and UMI come from the name -- the whole output record, every byte written out"""
    rec = _rec(b"r!AC#GT", b"")
    assert rec == (b"\x28\x00\x00\x00" b"\x00\x00\x00\x00\x07\x00\x00\x00\x08\xff\x48\x12\x00\x00\x00\x00\x00\x00\x00\x00\xff\xff\xff\xff\xff\xff\xff\xff\x00\x00\x00\x00" b"r!AC#GT\x00")
    assert tm.tagged_record(rec, NAME, TYPED) == (b"\x39\x00\x00\x00" b"\x00\x00\x00\x00\x07\x00\x00\x00\x08\xff\x48\x12\x00\x00\x00\x00\x00\x00\x00\x00\xff\xff\xff\xff\xff\xff\xff\xff\x00\x00\x00\x00"
                                                 b"r!AC#GT\x00" b"CRZAC\x00" b"URZGT\x00" b"REZI\x00")
    assert tm.tagged_record(rec, FILLED, TYPED) is None                    # -f: no CB tag, the record cannot be parsed and is not written


def test_name_with_two_separators_each():
    """x#y!AC#GT: the last '#', then the last '!' at or before it"""
    assert tm.tagged_record(_rec(b"x#y!AC#GT", NH), NAME, PLAIN) == _rec(b"x#y!AC#GT", NH + b"CRZAC\x00" + b"URZGT\x00")
    # quality tags are not read in name mode: CQ / UQ stay where they are
    assert tm.tagged_record(_rec(b"x#y!AC#GT", b"UQZII\x00" + GX), NAME, PLAIN) == _rec(b"x#y!AC#GT", b"UQZII\x00" + b"GXZG1\x00" + b"CRZAC\x00" + b"URZGT\x00")


def test_gene_and_mark_given_by_the_caller():
    """-g: the annotation's gene replaces the gene tag's; a spanning mark (exons and introns) writes no read type, so the RE entry stays"""
    rec = _rec(b"read1", CB + UB + GX + b"REAE")
    assert tm.tagged_record(rec, FILLED, TYPED, gene_name=b"GA", mark=6) == _rec(b"read1", CB + UB + b"REAE" + b"GXZGA\x00" + CR + UR)
    assert tm.tagged_record(rec, FILLED, TYPED, gene_name=b"", mark=1) == _rec(b"read1", CB + UB + GX + CR + UR + b"REZI\x00")      # no gene: GX is not edited
    assert tm.tagged_record(rec, FILLED, TYPED, gene_name=b"GA", mark=4) == _rec(b"read1", CB + UB + b"GXZGA\x00" + CR + UR + b"REZN\x00")


def test_records_that_are_not_written():
    assert tm.tagged_record(_rec(b"read1", CB + UB, flag=4), FILLED, PLAIN) is None            # unmapped: skipped
    assert tm.tagged_record(_rec(b"read1", CB + UB, flag=0x100), FILLED, PLAIN) is None        # not primary
    assert tm.tagged_record(_rec(b"read1", CB), FILLED, PLAIN) is None                         # no UMI: cannot be parsed
    low = bm.Cfg(tags=FILLED.tags, filled_bam=True, min_phred=33 + 20, n_refs=1)
    assert tm.tagged_record(_rec(b"read1", CB + UB + b"UQZI#\x00"), low, PLAIN) is None        # '#' is below the limit
    assert tm.tagged_record(_rec(b"read1", CB + UB + b"UQZII\x00"), low, PLAIN) == _rec(b"read1", CB + UB + CR + UR + b"UQZII\x00")
    assert tm.tagged_record(_rec(b"read1", CB + UB), bm.Cfg(tags=FILLED.tags, n_refs=0), PLAIN) is None   # no such reference
