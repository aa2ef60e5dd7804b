"""The reference model of a BAM record (tests/bam_model.py) on hand-worked records, each pinned to the rule it restates -- so that the model the
device decoder is held to is itself checked without a GPU.  Also: the writer's output back through gzip and the model's pure-Python record walk."""
import gzip
import struct

import pytest

import bam_model as bm
import bam_writer as bw

CFG = bm.Cfg(tags=("CB", "UB", "CY", "UY", "GX", "RE"), filled_bam=True, min_phred=0, read_type=True, intronic=b"N", intergenic=b"I", n_refs=3)
FULL = bm.Dicts(genes={bm.fnv1a(b"G1"): 7, bm.fnv1a(b"G2"): 8}, chr_of_ref=[5, 6, 4], names=None)
EMPTY = bm.Dicts(genes={}, chr_of_ref=[-1, -1, -1])
CB, UMI = "ACGTACGTACGT", "GGCCAATT"


def rec(tags, ref=0, flag=0, name="r1", **kw):
    return bw.record(ref, 10, name, flag=flag, tags=tags, **kw)


def row(tags, cfg=CFG, dicts=FULL, **kw):
    return bm.parse_record(rec(tags, **kw), cfg, dicts)


def base(**extra):
    t = [("CB", "Z", CB), ("UB", "Z", UMI), ("GX", "Z", "G1")]
    return t + list(extra.get("more", []))


def test_accepted_record_columns():
    r = row(base())
    assert (r.status, r.cb, r.umi, r.gene) == (bm.OK, bm.pack(CB.encode()), bm.pack(UMI.encode()), 7)
    assert r.aux == (bm.HAS_EXONS << 16) | 5 and r.need == 2                 # no read-type tag: HAS_EXONS (ReadParamsParser.cpp:67-90); chr touched
    assert r.cb == (1 << 24) | 0x1B1B1B                                   # 12 bases, two bits each (A C G T = 0 1 2 3), behind a leading 1


@pytest.mark.parametrize("flag,status", [(0x4, bm.SKIP), (0x100, bm.SKIP), (0x104, bm.SKIP), (0x800, bm.OK), (0x10, bm.OK), (0x200, bm.OK)])
def test_flags(flag, status):
    # BamController.cpp:87-88: unmapped (0x4) and secondary (0x100) are skipped; supplementary (0x800) is not
    assert row(base(), flag=flag).status == status


@pytest.mark.parametrize("ref,status", [(-1, bm.CANT_PARSE_NO_COUNT), (3, bm.CANT_PARSE_NO_COUNT), (2, bm.OK), (-7, bm.CANT_PARSE_NO_COUNT)])
def test_reference_id_outside_the_header(ref, status):
    # BamController.cpp:90-104: ref_id outside [0, n_refs) -> "can't parse", counted by neither side; ref_id == n_refs is outside
    assert row(base(), ref=ref).status == status


def test_missing_and_empty_barcodes_come_before_the_quality_filter():
    cfg = bm.Cfg(**{**CFG.__dict__, "min_phred": 126})
    low = ("CY", "Z", "!!!!")
    # FilledBamParamsParser.cpp:12-40: no CB / UB tag, or an empty one -> CANT_PARSE even when the quality would also fail
    assert row([("UB", "Z", UMI), low], cfg).status == bm.CANT_PARSE
    assert row([("CB", "Z", ""), ("UB", "Z", UMI), low], cfg).status == bm.CANT_PARSE
    assert row([("CB", "Z", CB), ("UB", "Z", ""), low], cfg).status == bm.CANT_PARSE
    assert row([("CB", "Z", CB), ("UB", "Z", UMI), low], cfg).status == bm.LOW_QUALITY


@pytest.mark.parametrize("min_phred,q,status", [
    (34, b"\"\"\"", bm.OK),          # ReadParameters.cpp:118-136: ... >= min passes; '"' = 34 == min
    (34, b"!", bm.LOW_QUALITY),      # 33 < 34
    (33, b"!!", bm.OK),              # the filter is on only when min > 33 (quality_offset)
    (126, b"~~", bm.OK),             # equal to the minimum
    (126, b"\x80", bm.LOW_QUALITY),  # bytes >= 0x80 are negative as signed char: below any minimum
    (34, b"\xff", bm.LOW_QUALITY),
    (126, b"", bm.OK),               # an empty quality string fails nothing
])
def test_quality_filter_signed_chars(min_phred, q, status):
    cfg = bm.Cfg(**{**CFG.__dict__, "min_phred": min_phred})
    assert row(base() + [("UY", "Z", q)], cfg).status == status
    assert row(base() + [("CY", "Z", q)], cfg).status == status


def test_first_occurrence_wins_and_numeric_closes():
    # host/bam_ingest.cpp:474-513: the first string occurrence of a name is the value ...
    r = row([("CB", "Z", CB), ("CB", "Z", "AAAA"), ("UB", "Z", UMI)])
    assert r.cb == bm.pack(CB.encode())
    # ... and a numeric one first makes the name absent for the rest of the record
    assert row([("CB", "i", 5), ("CB", "Z", CB), ("UB", "Z", UMI)]).status == bm.CANT_PARSE
    assert row([("GX", "C", 1), ("CB", "Z", CB), ("UB", "Z", UMI), ("GX", "Z", "G1")]).aux >> 16 == bm.HAS_NOT_ANNOTATED
    assert row([("CB", "B", ("f", [1.0])), ("CB", "Z", CB), ("UB", "Z", UMI)]).status == bm.CANT_PARSE
    # A counts as a one-byte string
    r = row([("CB", "A", "A"), ("UB", "A", "C")])
    assert r.status == bm.OK and r.cb == bm.pack(b"A") and r.umi == 1     # no gene: the UMI column is 1
    assert row([("CB", "H", "ACGT"), ("UB", "Z", UMI)]).cb == bm.pack(b"ACGT")   # H is a string like Z


@pytest.mark.parametrize("typ,val", [("c", -3), ("C", 200), ("s", -300), ("S", 60000), ("i", -5), ("I", 4_000_000_000), ("f", 1.5),
                                     ("B", ("c", [1, -2, 3])), ("B", ("C", [1, 2])), ("B", ("s", [-1])), ("B", ("S", [1, 2, 3])),
                                     ("B", ("i", [7] * 5)), ("B", ("I", [])), ("B", ("f", [0.5, 1.5])), ("Z", ""), ("H", "0AFF"), ("A", "x")])
def test_every_type_is_skipped_by_its_width(typ, val):
    # the walk must step over every type by its own width to find the tags behind it (SAMv1 §4.2.4)
    r = row([("xx", typ, val)] + base())
    assert r.status == bm.OK and r.gene == 7


def test_unknown_type_or_cut_value_stops_the_walk():
    # default: return (unknown type: cannot skip safely); a value past the end: return
    assert row([("CB", "Z", CB), ("UB", "Z", UMI), b"xxQ\x01\x02", ("GX", "Z", "G1")]).aux >> 16 == bm.HAS_NOT_ANNOTATED
    assert row([("CB", "Z", CB), b"xxB", ("UB", "Z", UMI)]).status == bm.CANT_PARSE            # B header cut: the walk stops before UB
    assert row([("CB", "Z", CB), ("UB", "Z", UMI), b"xxZ\x41\x42"]).status == bm.OK            # a string without its NUL at the end
    assert row([("CB", "Z", CB), b"xxB" + b"i" + struct.pack("<I", 1000) + b"\0" * 8, ("UB", "Z", UMI)]).status == bm.CANT_PARSE
    assert row([("CB", "Z", CB), ("UB", "Z", UMI), b"GX"]).aux >> 16 == bm.HAS_NOT_ANNOTATED     # fewer than 3 bytes left


def test_marks_and_read_type():
    # ReadParamsParser.cpp:67-90
    m = lambda t, cfg=CFG: row(base() + t, cfg).aux >> 16
    assert m([("RE", "A", "N")]) == bm.HAS_INTRONS
    assert m([("RE", "A", "I")]) == bm.HAS_NOT_ANNOTATED
    assert m([("RE", "A", "E")]) == bm.HAS_EXONS
    assert m([("RE", "Z", "")]) == bm.HAS_EXONS
    no_inter = bm.Cfg(**{**CFG.__dict__, "intergenic": b""})
    assert m([("RE", "A", "I")], no_inter) == bm.HAS_EXONS                # no intergenic value configured: matches nothing
    assert m([("RE", "Z", "")], no_inter) == bm.HAS_EXONS
    empty_intr = bm.Cfg(**{**CFG.__dict__, "intronic": b""})
    assert m([("RE", "Z", "")], empty_intr) == bm.HAS_INTRONS             # an empty intronic value matches an empty tag
    off = bm.Cfg(**{**CFG.__dict__, "read_type": False})
    assert m([("RE", "A", "N")], off) == bm.HAS_EXONS                     # read type off: the tag is not looked at
    # an intergenic read with a gene does not touch its chromosome: aux keeps no chromosome index
    assert row(base() + [("RE", "A", "I")]).aux == bm.HAS_NOT_ANNOTATED << 16


def test_empty_gene_is_no_gene():
    r = row([("CB", "Z", CB), ("UB", "Z", "ANNA"), ("GX", "Z", ""), ("RE", "A", "N")])
    # mark from the read type, but no gene: UMI column 1, gene NO_GENE, chromosome counted
    assert (r.umi, r.gene, r.aux, r.need) == (1, bm.NO_GENE, (bm.HAS_INTRONS << 16) | 5, 0)


def test_need_bits_and_dictionaries():
    assert row(base(), dicts=EMPTY).need == 3 and row(base(), dicts=EMPTY).gene == 0
    r = row([("CB", "Z", CB), ("UB", "Z", UMI)], dicts=EMPTY)
    assert r.need == 1                                                    # no gene, chromosome unknown
    r = row([("CB", "Z", CB), ("UB", "Z", "ACGN"), ("GX", "Z", "G2")])
    assert r.need == 3 and r.umi == 0 and r.gene == 8                     # an N: the caller packs it
    named = bm.Dicts(genes=FULL.genes, chr_of_ref=FULL.chr_of_ref, names=[b""] * 7 + [b"G1", b"G2"])
    assert row(base(), dicts=named).need == 2
    wrong = bm.Dicts(genes=FULL.genes, chr_of_ref=FULL.chr_of_ref, names=[b""] * 7 + [b"Gx", b"G2"])
    assert row(base(), dicts=wrong).need == 3 and row(base(), dicts=wrong).gene == 0     # a hash whose name differs goes to the caller
    short = bm.Dicts(genes=FULL.genes, chr_of_ref=FULL.chr_of_ref, names=[b"G1"])
    assert row(base(), dicts=short).need == 3


@pytest.mark.parametrize("s,packed", [("A" * 31, True), ("A" * 32, False), ("acgt", False), ("AC\x80T", False), ("", False), ("T", True)])
def test_packing(s, packed):
    # host/facade.cpp pack_bases: 1..31 of ACGT
    assert (bm.pack(s.encode("latin-1")) != 0) == packed


@pytest.mark.parametrize("name,status,cb,umi", [
    ("x!ACGT#GGTT", bm.OK, b"ACGT", b"GGTT"),
    ("a!b!ACGT#CC#GGTT", bm.OK, b"", None),                  # rfind('#') = the last '#'; rfind('!', up) = the last '!' before it: cb "ACGT#CC"
    ("x!#GGTT", bm.CANT_PARSE, None, None),                  # empty CB
    ("x!ACGT#", bm.CANT_PARSE, None, None),                  # empty UMI
    ("x#GG!TT", bm.CANT_PARSE, None, None),                  # no '!' before the last '#'
    ("ACGT#GG", bm.CANT_PARSE, None, None),
    ("!A#C", bm.OK, b"A", b"C"),
])
def test_read_name_mode(name, status, cb, umi):
    # ReadParamsParser.cpp:20-33; no quality filter in this mode (ReadParameters.cpp:42-56: min_phred_score 0)
    cfg = bm.Cfg(**{**CFG.__dict__, "filled_bam": False, "min_phred": 126})
    r = bm.parse_record(rec([("UY", "Z", "\x01"), ("GX", "Z", "G1")], name=name), cfg, FULL)
    assert r.status == status
    if status == bm.OK and cb:
        assert r.cb == bm.pack(cb) and r.umi == bm.pack(umi)
    if name.startswith("a!b!"):
        assert r.cb == 0 and r.need & 1                       # "ACGT#CC" does not pack
    if status == bm.OK:
        assert r.umi_quality is None


def test_odd_fixed_fields_are_data():
    # no CIGAR, no bases, a next_refID anywhere: the record is what its lengths say
    r = bm.parse_record(bw.record(1, 5, "q", seq="", cigar=[], next_ref=99, tags=base()), CFG, FULL)
    assert r.status == bm.OK and r.aux & 0xFFFF == 6
    r = bm.parse_record(bw.record(1, 5, "q", seq="ACG", cigar=[(1, op) for op in "MIDNSHP=X"], tags=base()), CFG, FULL)
    assert r.status == bm.OK
    # an l_read_name that claims more than the name: the tags are read where the lengths put them
    r = bm.parse_record(bw.record(1, 5, "q", seq="", cigar=[], l_read_name=2 + 3, tags=[b"zzZ"] + base()), CFG, FULL)
    assert r.status == bm.OK
    with pytest.raises(ValueError):                            # lengths past block_size: corrupt on both readers
        bm.parse_record(bw.record(1, 5, "q", seq="", cigar=[], l_read_name=200, tags=[]), CFG, FULL)


def test_window_summary():
    rows = [row(base() + [("UY", "Z", "AAA")]), row(base(), flag=4), row([("CB", "Z", CB), ("UB", "Z", UMI), ("UY", "Z", "A" * 70_000)]),
            row(base() + [("UY", "Z", "A" * 70_000)]), bm.parse_record(rec(base(), ref=0), CFG, EMPTY)]
    w = bm.window(rows)
    assert w.counts == [4, 1, 0, 0, 0] and w.n_accepted == 4
    assert (w.need_rec, w.need_pos, w.need_size) == ([4], [3], [rows[4].size])
    assert (w.quality_seen, w.any_gene) == (1, 1)
    assert (w.quality_len_min, w.quality_len_max) == (0, 70_000)      # over the gene-bearing reads: "AAA"... and the one without a string
    assert bm.window([row([("CB", "Z", CB), ("UB", "Z", UMI), ("UY", "Z", "AB")])]).quality_len_max == 0     # no gene: not counted


def test_writer_round_trip_through_gzip(tmp_path):
    recs = [bw.record(i % 3, i, "r%d" % i, seq="ACGTN"[: i % 6], cigar=[] if i % 4 == 0 else None,
                      tags=[("xx", "B", (sub, [1, 2])) for sub in "cCsSiIf"] + [("CB", "Z", CB), ("s1", "s", -2), ("S1", "S", 3), ("I1", "I", 9)])
            for i in range(300)]
    path = str(tmp_path / "w.bam")
    bw.write_bam(path, [("a", 10), ("b", 10), ("c", 10)], recs, block=777)
    raw = gzip.decompress(open(path, "rb").read())
    first, got = bm.records_of(raw)
    assert got == recs and first > 12
    for r in got:
        assert bm.parse_record(r, CFG, FULL).status == bm.CANT_PARSE      # no UB tag: every tag before it skipped by its width, none misread
