"""The model of read-parameter files (read_params_model.py) pinned on literal cases: the row forms of test_gpu_bam.py::test_read_parameter_files,
line ends, the fifth field, both quality filters, and the serving rules."""
import read_params_model as m


def row(line, min_phred=0):
    return m.parse_row(line, min_phred)


def test_row_forms():
    assert row(b"r1 ACGT TTGA IIII JJJJ\n") == dict(name=b"r1", cb=b"ACGT", umi=b"TTGA", quality=b"JJJJ", ok=True)
    assert row(b"@r1 ACGT TTGA IIII JJJJ\n")["name"] == b"r1"                    # one '@' off the name
    assert row(b"@@r1 ACGT TTGA IIII JJJJ\n")["name"] == b"@r1"                  # ... one only
    assert row(b"broken\n") == "malformed" and row(b"a b c d\n") == "malformed"   # fewer than four spaces
    assert row(b"r1  TTGA IIII JJJJ\n") == "malformed"                            # an empty barcode
    assert row(b"r1 ACGT  IIII JJJJ\n") == "malformed"                            # an empty UMI
    assert row(b" ACGT TTGA IIII JJJJ\n")["name"] == b""                          # an empty name is a name
    assert row(b"\n") is None and row(b"") is None and row(b"\r\n") is None       # empty lines are nothing
    assert row(b"r1 ACNT TTGA IIII JJJJ\n")["cb"] == b"ACNT"


def test_line_ends():
    assert row(b"r1 AC TT II JJ\r\n")["quality"] == b"JJ"                         # the '\r' goes with its '\n'
    assert row(b"r1 AC TT II JJ")["quality"] == b"JJ"                             # no final newline
    assert row(b"r1 AC TT II JJ\r")["quality"] == b"JJ\r"                         # ... and then a '\r' is the field's
    assert row(b"\r") == "malformed"
    lines, offs = m.split_lines(b"a b c d e\n\nf g h i j")
    assert lines == [b"a b c d e\n", b"\n", b"f g h i j"] and offs == [0, 10, 11]
    assert m.split_lines(b"") == ([], [])


def test_fifth_field_and_empty_quality_fields():
    assert row(b"r1 AC TT II J J J\n")["quality"] == b"J J J"                    # the rest of the line, spaces and all
    assert row(b"r1 AC TT  \n") == dict(name=b"r1", cb=b"AC", umi=b"TT", quality=b"", ok=True)
    assert row(b"r1 AC TT  \n", 53)["ok"] is True                                # nothing to fail on
    assert row(b"r1 AC TT II \n")["quality"] == b""


def test_quality_filters():
    # min_phred is a character code: 53 = '5'
    assert row(b"r1 AC TT 55 55\n", 53)["ok"] is True
    assert row(b"r1 AC TT 54 55\n", 53)["ok"] is False                           # the barcode's quality
    assert row(b"r1 AC TT 55 45\n", 53)["ok"] is False                           # the UMI's quality
    assert row(b"r1 AC TT !! !!\n", 33)["ok"] is True                            # the filter is on above 33 only
    assert row(b"r1 AC TT !! !!\n", 0)["ok"] is True
    assert row(b"r1 AC TT !! !!\n", 34)["ok"] is False
    assert row(b"r1 AC TT 5\xff 55\n", 53)["ok"] is False                        # characters are signed


def test_pack():
    assert m.pack(b"A") == 4 and m.pack(b"ACGT") == (1 << 8) | 0b00011011
    assert m.pack(b"") == 0 and m.pack(b"ACNT") == 0 and m.pack(b"A" * 32) == 0 and m.pack(b"A" * 31) == 1 << 62


def test_first_row_wins_across_files():
    rows = m.Rows([b"a AC TT II JJ\nb AA CC II JJ\na GG GG II JJ\n", b"junk\n\nb TT TT II JJ\n@c CA CA II JJ"], 0)
    assert [r["canonical"] if isinstance(r, dict) else r for r in rows.rows] == [0, 1, 0, "malformed", None, 1, 6]
    assert rows.counts() == dict(rows=7, valid=5, malformed=1, repeated=2)
    assert rows.lookup(b"a") == 0 and rows.lookup(b"@b") == 1 and rows.lookup(b"c") == 6 and rows.lookup(b"@c") == 6 and rows.lookup(b"d") == m.NONE


def test_serving():
    rows = m.Rows([b"a AC TT 55 55\nlow AC TT 44 55\nb AC TT 55 55\n"], 53)
    s = m.Server(rows)
    assert s.serve(m.SKIP, b"a") == (m.SKIP, m.NONE)                             # an unmapped / secondary record asks for nothing
    assert s.serve(m.CANT_PARSE_NO_COUNT, b"a") == (m.CANT_PARSE_NO_COUNT, m.NONE)
    assert s.serve(m.OK, b"@a") == (m.OK, 0)                                     # ... so the row is still there
    assert s.serve(m.OK, b"a") == (m.CANT_PARSE, m.NONE)                         # a name serves once
    assert s.serve(m.OK, b"zzz") == (m.CANT_PARSE, m.NONE)
    assert s.serve(m.CANT_PARSE, b"low") == (m.LOW_QUALITY, 1)                   # low quality wins over the annotation's verdict
    assert s.serve(m.OK, b"low") == (m.CANT_PARSE, m.NONE)                       # ... and the row is consumed
    assert s.serve(m.CANT_PARSE, b"b") == (m.CANT_PARSE, 2)                      # a record the annotation refuses still takes its row
    assert s.serve(m.OK, b"b") == (m.CANT_PARSE, m.NONE)
