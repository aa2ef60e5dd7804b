"""The model of -b / -F under -r and -P (tests/bam_tag_sources_model.py) pinned on hand-built records: the expected aux bytes stand here
literally, worked out by hand from the rules in the model's docstring.  The GPU tests compare the device's output with this model, so the model
itself is checked against nothing but these bytes.  And the new calls of the C-ABI are exported."""
import bam_filter_model as fm
import bam_model as bm
import bam_tag_model as tm
import bam_tag_sources_model as sm
import read_params_model as rp
from dropest_amd import capi
from test_bam_tag_model_cpu import _rec

NEW_CALLS = ["dropest_bam_decoder_set_reference_names", "dropest_read_params_replay_begin", "dropest_read_params_replay_end"]

# -r is never -f: barcode and UMI of a record without a row would come from its name
CFG = bm.Cfg(tags=("CB", "UB", "CQ", "UQ", "GX", "RE"), filled_bam=False, read_type=True, intronic=b"N", intergenic=b"I", n_refs=2)
PLAIN, TYPED = tm.OutCfg(), tm.OutCfg(read_type="RE", exonic=b"E", intronic=b"N", intergenic=b"I")
NH = b"NHi\x01\x00\x00\x00"


def _on_ref(rec, ref_id):
    return rec[:4] + ref_id.to_bytes(4, "little", signed=True) + rec[8:]


def _server(text, min_phred=0):
    return rp.Server(rp.Rows([text], min_phred))


def test_the_new_calls_are_exported():
    L = capi.lib()
    for name in NEW_CALLS:
        assert hasattr(L, name), "missing export: " + name


def test_existing_entries_under_read_parameters():
    """CR:Z, UR:i and UQ:Z of the record go (every type), the row's strings are appended; CQ is not edited under -r and stays where it is; the
    record's name ("id!CB#UMI" form or not) and its CB / UB tags are not looked at"""
    rec = _rec(b"r1", b"CRZold\x00" + NH + b"URi\x07\x00\x00\x00" + b"CQZFFFF\x00" + b"UQZ####\x00" + b"CBZTTTT\x00")
    out, written, kinds = sm.stream([rec], CFG, PLAIN, server=_server(b"r1 ACNg TTGA IIII JJJJ\n"))
    assert kinds == [sm.WRITTEN] and written == 1
    assert out == _rec(b"r1", NH + b"CQZFFFF\x00" + b"CBZTTTT\x00" + b"CRZACNg\x00" + b"URZTTGA\x00" + b"UQZJJJJ\x00")


def test_an_empty_fifth_field_writes_no_quality_and_drops_none():
    rec = _rec(b"@r1", b"UQZ##\x00" + NH)                                   # '@' on the record, none on the row
    out, _, kinds = sm.stream([rec], CFG, PLAIN, server=_server(b"r1 AC GT II \r\n"))
    assert kinds == [sm.WRITTEN]
    assert out == _rec(b"@r1", b"UQZ##\x00" + NH + b"CRZAC\x00" + b"URZGT\x00")


def test_which_records_are_written_under_read_parameters():
    """no row; a row an earlier record took; a low-quality row (which is consumed: the next record of that name finds nothing)"""
    text = b"a AC GT II II\n@b AC GT I# II\nc AC GT II II\n"
    recs = [_rec(n, NH) for n in (b"a", b"zz", b"a", b"b", b"b", b"c")] + [_rec(b"c", NH, flag=4)]
    out, written, kinds = sm.stream(recs, CFG, PLAIN, server=_server(text, 33 + 10))
    assert kinds == [sm.WRITTEN, sm.NO_ROW, sm.ROW_TAKEN, sm.LOW_QUALITY, sm.ROW_TAKEN, sm.WRITTEN, sm.SKIPPED]
    assert written == 2 and out == _rec(b"a", NH + b"CRZAC\x00URZGT\x00UQZII\x00") + _rec(b"c", NH + b"CRZAC\x00URZGT\x00UQZII\x00")
    # a second pass takes a NEW parser: the same records are accepted again (rule 5)
    assert sm.stream(recs, CFG, PLAIN, server=_server(text, 33 + 10))[0] == out


def test_gene_is_the_reference_name():
    """-P: the gene tag's value is the reference's name and the read is exonic; an empty name gives neither tag, so GX and RE stay as they are"""
    rec = _rec(b"x!AC#GT", b"GXZold\x00" + b"REAN")
    out, _, kinds = sm.stream([rec, _on_ref(rec, 1)], CFG, TYPED, ref_names=[b"chr1", b""])
    assert kinds == [sm.WRITTEN, sm.WRITTEN]
    assert out == _rec(b"x!AC#GT", b"GXZchr1\x00" + b"CRZAC\x00" + b"URZGT\x00" + b"REZE\x00") + _on_ref(_rec(b"x!AC#GT", b"GXZold\x00" + b"REAN" + b"CRZAC\x00" + b"URZGT\x00"), 1)
    # -P comes before -g: an annotation's answer is not looked at
    assert sm.stream([rec], CFG, TYPED, ref_names=[b"chr1", b""], annotated=[(b"GA", 4)])[0] == _rec(b"x!AC#GT", b"GXZchr1\x00CRZAC\x00URZGT\x00REZE\x00")


def test_reference_name_and_read_parameters_together():
    rec = _rec(b"plain", b"URZq\x00" + b"GXZold\x00")
    out, _, kinds = sm.stream([rec], CFG, TYPED, server=_server(b"plain acgt NNNN II KK\n"), ref_names=[b"7", b"8"])
    assert kinds == [sm.WRITTEN]
    assert out == _rec(b"plain", b"GXZ7\x00" + b"CRZacgt\x00" + b"URZNNNN\x00" + b"UQZKK\x00" + b"REZE\x00")


def test_annotation_and_read_parameters_together():
    """-g with -r: gene and mark are the annotation's, the strings the row's; a chromosome the annotation lacks loses the record AFTER it took its row"""
    recs = [_rec(b"a", b"GXZtag\x00"), _rec(b"b", NH), _rec(b"b", NH)]
    out, _, kinds = sm.stream(recs, CFG, TYPED, server=_server(b"a AC GT I J\nb CC GG I J\n"), annotated=[(b"GA", 4), None, (b"", 1)])
    assert kinds == [sm.WRITTEN, sm.NOT_PARSED, sm.ROW_TAKEN]
    assert out == _rec(b"a", b"GXZGA\x00" + b"CRZAC\x00" + b"URZGT\x00" + b"UQZJ\x00" + b"REZN\x00")


def test_filtered_pass_under_read_parameters():
    """-F: decisions belong to the accepted records in order; the corrected pair follows the other tags"""
    recs = [_rec(b"a", NH), _rec(b"nobody", NH), _rec(b"b", NH), _rec(b"c", b"CBZold\x00")]
    decisions = [(0, b"ACGG", b"TT"), (3, b"", b""), (0, b"", b"GA")]
    out, written, kinds = sm.stream(recs, CFG, fm.FilterOutCfg(), server=_server(b"a AC GT I J\nb CC GG I J\nc GG CC I \n"), decisions=decisions)
    assert kinds == [sm.WRITTEN, sm.NO_ROW, sm.NOT_KEPT, sm.WRITTEN] and written == 2 and sm.accepted(kinds) == 3
    assert out == _rec(b"a", NH + b"CRZAC\x00URZGT\x00UQZJ\x00" + b"CBZACGG\x00UBZTT\x00") + _rec(b"c", b"CBZold\x00" + b"CRZGG\x00URZCC\x00" + b"UBZGA\x00")
