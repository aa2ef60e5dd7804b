"""Tagged and filtered BAM output (-b, -F) under -r (read-parameter files) and -P (gene = chromosome name) at file level, behind
BamController::set_device_source_output, through tests/cpp/bam_sources_output: the files the device BAM path writes inflate to the input's header
followed by tests/bam_tag_sources_model.py's records; the .rds beside them is the one of the run without output; the -F pass leaves the ingest's
claims as they were; with the switch off both outputs are refused in the words they always were.  The construction (6 000 reads with missing,
low, duplicated and repeated rows and N barcodes, two parameter files, small windows) is test_gpu_bam_device_sources.py's."""
import gzip
import json
import os
import subprocess

import pytest

from dropest_amd.build import SOURCES_OUTPUT_TOOL, build_facade

import annotation_model as am
import bam_filter_model as fm
import bam_model as bm
import bam_tag_sources_model as sm
import bam_writer as bw
import read_params_model as rp
import rds_reader as rr
from test_gpu_bam_device_sources import DEVICE, REFS, SMALL, chromosome_genes, construction, one_file, taken, write_params  # noqa: F401 (fixtures)
from test_gpu_bam_sharded_device import _same_rds
from test_gpu_bam_tagged_file import check_bgzf

pytestmark = pytest.mark.gpu
PHRED = 10
CFG = bm.Cfg(tags=("CB", "UB", "CQ", "UQ", "GX", "RE"), filled_bam=False, min_phred=33 + PHRED, read_type=True, intronic=b"N", intergenic=b"I", n_refs=len(REFS))
OUT = fm.FilterOutCfg(read_type="RE", exonic=b"E", intronic=b"N", intergenic=b"I")      # the tool's tags
REF_NAMES = [n.encode() for n, _ in REFS]
ENV = dict(SMALL, DROPEST_MIN_PHRED=str(PHRED))


def run(tmp, mode, bams, sources, output=1, chromosome_gene=0, env=None, devices="-", quota=0, ok=True, dump=False, further=None):
    """-> (the tool's JSON line, the .rds, stderr[, the dumped decisions])"""
    build_facade()
    os.makedirs(str(tmp), exist_ok=True)
    out = str(tmp / "res")
    e = dict(os.environ, DROPEST_RPUPC="1", **(env or {}))
    if dump:
        e["DROPEST_FILTER_DUMP"] = str(tmp / "decisions.txt")
    if further:
        e["DROPEST_FURTHER_FILES"] = ":".join(further)
    res = subprocess.run([SOURCES_OUTPUT_TOOL, out, mode, str(chromosome_gene), str(sources), str(output), "3", "5", "-", "3", devices, str(quota)] + bams,
                         capture_output=True, text=True, timeout=300, cwd=str(tmp), env=e)
    if not ok:
        assert res.returncode != 0
        return res.stderr
    assert res.returncode == 0, res.stdout + res.stderr
    stats = json.loads(res.stdout.strip().splitlines()[-1])
    got = (stats, rr.read_rds(out + ".rds"), res.stderr)
    if dump:
        decisions = []
        for line in open(str(tmp / "decisions.txt")):
            v, cb, u = line.split()
            decisions.append((int(v), b"" if cb == "-" else cb.encode(), b"" if u == "-" else u.encode()))
        got += (decisions,)
    return got


def stream_of(bam):
    """(the header's bytes, the records) of a written BAM"""
    raw = gzip.decompress(open(bam, "rb").read())
    first, recs = bm.records_of(raw)
    return raw[:first], recs


def texts_of(mode):
    return [gzip.open(p, "rb").read() for p in mode[len("params:"):].split()]


def inflated(tmp, name):
    blob = open(os.path.join(str(tmp), name), "rb").read()
    n_blocks, total = check_bgzf(blob)
    got = gzip.decompress(blob)
    assert total == len(got)
    return got


def guards(kinds, out_records, need_taken=True):
    """on the expected side: no comparison passes on an empty case"""
    hist = {k: kinds.count(k) for k in set(kinds)}
    assert hist.get(sm.NO_ROW, 0) >= 20 and hist.get(sm.LOW_QUALITY, 0) >= 20 and (not need_taken or hist.get(sm.ROW_TAKEN, 0) >= 20), hist
    assert len(out_records) >= 300
    with_n = 0
    for r in out_records:
        at = r.find(b"CRZ", sm.layout(r)[3])
        with_n += b"N" in r[at + 3:r.index(b"\0", at)]
    assert with_n >= 10, with_n


def split_records(body):
    out, o = [], 0
    while o < len(body):
        n = 4 + int.from_bytes(body[o:o + 4], "little")
        out.append(body[o:o + n]); o += n
    return out


def check_tagged(tmp, bam, entry, want_body):
    header, _ = stream_of(bam)
    stem = os.path.basename(bam)[:-4]
    got = inflated(tmp, stem + ".tagged.bam")
    assert entry["name"] == stem + ".tagged.bam" and entry["windows"] >= 4
    assert got[:len(header)] == header
    got_recs, want_recs = split_records(got[len(header):]), split_records(want_body)
    assert len(got_recs) == len(want_recs) == entry["records"]
    for k, (a, b) in enumerate(zip(got_recs, want_recs)):      # record for record
        assert a == b, k


def server_of(mode):
    return rp.Server(rp.Rows(texts_of(mode), CFG.min_phred))


# ---- -b ---------------------------------------------------------------------------------------------------------------------------------------
def test_tagged_file_under_read_parameters(one_file, tmp_path):
    f = one_file
    _, recs = stream_of(f["bam"])
    want, written, kinds = sm.stream(recs, CFG, OUT, server=server_of(f["mode"]))
    guards(kinds, split_records(want))
    assert written == len(f["kept"])
    stats, d, err = run(tmp_path, f["mode"], [f["bam"]], "1b", env=ENV)
    assert taken(err) == [1], err
    check_tagged(tmp_path, f["bam"], stats["tagged"][0], want)
    assert stats["saved"] == written and stats["low_quality"] == f["n"]["low"]
    _same_rds(d, f["host"][3])                                              # the .rds of the run without -b


def test_tagged_files_of_two_inputs_over_one_table(tmp_path):
    """names of the first file aligned again in the second: their rows are taken, the records not written"""
    recs1, rows1, kept1, n1 = construction(3_000, 5)
    again = ["read%d" % i for i in range(0, 3_000, 50)]
    recs2, rows2, kept2, n2 = construction(3_000, 6, first=3_000, taken_names=again)
    mode = write_params(tmp_path, rows1 + rows2, parts=3)
    bams = [str(tmp_path / "a.bam"), str(tmp_path / "b.bam")]
    bw.write_bam(bams[0], REFS, recs1, block=1_500); bw.write_bam(bams[1], REFS, recs2, block=1_500)
    server = server_of(mode)                                                # one parser serves both files
    want1, w1, kinds1 = sm.stream(recs1, CFG, OUT, server=server)
    want2, w2, kinds2 = sm.stream(recs2, CFG, OUT, server=server)
    guards(kinds1 + kinds2, split_records(want1 + want2))
    assert kinds2.count(sm.ROW_TAKEN) >= n2["again"] - 5 and (w1, w2) == (len(kept1), len(kept2))
    stats, d, err = run(tmp_path / "b", mode, bams, "1b", env=ENV)
    assert taken(err) == [1, 1], err
    check_tagged(tmp_path / "b", bams[0], stats["tagged"][0], want1)
    check_tagged(tmp_path / "b", bams[1], stats["tagged"][1], want2)
    _same_rds(d, run(tmp_path / "plain", mode, bams, "1", env=ENV)[1])


@pytest.mark.parametrize("with_gtf", [False, True], ids=["no-gtf", "gtf"])
def test_tagged_file_with_chromosome_genes(chromosome_genes, tmp_path, with_gtf):
    f = chromosome_genes
    extra = {"DROPEST_GTF": f["gtf"]} if with_gtf else {}                    # -P comes before -g: the annotation is not asked
    _, recs = stream_of(f["bam"])
    want, written, kinds = sm.stream(recs, CFG, OUT, ref_names=REF_NAMES)
    assert written == f["n"] >= 300 and want.count(b"REZE\x00") == written
    stats, d, err = run(tmp_path / "b", "name", [f["bam"]], "1b", chromosome_gene=1, env=dict(SMALL, **extra))
    assert taken(err) == [1], err
    check_tagged(tmp_path / "b", f["bam"], stats["tagged"][0], want)
    _same_rds(d, run(tmp_path / "plain", "name", [f["bam"]], "1", chromosome_gene=1, env=dict(SMALL, **extra))[1])


def test_tagged_file_with_chromosome_genes_and_read_parameters(one_file, tmp_path):
    f = one_file
    _, recs = stream_of(f["bam"])
    want, written, kinds = sm.stream(recs, CFG, OUT, server=server_of(f["mode"]), ref_names=REF_NAMES)
    guards(kinds, split_records(want))
    stats, d, err = run(tmp_path / "b", f["mode"], [f["bam"]], "1b", chromosome_gene=1, env=ENV)
    assert taken(err) == [1], err
    check_tagged(tmp_path / "b", f["bam"], stats["tagged"][0], want)
    _same_rds(d, run(tmp_path / "plain", f["mode"], [f["bam"]], "1", chromosome_gene=1, env=ENV)[1])


def test_tagged_file_with_an_annotation_and_read_parameters(one_file, tmp_path):
    """-g with -r: gene and mark are the annotation's (tests/annotation_model.py), the strings the row's; a record on a chromosome the annotation
    lacks takes its row and is not written"""
    f = one_file
    gtf = str(tmp_path / "a.gtf")
    with open(gtf, "w") as fh:
        fh.write('chr1\ts\texon\t1\t500000\t.\t+\t.\tgene_id "A"; transcript_id "T";\n')
        fh.write('chr2\ts\texon\t1\t2000\t.\t+\t.\tgene_id "B"; transcript_id "U";\nchr2\ts\texon\t4001\t500000\t.\t+\t.\tgene_id "B"; transcript_id "U";\n')
        fh.write('chr3\ts\texon\t3000\t3500\t.\t-\t.\tgene_id "C"; transcript_id "V";\n')
    ann = am.Annotation(am.read_gtf(gtf))
    _, recs = stream_of(f["bam"])
    annotated = []
    for r in recs:
        ref_id, pos = int.from_bytes(r[4:8], "little", signed=True), int.from_bytes(r[8:12], "little", signed=True)
        got = ann.gene_for_read(REFS[ref_id][0], pos, pos + 40)               # (40 M: bam_writer's default read)
        annotated.append(None if got is None else (got[0].encode(), got[1]))
    marks = {a[1] for a in annotated if a}
    assert annotated.count(None) > 1000 and {2, 4} <= marks and any(m not in (1, 2, 4) for m in marks) and any(a and not a[0] for a in annotated)
    want, written, kinds = sm.stream(recs, CFG, OUT, server=server_of(f["mode"]), annotated=annotated)
    assert written >= 300 and kinds.count(sm.NOT_PARSED) > 1000 and kinds.count(sm.LOW_QUALITY) >= 20
    env = dict(ENV, DROPEST_GTF=gtf)
    stats, d, err = run(tmp_path / "b", f["mode"], [f["bam"]], "1b", env=env)
    assert taken(err) == [1], err
    check_tagged(tmp_path / "b", f["bam"], stats["tagged"][0], want)
    assert stats["saved"] == written
    _same_rds(d, run(tmp_path / "plain", f["mode"], [f["bam"]], "1", env=env)[1])


# ---- -F ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def filtered_case(tmp_path_factory):
    """the construction with one more row, "fresh", that no record of the file asks for; and a further file that asks for it among names the
    first file consumed"""
    tmp = tmp_path_factory.mktemp("sources_filtered")
    recs, rows, kept, n = construction(6_000, 17)
    rows.insert(100, "fresh ACGTACGTACGT ACGTACGT IIIIIIIIIIII IIIIIIII")
    mode = write_params(tmp, rows)
    bam, more = str(tmp / "r.bam"), str(tmp / "more.bam")
    bw.write_bam(bam, REFS, recs, block=1_500)
    names = ["read%d" % i for i in range(0, 6_000, 40)]
    bw.write_bam(more, REFS, [bw.record(1, k, nm, tags=[("GX", "Z", "ENSG00001")]) for k, nm in enumerate(names[:75] + ["fresh"] + names[75:])], block=1_500)
    return dict(tmp=tmp, mode=mode, bam=bam, more=more, n_more=len(names) + 1, recs=stream_of(bam)[1], header=stream_of(bam)[0])


def check_filtered(f, tmp, stats, decisions):
    want, written, kinds = sm.stream(f["recs"], CFG, OUT, server=server_of(f["mode"]), decisions=decisions)
    assert sm.accepted(kinds) == len(decisions)                             # the same records are accepted as in the ingest
    guards(kinds, split_records(want))
    assert kinds.count(sm.NOT_KEPT) >= 20
    got = inflated(tmp, "r.filtered.bam")
    assert got[:len(f["header"])] == f["header"]
    got_recs, want_recs = split_records(got[len(f["header"]):]), split_records(want)
    assert len(got_recs) == len(want_recs)
    for k, (a, b) in enumerate(zip(got_recs, want_recs)):
        assert a == b, k
    fl = stats["filtered"]
    assert fl["name"] == "r.filtered.bam" and fl["windows"] >= 4 and fl["total_reads"] == len(decisions)
    assert fl["written"] == written == fl["corrections_written"] == sum(1 for d in decisions if d[0] == 0)
    return got


def test_filtered_file_under_read_parameters(filtered_case, tmp_path):
    f = filtered_case
    stats, d, err, decisions = run(tmp_path, f["mode"], [f["bam"]], "1F", env=ENV, dump=True, further=[f["more"]])
    assert taken(err) == [1, 1], err                                        # the ingest and the further file on the device path (the -F pass has no other)
    check_filtered(f, tmp_path, stats, decisions)
    # the further file after the pass: every name the ingest consumed is still consumed (the claims came back), the one fresh row serves
    assert stats["further"] == dict(total_reads=f["n_more"], cant_parse=f["n_more"] - 1, low_quality=0, saved=1)


def test_filtered_file_of_a_sharded_container(filtered_case, tmp_path):
    """two shards on one GPU, a quota that puts their boundary inside a window: the bytes of the one-context file"""
    f = filtered_case
    one = run(tmp_path / "one", f["mode"], [f["bam"]], "1F", env=ENV)
    stats, d, err = run(tmp_path / "two", f["mode"], [f["bam"]], "1F", env=ENV, devices="0,0", quota=1_777)
    assert taken(err) == [1], err
    assert stats["filtered"]["written"] == one[0]["filtered"]["written"] >= 300 and stats["filtered"]["windows"] >= 4
    assert inflated(tmp_path / "two", "r.filtered.bam") == inflated(tmp_path / "one", "r.filtered.bam")


# ---- the switch off ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", ["0", "1"])
def test_output_stays_refused_without_the_switch(one_file, chromosome_genes, tmp_path, switch):
    f, c = one_file, chromosome_genes
    err = run(tmp_path / "b", f["mode"], [f["bam"]], switch + "b", output=0, env=DEVICE, ok=False)
    assert "Tagged BAM output (-b) is written on the device BAM path only, which this configuration cannot take: read-parameter files (-r) are served by the host reader" in err
    err = run(tmp_path / "F", f["mode"], [f["bam"]], switch + "F", output=0, env=DEVICE, ok=False)
    assert "Filtered BAM output (-F) is written on the device BAM path only, which this configuration cannot take: read-parameter files (-r) are served by the host reader" in err
    err = run(tmp_path / "Pb", "name", [c["bam"]], switch + "b", output=0, chromosome_gene=1, env=DEVICE, ok=False)
    assert "Tagged BAM output (-b) is written on the device BAM path only, which this configuration cannot take: gene = chromosome name is resolved by the host reader" in err
    err = run(tmp_path / "PF", "name", [c["bam"]], switch + "F", output=0, chromosome_gene=1, env=DEVICE, ok=False)
    assert "Filtered BAM output (-F) is written on the device BAM path only, which this configuration cannot take: gene = chromosome name is resolved by the host reader" in err
    if switch == "0":      # the new switch alone changes nothing: it works together with set_device_read_sources
        err = run(tmp_path / "b1", f["mode"], [f["bam"]], "0b", output=1, env=DEVICE, ok=False)
        assert "cannot take: read-parameter files (-r) are served by the host reader" in err
