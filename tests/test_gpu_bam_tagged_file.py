"""Tagged BAM output (-b) at file level, through tests/cpp/bam_tagged: BamController::parse_bam_files(files, true, container) on the device BAM
path.  The `<stem>.tagged.bam` it writes is BGZF with the end-of-file block, inflates to the input's header bytes followed by
tests/bam_tag_model.py's records, and the ingest beside it is the one bam_to_counts makes (the same .rds)."""
import gzip
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from dropest_amd.build import build_facade

import bam_model as bm
import bam_tag_model as tm
import bam_writer as bw
import rds_reader as rr
from test_gpu_bam_tag_window import make_records

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tests", "cpp", "bam_tagged")
COUNTS_TOOL = os.path.join(ROOT, "tests", "cpp", "bam_to_counts")
REFS = [("chr%d" % i, 1 << 20) for i in range(4)]
EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
CFG = bm.Cfg(tags=("CB", "UB", "CQ", "UQ", "GX", "RE"), filled_bam=True, read_type=True, intronic=b"N", intergenic=b"I", n_refs=len(REFS))
OUT = tm.OutCfg(read_type="RE", exonic=b"E", intronic=b"N", intergenic=b"I")          # the tool's tags (as bam_to_counts: RE with N / I / E)
SMALL_WINDOWS = {"DROPEST_BAM_WINDOW_BLOCKS": "64", "DROPEST_BAM_TAGGED_BATCH_KB": "1024"}


class Input:
    """a written BAM, its header bytes and what the model makes of its records (computed once, shared by the tests that read the file)"""
    def __init__(self, path, recs, cfg=CFG, block=12_345, refs=REFS, overrides=None):
        self.path = path
        bw.write_bam(path, refs, recs, block=block)
        raw = gzip.decompress(open(path, "rb").read())
        first, _ = bm.records_of(raw)
        self.header = raw[:first]
        model = [tm.tagged_record(r, cfg, OUT, *(overrides[i] if overrides else ())) if not overrides or overrides[i] is not None else None for i, r in enumerate(recs)]
        self.records = [m for m in model if m is not None]
        self.want = self.header + b"".join(self.records)


def run(cwd, mode, bams, env=None, expect_failure=False):
    build_facade()
    res = subprocess.run([TOOL, os.path.join(str(cwd), "res"), mode, "3"] + bams, capture_output=True, text=True, timeout=300, cwd=str(cwd), env=dict(os.environ, **(env or {})))
    if expect_failure:
        return res
    assert res.returncode == 0, res.stdout + res.stderr
    return json.loads(res.stdout.strip().splitlines()[-1])


def check_bgzf(blob):
    """every block: gzip magic with FEXTRA, the BC subfield, ISIZE of at most 65 536; the file ends in the 28-byte end-of-file block"""
    at, n, total = 0, 0, 0
    while at < len(blob):
        assert blob[at:at + 4] == b"\x1f\x8b\x08\x04", at
        xlen = struct.unpack_from("<H", blob, at + 10)[0]
        assert xlen == 6 and blob[at + 12:at + 16] == b"BC\x02\x00", at
        bsize = struct.unpack_from("<H", blob, at + 16)[0] + 1
        isize = struct.unpack_from("<I", blob, at + bsize - 4)[0]
        assert isize <= 65536 and at + bsize <= len(blob)
        total += isize; at += bsize; n += 1
    assert at == len(blob) and blob[-28:] == EOF_BLOCK
    return n, total


def check_output(cwd, stem, inp, entry):
    blob = open(os.path.join(str(cwd), stem + ".tagged.bam"), "rb").read()
    n_blocks, total = check_bgzf(blob)
    got = gzip.decompress(blob)
    assert total == len(got) == len(inp.want) and got == inp.want
    assert entry["name"] == stem + ".tagged.bam" and entry["records"] == len(inp.records)
    assert entry["inflated_bytes"] == len(inp.want) and entry["compressed_bytes"] == len(blob)
    return n_blocks


def _plain(v):
    if not isinstance(v, rr.RObject):
        if isinstance(v, np.ndarray):
            return [None if (isinstance(x, float) and x != x) else x for x in v.tolist()]
        if isinstance(v, (list, tuple)):
            return [_plain(x) for x in v]
        return v
    return (v.kind, _plain(v.value), {k: _plain(x) for k, x in sorted(v.attributes.items())})


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    """~20 000 records of every kind test_gpu_bam_tag_window.py writes; every record with a UQ of one length, so the windows go in bulk"""
    d = tmp_path_factory.mktemp("tagged_base")
    return Input(str(d / "base.bam"), make_records(True, False, seed=5, n=20_000, uq="all"))


@pytest.fixture(scope="module")
def two_lengths(tmp_path_factory):
    d = tmp_path_factory.mktemp("tagged_two")
    return Input(str(d / "lengths.bam"), make_records(True, False, seed=6, n=4_000, uq="two"), block=997)


def test_tagged_file_and_unchanged_ingest(tmp_path, base):
    stats = run(tmp_path, "filled", [base.path], env=SMALL_WINDOWS)
    (entry,) = stats["files"]
    assert entry["windows"] >= 3 and entry["batches"] >= 3
    n_blocks = check_output(tmp_path, "base", base, entry)
    assert n_blocks > len(base.want) // 65280                              # full chunks (every batch is a multiple of 65 280) + the end-of-file block
    assert stats["saved"] == len(base.records) == entry["records"] > 15_000
    # the ingest itself: the .rds bam_to_counts writes from the same file
    (tmp_path / "counts").mkdir()
    res = subprocess.run([COUNTS_TOOL, str(tmp_path / "counts" / "res"), "filled", "0", "0", "-", "3", base.path], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    plain = json.loads(res.stdout.strip().splitlines()[-1])
    assert {k: stats[k] for k in ("total_reads", "cant_parse", "low_quality", "saved")} == {k: plain[k] for k in ("total_reads", "cant_parse", "low_quality", "saved")}
    a, b = rr.read_rds(str(tmp_path / "res.rds")), rr.read_rds(str(tmp_path / "counts" / "res.rds"))
    assert a.names == b.names
    for key in a.names:
        assert _plain(a[key]) == _plain(b[key]), key


def test_pipelined_window_order(tmp_path, base):
    stats = run(tmp_path, "filled", [base.path], env=dict(SMALL_WINDOWS, DROPEST_BAM_PIPELINE="1"))
    assert stats["files"][0]["windows"] >= 3
    check_output(tmp_path, "base", base, stats["files"][0])


def test_windows_that_go_through_the_host(tmp_path, two_lengths):
    """UMI quality strings of two lengths: the container takes such a window record by record from the host's bytes; the tagged output is made
    before that and does not depend on it"""
    stats = run(tmp_path, "filled", [two_lengths.path], env=SMALL_WINDOWS)
    assert stats["files"][0]["windows"] >= 3 and stats["saved"] == len(two_lengths.records)
    check_output(tmp_path, "lengths", two_lengths, stats["files"][0])


def test_two_input_files_two_outputs(tmp_path, base, two_lengths):
    stats = run(tmp_path, "filled", [two_lengths.path, base.path], env=SMALL_WINDOWS)
    assert [f["name"] for f in stats["files"]] == ["lengths.tagged.bam", "base.tagged.bam"]
    check_output(tmp_path, "lengths", two_lengths, stats["files"][0])
    check_output(tmp_path, "base", base, stats["files"][1])
    assert stats["saved"] == len(base.records) + len(two_lengths.records)


def test_file_with_no_accepted_record(tmp_path, two_lengths):
    """(beside a file that has some, so that the estimation behind the ingest has reads to work on)"""
    recs = [bw.record(0, i, "r%d" % i, flag=4, tags=[("CB", "Z", "ACGT"), ("UB", "Z", "ACGT")]) for i in range(200)]
    inp = Input(str(tmp_path / "none.bam"), recs)
    assert inp.records == [] and inp.want == inp.header
    stats = run(tmp_path, "filled", [inp.path, two_lengths.path])
    assert stats["saved"] == len(two_lengths.records)
    check_output(tmp_path, "none", inp, stats["files"][0])                 # the header and the end-of-file block
    assert stats["files"][0]["records"] == 0


def test_read_names_as_the_source(tmp_path):
    cfg = bm.Cfg(tags=CFG.tags, filled_bam=False, read_type=True, intronic=b"N", intergenic=b"I", n_refs=len(REFS))
    inp = Input(str(tmp_path / "names.bam"), make_records(False, False, seed=8, n=3_000), cfg=cfg, block=997)
    stats = run(tmp_path, "name", [inp.path], env=SMALL_WINDOWS)
    assert stats["saved"] == len(inp.records) > 2_000
    check_output(tmp_path, "names", inp, stats["files"][0])


@pytest.mark.parametrize("stream", ["sparse", "dense"])
def test_genes_from_an_annotation(tmp_path, stream):
    """-g: the gene names come from the annotation's name pool and the marks from its verdict (checked against tests/annotation_model.py): a read
    that spans exons and introns gets no read-type tag, a record on a reference the annotation lacks is not written.  In the dense annotation
    many reads end where more than 16 transcripts lie: the annotation kernel leaves those to the host, whose gene and mark the tag kernels are
    then given (dropest_bam_decoder_patch_annotation) -- the output is the model's all the same."""
    import annotation_cases as ac
    case = ac.make(tmp_path, stream)
    model = case.model
    refs = [(c, 1_000_000) for c in case.chromosomes] + [("chrUn", 1000)]
    usable = [(c, p, e) for c, p, e in case.queries if c in case.chromosomes and e > p and e < 1_000_000]
    usable = usable[::max(1, len(usable) // 4000)]                           # (every n-th query: all kinds of them)
    n_deep = sum(1 for q in usable if max(model.depths_of_read(*q)) > 16)
    assert (n_deep > 100) if stream == "dense" else (n_deep == 0)
    rng = np.random.default_rng(3)
    recs, overrides, marks = [], [], set()
    for i, (chr_, p, end) in enumerate(usable):
        cb = "".join(rng.choice(list("ACGT"), 12)); umi = "".join(rng.choice(list("ACGT"), 8))
        rid = len(refs) - 1 if i % 50 == 0 else case.chromosomes.index(chr_)
        ln = end - p
        recs.append(bw.record(rid, p, "r%d" % i, seq="ACGT", cigar=[(ln, "M")] if ln < 4 else [(4, "M"), (ln - 4, "N")], qual=b"\x20" * 4,
                              tags=[("GX", "Z", "FROM_THE_TAG"), ("CB", "Z", cb), ("RE", "A", "N"), ("UB", "Z", umi)]))
        got = model.gene_for_read(chr_, p, end) if rid < len(case.chromosomes) else None
        overrides.append(None if got is None else (got[0].encode(), got[1]))
        if got is not None:
            marks.add(got[1])
    # exonic and intronic reads, spanning ones (several bits), reads outside every gene (no bit under -g), a reference the annotation lacks
    assert None in overrides and {0, 2, 4} <= marks and any(m in (3, 5, 6, 7) for m in marks) and any(o and o[0] for o in overrides)
    cfg = bm.Cfg(tags=CFG.tags, filled_bam=True, read_type=True, intronic=b"N", intergenic=b"I", n_refs=len(refs))
    inp = Input(str(tmp_path / "ann.bam"), recs, cfg=cfg, refs=refs, overrides=overrides)
    stats = run(tmp_path, "filled", [inp.path], env=dict(SMALL_WINDOWS, DROPEST_GTF=case.path))
    assert stats["saved"] == len(inp.records) and stats["cant_parse"] == sum(1 for o in overrides if o is None)
    check_output(tmp_path, "ann", inp, stats["files"][0])
    assert any(b"REAN" in r and b"REZ" not in r for r in inp.records)      # a spanning read keeps its old RE entry and gets none


def test_read_parameter_files_are_refused(tmp_path, two_lengths):
    params = str(tmp_path / "p.gz")
    with gzip.open(params, "wt") as f:
        f.write("r1 ACGT ACGT IIII IIII\n")
    res = run(tmp_path, "params:" + params, [two_lengths.path], expect_failure=True)
    assert res.returncode != 0 and "read-parameter files" in res.stderr and "-b" in res.stderr
    said = json.loads(res.stdout.strip().splitlines()[-1])
    assert said == {"error": True, "total_reads": 0, "cant_parse": 0, "low_quality": 0, "saved": 0, "files_written": 0}      # nothing was read into the container
    assert not os.path.exists(str(tmp_path / "lengths.tagged.bam"))
