"""Filtered BAM output (-F) at file level, through tests/cpp/bam_filtered: BAM file(s) -> container -> merge_and_filter ->
BamController::write_filtered_bam_files on the device BAM path.  The one `<first stem>.filtered.bam` it writes is BGZF with the end-of-file block and
inflates to the first input's header bytes followed by tests/bam_filter_model.py's records over the container's decisions (dumped by the tool as
strings); on a hand-built file the decisions themselves follow from how the file was made."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from dropest_amd.build import build_facade

import bam_filter_model as fm
import bam_model as bm
import bam_writer as bw
from test_gpu_bam_tag_window import _fillers
from test_gpu_bam_tagged_file import check_bgzf, REFS, SMALL_WINDOWS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tests", "cpp", "bam_filtered")
CFG = bm.Cfg(tags=("CB", "UB", "CQ", "UQ", "GX", "RE"), filled_bam=True, read_type=True, intronic=b"N", intergenic=b"I", n_refs=len(REFS))
OUT = fm.FilterOutCfg(read_type="RE", exonic=b"E", intronic=b"N", intergenic=b"I")      # the tool's tags (as bam_tagged: RE with N / I / E)
WRITTEN, NO_GENE, CELL_NOT_KEPT, WRONG_GENE, WRONG_UMI = range(5)


def run(cwd, bams, merge="none", min_after=2, umi="simple", save=1, mode="filled", env=None, dump=True, expect_failure=False):
    """-> (the tool's JSON line, the dumped decisions [(verdict, cb, umi)]); with expect_failure the finished process"""
    build_facade()
    e = dict(os.environ, **(env or {}))
    dump_path = os.path.join(str(cwd), "decisions.txt")
    if dump:
        e["DROPEST_FILTER_DUMP"] = dump_path
    res = subprocess.run([TOOL, mode, merge, "0", str(min_after), umi, str(save)] + bams, capture_output=True, text=True, timeout=300, cwd=str(cwd), env=e)
    if expect_failure:
        return res
    assert res.returncode == 0, res.stdout + res.stderr
    decisions = []
    for line in open(dump_path):
        v, cb, u = line.split()
        decisions.append((int(v), b"" if cb == "-" else cb.encode(), b"" if u == "-" else u.encode()))
    return json.loads(res.stdout.strip().splitlines()[-1]), decisions


def header_of(path):
    raw = gzip.decompress(open(path, "rb").read())
    return raw[:bm.records_of(raw)[0]]


def check_output(cwd, stem, header, recs, stats, decisions):
    """the file is BGZF ending in the end-of-file block; inflated, the header and the model's records; the counters agree with the decisions"""
    blob = open(os.path.join(str(cwd), stem + ".filtered.bam"), "rb").read()
    n_blocks, total = check_bgzf(blob)
    got = gzip.decompress(blob)
    body, written, used = fm.filtered_stream(recs, CFG, OUT, decisions)
    assert used == len(decisions)                                               # read i of the container is the i-th accepted record
    want = header + body
    assert total == len(got) == len(want) and got == want
    verdicts = [d[0] for d in decisions]
    assert stats["name"] == stem + ".filtered.bam" and stats["total_reads"] == len(decisions)
    assert stats["written"] == written == verdicts.count(WRITTEN)
    assert stats["wrong_genes"] == verdicts.count(WRONG_GENE) and stats["wrong_umis"] == verdicts.count(WRONG_UMI)
    assert stats["inflated_bytes"] == len(want) and stats["compressed_bytes"] == len(blob)
    return n_blocks


# ---- (a) a hand-built file: its answers follow from construction -----------------------------------------------------------------------------
K, S = "ACGTACGATTAC", "TTGGCCCCAAGG"            # on the whitelist: K gets three genes (kept), S one (under min_genes_after_merge = 2)
M, M2 = "ACGTACGATTAA", "TTGGCCCCAAGA"           # one mismatch from K / from S, not on the whitelist
HAND = [   # (barcode, UMI, gene, flag)
    (K, "AAAACCCC", "G1", 0), (K, "AAAACCCC", "G1", 0),
    (K, "AAAACCCN", "G1", 0),                    # 2: exactly one UMI of (K, G1) within one mismatch: AAAACCCC
    (K, "GGGGTTTT", "G2", 0), (K, "CCCCAAAA", "G3", 0),
    (K, "TTTTGGGG", None, 0),                    # 5: no gene
    (K, "TTTTGGGG", "G1", 4),                    # unmapped: not accepted, takes no decision
    (S, "ACACACAC", "G1", 0), (S, "GTGTGTGT", "G1", 0),                                   # 6, 7 (among the accepted): cell not kept
    (M, "GGGGTTTT", "G2", 0), (M, "CCCCAAAA", "G3", 0), (M, "AAAACCCC", "G1", 0),         # 8, 9, 10: K's molecules, so M merges into K
    (M2, "ACACACAC", "G1", 0), (M2, "GTGTGTGT", "G1", 0),                                 # 11, 12: S's molecules; the target is not kept
] + [(K, u, g, 0) for u, g in (("GTCAGTCA", "G1"), ("TGACTGAC", "G2"), ("CATGCATG", "G3"), ("GATCGATC", "G1"), ("CTAGCTAG", "G2"), ("AGTCAGTC", "G3"),
                                ("TCGATCGA", "G1"), ("GTCAGTCA", "G2"), ("TGACTGAC", "G3"), ("CATGCATG", "G1"), ("GACTGACT", "G2"), ("ATATCGCG", "G3"))]


def hand_records(rows, first=0):
    recs = []
    for i, (cb, umi, gene, flag) in enumerate(rows):
        tags = [("NH", "i", i), ("CB", "Z", cb), ("UB", "Z", umi)] + ([("GX", "Z", gene)] if gene else []) + ([("UR", "Z", "old")] if i % 3 == 0 else [])
        recs.append(bw.record(i % 4, 100 + i, "h%d" % (first + i), flag=flag, seq="ACGT" * 6, tags=tags))
    return recs


def whitelist(tmp_path):
    path = str(tmp_path / "whitelist.txt")
    rc = lambda s: s[::-1].translate(str.maketrans("ACGT", "TGCA"))      # the file holds reverse complements (BarcodesParser::read_line)
    # two parts of six bases, one part per line: K, S and the two mixed barcodes are on the whitelist
    open(path, "w").write("%s %s\n%s %s\n" % (rc(K[:6]), rc(S[:6]), rc(K[6:]), rc(S[6:])))
    return path


@pytest.mark.parametrize("save", [1, 0])
def test_hand_built_file(tmp_path, save):
    recs = hand_records(HAND)
    path = str(tmp_path / "hand.bam")
    bw.write_bam(path, REFS, recs, block=700)
    stats, dec = run(tmp_path, [path], merge="real:" + whitelist(tmp_path), min_after=2, save=save)
    assert len(dec) == len(HAND) - 1
    acc = [r for r in HAND if r[3] == 0]
    for k, (cb, umi, gene, _) in enumerate(acc):
        v, out_cb, out_umi = dec[k]
        if gene is None:
            assert v == NO_GENE
        elif cb in (S, M2):
            assert v == CELL_NOT_KEPT                                          # S has one gene; M2's target is S (or itself): not kept either way
        elif "N" in umi:
            # save_umi_merge_targets: the read is written under its one target; without the targets nobody knows where the UMI went
            assert (v, out_cb, out_umi) == ((WRITTEN, K.encode(), b"AAAACCCC") if save else (WRONG_UMI, K.encode(), umi.encode()))
        else:
            assert (v, out_cb, out_umi) == (WRITTEN, K.encode(), umi.encode())  # K's own reads, and M's under K's barcode
    assert stats["wrong_umis"] == (0 if save else 1) and stats["wrong_genes"] == 0
    assert stats["written"] == sum(1 for r in acc if r[2] and r[0] in (K, M)) - (0 if save else 1)
    check_output(tmp_path, "hand", header_of(path), recs, stats, dec)


# ---- (b) ~20 000 records with every kind of aux entry, a few dozen kept cells and thousands that are not ---------------------------------------
def varied_records(n, seed):
    rng = np.random.default_rng(seed)
    fill = _fillers()
    genes = ["GENE%d" % i for i in range(40)]
    big = ["".join(rng.choice(list("ACGT"), 12)) for _ in range(40)]
    recs = []
    for i in range(n):
        cb = big[int(rng.integers(0, len(big)))] if rng.random() < 0.6 else "".join(rng.choice(list("ACGT"), 12))
        umi = "".join(rng.choice(list("ACGT"), 8))
        if i % 211 == 0:
            cb = cb[:5] + "N" + cb[6:]
        if i % 223 == 0:
            umi = umi[:2] + "N" + umi[3:]
        g = None if i % 9 == 0 else genes[int(rng.integers(0, len(genes)))]
        rt = [None, "N", "I", "E"][i % 4] if g else None
        tags = []
        if i % 5 == 0:
            tags.append(("CR", "Z", "OLDOLD"))
        tags += [("CB", "Z", cb), fill[i % len(fill)]]
        if i % 7 == 0:
            tags.append(("UR", "i", 77))
        tags += [("UB", "Z", umi), fill[(i * 7 + 3) % len(fill)], ("UQ", "Z", "".join(chr(33 + int(x)) for x in rng.integers(2, 40, 8)))]
        if i % 6 == 1:
            tags.append(("CQ", "Z", "".join(chr(33 + int(x)) for x in rng.integers(2, 40, 12))))
        if g:
            tags.append(("GX", "Z", g))
        if rt:
            tags.append(("RE", "A" if i % 8 < 4 else "Z", rt))
        if i % 11 == 0:
            tags.append(("CB", "Z", "AGAIN"))                                  # the corrected tag's name a second time
        if i % 301 == 7:
            tags.append(b"QQ?" + b"UBZbehind the stop\x00")                    # ... and behind the point where the walk stops
        flag, ref = 0, int(rng.integers(0, 4))
        if i % 97 == 1:
            flag = 4
        elif i % 97 == 2:
            flag = 0x100
        elif i % 97 == 3:
            ref = -1
        elif i % 97 == 4:
            tags = [t for t in tags if not (isinstance(t, tuple) and t[0] == "UB")]
        recs.append(bw.record(ref, i, "r%d" % i, flag=flag, tags=tags))
    return recs


@pytest.fixture(scope="module")
def varied(tmp_path_factory):
    d = tmp_path_factory.mktemp("filtered_varied")
    path = str(d / "varied.bam")
    recs = varied_records(20_000, seed=17)
    bw.write_bam(path, REFS, recs, block=12_345)
    return path, recs, header_of(path)


def test_varied_file_in_both_window_orders(tmp_path, varied):
    path, recs, header = varied
    stats, dec = run(tmp_path, [path], min_after=10, env=SMALL_WINDOWS)
    verdicts = [d[0] for d in dec]
    assert verdicts.count(WRITTEN) >= 2000 and verdicts.count(CELL_NOT_KEPT) >= 2000 and verdicts.count(NO_GENE) >= 1000      # else this proves nothing
    assert 24 <= len({d[1] for d in dec if d[0] == WRITTEN}) <= 60                                                            # a few dozen kept cells
    assert stats["windows"] >= 3 and stats["batches"] >= 3
    n_blocks = check_output(tmp_path, "varied", header, recs, stats, dec)
    assert n_blocks > stats["inflated_bytes"] // 65280                          # full chunks + the end-of-file block
    first = open(str(tmp_path / "varied.filtered.bam"), "rb").read()
    (tmp_path / "pipelined").mkdir()
    stats_p, dec_p = run(tmp_path / "pipelined", [path], min_after=10, env=dict(SMALL_WINDOWS, DROPEST_BAM_PIPELINE="1"))
    assert dec_p == dec
    assert gzip.decompress(open(str(tmp_path / "pipelined" / "varied.filtered.bam"), "rb").read()) == gzip.decompress(first)
    for key in ("name", "total_reads", "written", "wrong_genes", "wrong_umis", "inflated_bytes"):
        assert stats_p[key] == stats[key]
    assert stats_p["windows"] >= 3 and stats_p["batches"] >= 3


# ---- (c) two inputs: one output, named after the first, with the first's header ----------------------------------------------------------------
@pytest.fixture(scope="module")
def two_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("filtered_two")
    rows_b = [(K, "GTCAGTCA", "G1", 0), (K, "AAAACCCC", "G1", 0), (S, "ACACACAC", "G1", 0), (K, "TTTTAAAA", None, 0), (K, "CGCGCGCG", "G2", 0)]
    recs_a, recs_b = hand_records(HAND), hand_records(rows_b, first=100)
    a, b = str(d / "first.bam"), str(d / "second.bam")
    bw.write_bam(a, REFS, recs_a, block=700)
    bw.write_bam(b, REFS + [("chrX", 5000)], recs_b, block=700, header_text="@HD\tVN:1.6\tSO:unsorted\n@CO\tthe second file\n")
    return a, b, recs_a, recs_b


def test_two_inputs_make_one_output(tmp_path, two_files):
    a, b, recs_a, recs_b = two_files
    assert header_of(a) != header_of(b)
    stats, dec = run(tmp_path, [a, b], min_after=2)
    assert len(dec) == len(recs_a) - 1 + len(recs_b)
    assert [d[0] for d in dec[-len(recs_b):]] == [WRITTEN, WRITTEN, CELL_NOT_KEPT, NO_GENE, WRITTEN]
    check_output(tmp_path, "first", header_of(a), recs_a + recs_b, stats, dec)
    assert sorted(f for f in os.listdir(str(tmp_path)) if f.endswith(".bam")) == ["first.filtered.bam"]      # no second.filtered.bam


# ---- (d) what is refused ------------------------------------------------------------------------------------------------------------------
def refused(res, cwd, *words):
    assert res.returncode == 1, res.stdout + res.stderr
    for w in words:
        assert w in res.stderr, res.stderr
    lines = res.stdout.strip().splitlines()
    if lines:                                                                   # no half-written claim in filtered_file()
        claim = json.loads(lines[-1])
        assert claim["error"] is True and claim["name"] == "" and claim["windows"] == 0 and claim["total_reads"] == 0 and claim["written"] == 0
    assert [f for f in os.listdir(str(cwd)) if f.endswith(".filtered.bam")] == []      # ... and no half-written file


def test_other_files_than_the_container_was_filled_from(tmp_path, two_files):
    a, b, recs_a, recs_b = two_files
    for k, second in enumerate(([b, a], [a], [b], [a, b, b], [a, a])):
        cwd = tmp_path / ("case%d" % k)
        cwd.mkdir()
        res = run(cwd, [a, b], min_after=2, dump=False, env={"DROPEST_FILTER_FILES": ":".join(second)}, expect_failure=True)
        refused(res, cwd, "not the files the container was filled from")


def test_a_sharded_container_is_refused(tmp_path, two_files):
    a, b, _, _ = two_files
    res = run(tmp_path, [a, b], min_after=2, dump=False, env={"DROPEST_DEVICES": "0,0"}, expect_failure=True)
    refused(res, tmp_path, "Filtered BAM output (-F)", "shard")


def test_read_parameter_files_are_refused(tmp_path):
    rows = [(K, "AAAACCCC", "G1"), (K, "GGGGTTTT", "G2"), (S, "ACACACAC", "G1")]
    recs = [bw.record(0, 10 + i, "p%d" % i, tags=[("GX", "Z", g)]) for i, (_, _, g) in enumerate(rows)]
    path, params = str(tmp_path / "r.bam"), str(tmp_path / "params.gz")
    bw.write_bam(path, REFS, recs)
    with gzip.open(params, "wt") as f:
        for i, (cb, umi, _) in enumerate(rows):
            f.write("p%d %s %s %s %s\n" % (i, cb, umi, "I" * len(cb), "I" * len(umi)))
    res = run(tmp_path, [path], mode="params:" + params, min_after=1, dump=False, expect_failure=True)
    refused(res, tmp_path, "Filtered BAM output (-F)", "read-parameter files (-r)")
