"""The device BAM path feeding a SHARDED container (BamController -> dropest_bam_decoder_* -> CellsDataContainer::add_records_packed_device
-> dropest_shard_push_reads_device): windows cut at quota boundaries, reads that came through add_record first, two files, -g, and the
configurations that still go to the host reader.  Every .rds is compared key by key with the roads that existed before: one context fed
by the device path, and the sharded container fed by the host reader."""
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

from dropest_amd import capi
from dropest_amd.build import build_facade
from dropest_amd.synth import SynthStream

import annotation_cases
import bam_writer as bw
import rds_reader as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tests", "cpp", "bam_sharded_device")
WL = os.path.join(ROOT, "dropest_amd", "data", "barcodes", "10x_aug_2016_split")
QUOTA = 7001
DEVICE = {"DROPEST_BAM_DEVICE": "1", "DROPEST_BAM_WINDOW_BLOCKS": "64", "DROPEST_BAM_TRACE": "1", "DROPEST_BAM_TRACE_READER": "1"}
REFS = [("chr%d" % i, 1_000_000) for i in range(25)] + [("chrLate", 1_000_000)]


def _plain(v):
    """An RObject tree (rds_reader) as plain python, for equality: (kind, value, attributes)."""
    if not isinstance(v, rr.RObject):
        if isinstance(v, np.ndarray):
            return [None if (isinstance(x, float) and x != x) else x for x in v.tolist()]
        if isinstance(v, (list, tuple)):
            return [_plain(x) for x in v]
        return v
    return (v.kind, _plain(v.value), {k: _plain(x) for k, x in sorted(v.attributes.items())})


def _same_rds(d1, d2):
    assert d1.names == d2.names and "reads_per_umi_per_cell" in d1.names
    for key in d1.names:
        if key == "merge_targets":      # (the order of that list is the reference's hash order)
            a, b = ({n: _plain(x) for n, x in zip(d.names or [], d.value)} for d in (d1[key], d2[key]))
            assert a == b
        else:
            assert _plain(d1[key]) == _plain(d2[key]), key


def _run(tmp, bams, env, mode="filled", wl="-", quota=0, pre="-", k=0, min_before=3, min_after=10):
    """-> (the .rds, {"saved", "shard_reads"}, stderr)"""
    build_facade()
    os.makedirs(str(tmp), exist_ok=True)
    out = str(tmp / "res")
    res = subprocess.run([TOOL, out, mode, str(min_before), str(min_after), wl, "2", str(quota), pre, str(k)] + bams, capture_output=True, text=True,
                         timeout=300, env=dict(os.environ, DROPEST_RPUPC="1", **env))
    assert res.returncode == 0, res.stdout + res.stderr
    return rr.read_rds(out + ".rds"), json.loads(res.stdout.strip().splitlines()[-1]), res.stderr


def _windows(stderr):
    """records of every window of the device path, in order (the reader's trace)"""
    return [int(x) for x in re.findall(r"\[bam\] window \d+: .*? blocks, (\d+) records", stderr)]


def _dealt(n, shards, quota=QUOTA):
    per = [0] * shards
    for shard, _, count in capi.deal_range(0, n, quota, shards):
        per[shard] += count
    return per


def _records(n_reads, qual=False, n_every=97, gene_prefix="G", seed_stream=None, late=None):
    """BAM records of a synthetic stream (a UMI with N every n_every-th read).  late = (from, gene prefix): reads from there on carry genes of
    another name, and every third of them lies on chrLate."""
    qrng = np.random.default_rng(31)
    s = SynthStream(n_reads=n_reads, n_cells=25, n_genes=300, umi_len=8, permille_neighbour=150, permille_intron=100, **(seed_stream or {}))
    cb, umi, gene, aux = s.generate_host()
    recs, rows = [], []
    for i in range(len(cb)):
        c, u = capi.unpack_code(cb[i]), capi.unpack_code(umi[i])
        if i % n_every == 0:
            u = u[:3] + "N" + u[4:]
        is_late = late is not None and i >= late[0]
        g = None if gene[i] == capi.NO_GENE else "%s%d" % (late[1] if is_late else gene_prefix, gene[i])
        mark = int(aux[i] >> 16) & 7
        ref = 25 if is_late and i % 3 == 0 else int(aux[i]) & 0xFFFF
        tags = [("CB", "Z", c), ("UB", "Z", u)]
        q = "".join(chr(int(x)) for x in qrng.integers(35, 74, 8)) if qual else None
        if qual:
            tags.append(("UQ", "Z", q))
        if g:
            tags += [("GX", "Z", g), ("RE", "A", "N" if mark & 4 else "E")]
        recs.append(bw.record(ref, i, "r%d" % i, tags=tags))
        rows.append((c, u, g, REFS[ref][0], (4 if mark & 4 else 2) if g else 1, q))
    return recs, rows


@pytest.mark.parametrize("wl,qual", [(False, False), (True, False), (False, True), (True, True)])
def test_windows_cut_at_quota_boundaries_write_the_same_rds(tmp_path, wl, qual):
    """The 60 000 reads of test_gpu_bam.py::test_sharded_container_writes_the_same_rds through the device path into three shards of quota 7 001:
    the .rds of one context fed by the device path, and of the three shards fed by the host reader."""
    recs, _ = _records(60_000, qual=qual)
    bam = str(tmp_path / "s.bam")
    bw.write_bam(bam, REFS, recs, block=16_000)
    wlf = WL if wl else "-"
    d_dev, st_dev, err = _run(tmp_path / "dev", [bam], dict(DEVICE, DROPEST_DEVICES="0,0,0"), wl=wlf, quota=QUOTA)
    assert "taken: 1" in err and "taken: 0" not in err, err          # (the parent commit hands a sharded container's file to the host reader)
    wins = _windows(err)
    assert len(wins) >= 3 and sum(wins) == 60_000 == st_dev["saved"], wins
    assert st_dev["shard_reads"] == _dealt(60_000, 3) == [QUOTA, QUOTA, 60_000 - 2 * QUOTA]
    ends = set(np.cumsum(wins).tolist())
    assert QUOTA not in ends and 2 * QUOTA not in ends               # both boundaries fall inside a window: two windows were cut
    d_one, st_one, err_one = _run(tmp_path / "one", [bam], DEVICE, wl=wlf)
    assert "taken: 1" in err_one and st_one["shard_reads"] == []
    d_host, st_host, _ = _run(tmp_path / "host", [bam], dict(DROPEST_DEVICES="0,0,0"), wl=wlf, quota=QUOTA)
    assert st_host["shard_reads"] == st_dev["shard_reads"]
    _same_rds(d_dev, d_one)
    _same_rds(d_dev, d_host)
    assert len(d_dev["merge_targets"].value) > 10 or not wl
    per_gene = d_dev["reads_per_umi_per_cell"]["reads_per_umi"].value
    with_quality = sum(1 for g in per_gene for e in g.value if len(e.value[1].value) == 8)
    assert (with_quality > 1000) if qual else (with_quality == 0)


def _tsv(path, rows):
    with open(path, "w") as f:
        for c, u, g, chr_, mark, q in rows:
            f.write("\t".join([c, u, g or "-", chr_, str(mark), q or "-"]) + "\n")


def test_reads_from_add_record_first_then_the_device_path(tmp_path):
    """1 500 reads through add_record leave a partial batch pending; the file's first window must come behind them, on the shard their count
    leads to.  Against one context fed the same way."""
    recs, _ = _records(20_000)
    bam = str(tmp_path / "s.bam")
    bw.write_bam(bam, REFS, recs, block=16_000)
    _, rows = _records(2_000, n_every=53, seed_stream=dict(seed=5))
    pre = str(tmp_path / "pre.tsv")
    _tsv(pre, rows)
    d_dev, st, err = _run(tmp_path / "dev", [bam], dict(DEVICE, DROPEST_DEVICES="0,0,0"), quota=QUOTA, pre=pre, k=1500)
    assert "taken: 1" in err and len(_windows(err)) >= 3
    assert st["saved"] == 20_000 and st["shard_reads"] == _dealt(21_500, 3)
    d_one, _, err_one = _run(tmp_path / "one", [bam], DEVICE, pre=pre, k=1500)
    assert "taken: 1" in err_one
    _same_rds(d_dev, d_one)


def test_two_files_the_second_with_new_genes_and_a_new_chromosome(tmp_path):
    """The dictionaries go on from file to file, and the second decoder starts on the shard the running count has reached."""
    recs_a, _ = _records(12_000)
    recs_b, _ = _records(12_000, n_every=89, seed_stream=dict(seed=9), late=(9_000, "H"))
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    bw.write_bam(a, REFS, recs_a, block=16_000)
    bw.write_bam(b, REFS, recs_b, block=16_000)
    d_dev, st, err = _run(tmp_path / "dev", [a, b], dict(DEVICE, DROPEST_DEVICES="0,0,0"), quota=QUOTA)
    assert err.count("taken: 1") == 2 and "taken: 0" not in err
    assert st["saved"] == 24_000 and st["shard_reads"] == _dealt(24_000, 3)
    d_host, st_host, _ = _run(tmp_path / "host", [a, b], dict(DROPEST_DEVICES="0,0,0"), quota=QUOTA)
    assert st_host["shard_reads"] == st["shard_reads"]
    _same_rds(d_dev, d_host)
    genes = rr.dgcmatrix_to_dense(d_dev["cm_raw"])[1]
    assert any(str(g).startswith("H") for g in genes) and any(str(g).startswith("G") for g in genes)


def test_read_parameter_files_still_go_to_the_host_reader(tmp_path):
    """-r on a sharded container with DROPEST_BAM_DEVICE=1: the device path declines the file (taken: 0) and the result is the host reader's."""
    _, rows = _records(8_000)
    recs, lines = [], []
    for i, (c, u, g, chr_, mark, _) in enumerate(rows):
        tags = [("GX", "Z", g), ("RE", "A", "N" if mark == 4 else "E")] if g else []
        recs.append(bw.record(REFS.index((chr_, 1_000_000)), i, "read%d" % i, tags=tags))
        lines.append("read%d %s %s %s %s" % (i, c, u, "I" * len(c), "I" * len(u)))
    bam, params = str(tmp_path / "r.bam"), str(tmp_path / "p.gz")
    bw.write_bam(bam, REFS, recs, block=16_000)
    with gzip.open(params, "wt") as f:
        f.write("\n".join(lines) + "\n")
    d_dev, st, err = _run(tmp_path / "dev", [bam], dict(DEVICE, DROPEST_DEVICES="0,0,0"), mode="params:" + params, quota=QUOTA)
    assert "taken: 0" in err and "taken: 1" not in err
    d_host, st_host, _ = _run(tmp_path / "host", [bam], dict(DROPEST_DEVICES="0,0,0"), mode="params:" + params, quota=QUOTA)
    assert st["saved"] == st_host["saved"] == 8_000 and st["shard_reads"] == st_host["shard_reads"] == _dealt(8_000, 3)
    _same_rds(d_dev, d_host)


def test_genes_from_a_gtf_on_two_shards(tmp_path):
    """-g: the annotation tables are made on the decoding shard's GPU; alignments over a small GTF, two shards."""
    case = annotation_cases.make(tmp_path, "sparse", seed=3, n_background=300, n_cross=300)
    refs = [("chr1", 1_000_000), ("chr2", 1_000_000), ("chrX", 1_000_000)]
    rng = np.random.default_rng(8)
    cb, umi, _, _ = SynthStream(n_reads=12_000, n_cells=15, n_genes=10, umi_len=8).generate_host()
    starts = [r for r in case.records if r.chr in ("chr1", "chr2", "chrX")]
    recs = []
    for i in range(len(cb)):
        r = starts[int(rng.integers(0, len(starts)))]
        p = max(0, r.start + int(rng.integers(-30, 30)))
        cigar = [[(40, "M")], [(5, "S"), (35, "M")], [(15, "M"), (int(rng.integers(50, 900)), "N"), (25, "M")]][int(rng.integers(0, 3))]
        recs.append(bw.record([x[0] for x in refs].index(r.chr), p, "r%d" % i, tags=[("CB", "Z", capi.unpack_code(cb[i])), ("UB", "Z", capi.unpack_code(umi[i]))], cigar=cigar))
    bam = str(tmp_path / "g.bam")
    bw.write_bam(bam, refs, recs, block=6_000)      # (records without gene tags are short: blocks small enough for more than three windows of 64)
    env = {"DROPEST_GTF": case.path}
    d_dev, st, err = _run(tmp_path / "dev", [bam], dict(DEVICE, DROPEST_DEVICES="0,0", **env), quota=5_003, min_before=2, min_after=3)
    assert "taken: 1" in err and len(_windows(err)) >= 3
    assert st["saved"] > 3_000 and st["shard_reads"] == _dealt(st["saved"], 2, 5_003)
    d_host, st_host, _ = _run(tmp_path / "host", [bam], dict(DROPEST_DEVICES="0,0", **env), quota=5_003, min_before=2, min_after=3)
    assert st_host == st
    _same_rds(d_dev, d_host)
    assert len(rr.dgcmatrix_to_dense(d_dev["cm_raw"])[1]) > 20
