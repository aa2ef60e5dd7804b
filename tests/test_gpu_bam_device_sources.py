"""-r (read-parameter files) and -P (gene = chromosome name) on the device BAM path, behind BamController::set_device_read_sources, through
tests/cpp/bam_sources: the files are taken by the device path (taken: 1) and the .rds is the host reader's and the oracle's; with the switch
off everything is as before (taken: 0)."""
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

from dropest_amd.build import SOURCES_TOOL, build_facade
from oracle import Oracle

import bam_writer as bw
import rds_reader as rr
from test_gpu_bam import _reads
from test_gpu_bam_sharded_device import _same_rds

pytestmark = pytest.mark.gpu
REFS = [("chr%d" % i, 1_000_000) for i in range(25)]
DEVICE = {"DROPEST_BAM_DEVICE": "1", "DROPEST_BAM_TRACE": "1"}
SMALL = dict(DEVICE, DROPEST_BAM_WINDOW_BLOCKS="64")


def run(tmp, mode, bams, sources, chromosome_gene=0, env=None, devices="-", quota=0, min_before=3, min_after=5, ok=True):
    """-> (matrix {(gene, cell): count}, cells, counters, the .rds, stderr)"""
    build_facade()
    os.makedirs(str(tmp), exist_ok=True)
    out = str(tmp / "res")
    res = subprocess.run([SOURCES_TOOL, out, mode, str(chromosome_gene), str(sources), str(min_before), str(min_after), "-", "3", devices, str(quota)] + bams,
                         capture_output=True, text=True, timeout=300, cwd=str(tmp), env=dict(os.environ, DROPEST_RPUPC="1", **(env or {})))
    if not ok:
        assert res.returncode != 0
        return res.stderr
    assert res.returncode == 0, res.stdout + res.stderr
    stats = json.loads(res.stdout.strip().splitlines()[-1])
    d = rr.read_rds(out + ".rds")
    cm, genes, cells = rr.dgcmatrix_to_dense(d["cm"])
    got = {(genes[r], cells[c]): int(cm[r, c]) for r, c in zip(*np.nonzero(cm))}
    return got, cells, {k: stats[k] for k in ("total_reads", "cant_parse", "low_quality", "saved")}, d, res.stderr


def taken(err):
    return [int(x) for x in re.findall(r"\(taken: (\d)\)", err)]


def oracle(kept, min_before=3, min_after=5):
    o = Oracle(min_genes_before=min_before, min_genes_after=min_after)
    for cb, umi, g, chr_, m, q in kept:
        o.add_record(cb, umi, g or "", chr_, m, **({"umi_qual": q} if q else {}))
    o.set_initialized(); o.merge_and_filter()
    gi, ci, v = o.count_matrix(filtered=True)
    cols = [o.cell_barcode(int(k)) for k in o.filtered_cells()]
    return {(o.gene_name(int(g)), cols[int(c)]): int(x) for g, c, x in zip(gi, ci, v)}, cols


def construction(n_reads, seed, first=0, taken_names=(), quality_lengths=(8,)):
    """The construction of test_gpu_bam.py::test_read_parameter_files: reads without a row, rows of low quality, names aligned twice, repeated
    rows, '@', broken rows -- and barcodes with N.  first: the number of the first read's name; taken_names: names of an earlier file, aligned
    again here (they cannot be parsed any more).  -> records, row lines, the reads that are kept, the counts of each kind"""
    reads = _reads(n_reads, seed_cells=12)
    rng = np.random.default_rng(seed)
    recs, rows, kept = [], [], []
    n = dict(missing=0, low=0, dup=0, repeated=0, with_n=0, again=0)
    for i, (cb, umi, g, chr_, mark) in enumerate(reads):
        if g is None:
            tags, m = [], 1
        else:
            code, m = (("N", 4) if mark & 4 else ("I", 1) if mark == 1 else ("E", 2))
            tags = [("GX", "Z", g), ("RE", "A", code)]
        name = "read%d" % (first + i)
        recs.append(bw.record(int(chr_[3:]), i, name, tags=tags))
        kind = int(rng.integers(0, 30))
        if kind == 0:
            n["missing"] += 1; continue
        low = kind == 1
        if kind == 4:
            cb = cb[:5] + "N" + cb[6:]; n["with_n"] += 1
        half = i * len(quality_lengths) // len(reads)      # (every length has cells of its own: a molecule's reads must agree on it, UMI.cpp:26-28)
        if len(quality_lengths) > 1:
            cb = "ACGT"[half] * 3 + cb[3:]
        ql = quality_lengths[half]
        qcb = "".join(chr(int(x)) for x in rng.integers(53, 74, len(cb)))
        qumi = "".join(chr(int(x)) for x in rng.integers(53, 74, ql))
        if low:
            qumi = qumi[:2] + chr(33 + 5) + qumi[3:]; n["low"] += 1
        rows.append("%s%s %s %s %s %s" % ("@" if i % 2 else "", name, cb, umi, qcb, qumi))
        if kind == 2:
            recs.append(bw.record(int(chr_[3:]), i, name, tags=tags)); n["dup"] += 1
        if kind == 3:
            rows.append("%s %s %s %s %s" % (name, "AAAA", "CCCC", "IIII", "IIII")); n["repeated"] += 1
        if not low:
            kept.append((cb, umi, g, chr_, m, qumi))
    for name in taken_names:
        recs.insert(int(rng.integers(0, len(recs))), bw.record(3, 77, name, tags=[("GX", "Z", "ENSG00001")])); n["again"] += 1
    rows.insert(5, "broken row without enough fields")
    rows.insert(9, "emptycb  ACGT II II")
    return recs, rows, kept, n


def write_params(tmp, rows, parts=2):
    paths = []
    for k in range(parts):
        part = rows[len(rows) * k // parts:len(rows) * (k + 1) // parts]
        paths.append(str(tmp / ("p%d.gz" % k)))
        with gzip.open(paths[-1], "wb") as f:
            f.write(("\n".join(part) + ("\n" if k % 2 == 0 else "")).encode())      # (the second file's last line has no newline)
    return "params:" + " ".join(paths)


def guards(n, want):
    assert n["missing"] >= 20 and n["low"] >= 20 and n["dup"] >= 20 and n["repeated"] >= 20 and n["with_n"] >= 10 and len(want) >= 300, (n, len(want))


@pytest.fixture(scope="module")
def one_file(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sources")
    recs, rows, kept, n = construction(6_000, 17)
    mode = write_params(tmp, rows)
    bam = str(tmp / "r.bam")
    bw.write_bam(bam, REFS, recs, block=1_500)
    want, cols = oracle(kept)
    guards(n, want)
    host = run(tmp / "host", mode, [bam], 1, env={"DROPEST_MIN_PHRED": "10"})
    return dict(mode=mode, bam=bam, want=want, cols=cols, n=n, kept=kept, n_recs=len(recs), host=host)


def check_counters(f, stats):
    n = f["n"]
    assert stats == dict(total_reads=f["n_recs"], cant_parse=n["missing"] + n["dup"], low_quality=n["low"], saved=len(f["kept"]))


def test_parameter_files_on_the_device_path(one_file, tmp_path):
    f = one_file
    got_h, cells_h, stats_h, d_h, err_h = f["host"]
    assert taken(err_h) == [] and got_h == f["want"] and cells_h == f["cols"]
    check_counters(f, stats_h)
    got, cells, stats, d, err = run(tmp_path / "on", f["mode"], [f["bam"]], 1, env=dict(DEVICE, DROPEST_MIN_PHRED="10"))
    assert taken(err) == [1], err
    assert got == f["want"] and cells == f["cols"]
    check_counters(f, stats)
    _same_rds(d, d_h)
    # the switch off: everything as before
    got, cells, stats, d, err = run(tmp_path / "off", f["mode"], [f["bam"]], 0, env=dict(DEVICE, DROPEST_MIN_PHRED="10"))
    assert taken(err) == [0], err
    check_counters(f, stats)
    _same_rds(d, d_h)


@pytest.mark.parametrize("order", ["one-by-one", "pipelined"])
def test_small_windows_in_both_orders(one_file, tmp_path, order):
    f = one_file
    env = dict(SMALL, DROPEST_MIN_PHRED="10", **({"DROPEST_BAM_PIPELINE": "1"} if order == "pipelined" else {}))
    got, cells, stats, d, err = run(tmp_path, f["mode"], [f["bam"]], 1, env=env)
    assert taken(err) == [1] and int(re.search(r"device path: (\d+) windows", err).group(1)) >= 4, err
    check_counters(f, stats)
    _same_rds(d, f["host"][3])


def test_sharded_container_with_a_small_quota(one_file, tmp_path):
    f = one_file
    env = dict(SMALL, DROPEST_MIN_PHRED="10")
    got, cells, stats, d, err = run(tmp_path / "dev", f["mode"], [f["bam"]], 1, env=env, devices="0,0,0", quota=701)
    assert taken(err) == [1], err
    d_h = run(tmp_path / "host", f["mode"], [f["bam"]], 1, env={"DROPEST_MIN_PHRED": "10"}, devices="0,0,0", quota=701)[3]
    check_counters(f, stats)
    _same_rds(d, d_h)


def test_two_files_over_one_table(tmp_path):
    """names of the first file aligned again in the second: their rows are taken"""
    recs1, rows1, kept1, n1 = construction(3_000, 5)
    again = ["read%d" % i for i in range(0, 3_000, 50)]
    recs2, rows2, kept2, n2 = construction(3_000, 6, first=3_000, taken_names=again)
    mode = write_params(tmp_path, rows1 + rows2, parts=3)
    bams = [str(tmp_path / "a.bam"), str(tmp_path / "b.bam")]
    bw.write_bam(bams[0], REFS, recs1, block=1_500); bw.write_bam(bams[1], REFS, recs2, block=1_500)
    want, cols = oracle(kept1 + kept2)
    guards({k: n1[k] + n2[k] for k in n1}, want)
    assert n2["again"] == 60
    got_h, cells_h, stats_h, d_h, _ = run(tmp_path / "host", mode, bams, 1, env={"DROPEST_MIN_PHRED": "10"})
    assert got_h == want and cells_h == cols
    got, cells, stats, d, err = run(tmp_path / "dev", mode, bams, 1, env=dict(SMALL, DROPEST_MIN_PHRED="10"))
    assert taken(err) == [1, 1], err
    assert stats == stats_h and stats["saved"] == len(kept1) + len(kept2) and stats["cant_parse"] == sum(n[k] for n in (n1, n2) for k in ("missing", "dup", "again"))
    _same_rds(d, d_h)


def test_quality_strings_of_two_lengths_go_through_the_host(tmp_path):
    recs, rows, kept, n = construction(6_000, 8, quality_lengths=(8, 6))
    mode = write_params(tmp_path, rows)
    bam = str(tmp_path / "q.bam")
    bw.write_bam(bam, REFS, recs, block=1_500)
    got_h, cells_h, stats_h, d_h, _ = run(tmp_path / "host", mode, [bam], 1, env={"DROPEST_MIN_PHRED": "10"})
    got, cells, stats, d, err = run(tmp_path / "dev", mode, [bam], 1, env=dict(SMALL, DROPEST_MIN_PHRED="10"))
    assert taken(err) == [1], err
    assert stats == stats_h and stats["saved"] == len(kept) and stats["low_quality"] == n["low"]
    _same_rds(d, d_h)


@pytest.fixture(scope="module")
def chromosome_genes(tmp_path_factory):
    """reads over 25 references; the oracle is fed gene = chromosome name with mark 2"""
    tmp = tmp_path_factory.mktemp("chromosome")
    reads = _reads(6_000, seed_cells=15)
    recs, kept = [], []
    for i, (cb, umi, g, chr_, mark) in enumerate(reads):
        tags = [("GX", "Z", g), ("RE", "A", "N")] if g and i % 2 else []          # (neither is looked at)
        recs.append(bw.record(int(chr_[3:]), i, "r%d!%s#%s" % (i, cb, umi), tags=tags))
        kept.append((cb, umi, chr_, chr_, 2, ""))
    bam = str(tmp / "c.bam")
    bw.write_bam(bam, REFS, recs, block=1_500)
    want, cols = oracle(kept, 3, 5)
    assert len(want) >= 300 and len({g for g, _ in want}) == 25
    gtf = str(tmp / "a.gtf")
    with open(gtf, "w") as fh:
        fh.write('chr1\ts\texon\t1\t500000\t.\t+\t.\tgene_id "A"; transcript_id "T";\n')
    return dict(bam=bam, want=want, cols=cols, n=len(recs), gtf=gtf, recs=recs, tmp=tmp)


@pytest.mark.parametrize("with_gtf", [False, True], ids=["no-gtf", "gtf"])
def test_gene_is_the_chromosome_name(chromosome_genes, tmp_path, with_gtf):
    f = chromosome_genes
    extra = {"DROPEST_GTF": f["gtf"]} if with_gtf else {}
    got_h, cells_h, stats_h, d_h, err_h = run(tmp_path / "host", "name", [f["bam"]], 1, chromosome_gene=1, env=extra)
    assert got_h == f["want"] and cells_h == f["cols"] and stats_h["saved"] == f["n"] and taken(err_h) == []
    got, cells, stats, d, err = run(tmp_path / "dev", "name", [f["bam"]], 1, chromosome_gene=1, env=dict(SMALL, **extra))
    assert taken(err) == [1], err
    assert got == f["want"] and cells == f["cols"] and stats == stats_h
    _same_rds(d, d_h)
    _, _, stats, d, err = run(tmp_path / "off", "name", [f["bam"]], 0, chromosome_gene=1, env=dict(SMALL, **extra))
    assert taken(err) == [0] and stats == stats_h
    _same_rds(d, d_h)


def test_chromosome_genes_with_parameter_files(one_file, tmp_path):
    f = one_file
    d_h = run(tmp_path / "host", f["mode"], [f["bam"]], 1, chromosome_gene=1, env={"DROPEST_MIN_PHRED": "10"})
    got, cells, stats, d, err = run(tmp_path / "dev", f["mode"], [f["bam"]], 1, chromosome_gene=1, env=dict(SMALL, DROPEST_MIN_PHRED="10"))
    assert taken(err) == [1], err
    check_counters(f, stats)
    assert stats == d_h[2] and got == d_h[0] and len({g for g, _ in got}) == 25
    _same_rds(d, d_h[3])


@pytest.mark.parametrize("switch", ["0", "1"])
def test_output_stays_refused(one_file, chromosome_genes, tmp_path, switch):
    f, c = one_file, chromosome_genes
    err = run(tmp_path / "b", f["mode"], [f["bam"]], switch + "b", env=DEVICE, ok=False)
    assert "Tagged BAM output (-b) is written on the device BAM path only, which this configuration cannot take: read-parameter files (-r) are served by the host reader" in err
    err = run(tmp_path / "F", f["mode"], [f["bam"]], switch + "F", env=DEVICE, ok=False)
    assert "Filtered BAM output (-F) is written on the device BAM path only, which this configuration cannot take: read-parameter files (-r) are served by the host reader" in err
    err = run(tmp_path / "Pb", "name", [c["bam"]], switch + "b", chromosome_gene=1, env=DEVICE, ok=False)
    assert "Tagged BAM output (-b) is written on the device BAM path only, which this configuration cannot take: gene = chromosome name is resolved by the host reader" in err
    err = run(tmp_path / "PF", "name", [c["bam"]], switch + "F", chromosome_gene=1, env=DEVICE, ok=False)
    assert "Filtered BAM output (-F) is written on the device BAM path only, which this configuration cannot take: gene = chromosome name is resolved by the host reader" in err
