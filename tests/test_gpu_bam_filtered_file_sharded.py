"""Filtered BAM output (-F) of a sharded or split container at file level, through tests/cpp/bam_filtered_sharded: BAM file(s) -> container on a
device list -> merge_and_filter -> BamController::write_filtered_bam_files with set_sharded_filtered_output on.  The one `<first stem>.filtered.bam`
is BGZF with the end-of-file block, inflates to the first input's header followed by tests/bam_filter_model.py's records over the SHARDED
container's dumped decisions, and to the very bytes the one-context tool (tests/cpp/bam_filtered) writes for the same files -- with shard quotas
that put a boundary behind the first read, inside a window, at a file boundary and one read behind it, and beyond the stream (every shard but
the first empty).  With the switch off the container is refused as before; -r files stay refused; a container that splits on its own goes
through the same code."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from dropest_amd.build import build_facade

import bam_writer as bw
from test_gpu_bam_filtered_file import (CELL_NOT_KEPT, HAND, K, M, NO_GENE, S, WRITTEN, check_output, hand_records, header_of, refused, run, two_files, varied,  # noqa: F401 (fixtures)
                                        varied_records, whitelist)
from test_gpu_bam_tagged_file import REFS, SMALL_WINDOWS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tests", "cpp", "bam_filtered_sharded")
DEVICE_LISTS = ["0,0", "0,0,0"]


def run_sharded(cwd, bams, devices, quota, merge="none", min_after=2, umi="simple", save=1, mode="filled", env=None, dump=True, expect_failure=False):
    """-> (the tool's JSON line, the dumped decisions [(verdict, cb, umi)]); with expect_failure the finished process"""
    build_facade()
    e = dict(os.environ, **(env or {}))
    dump_path = os.path.join(str(cwd), "decisions.txt")
    if dump:
        e["DROPEST_FILTER_DUMP"] = dump_path
    res = subprocess.run([TOOL, mode, merge, "0", str(min_after), umi, str(save), devices, str(quota)] + bams, capture_output=True, text=True, timeout=300, cwd=str(cwd), env=e)
    if expect_failure:
        return res
    assert res.returncode == 0, res.stdout + res.stderr
    decisions = []
    for line in open(dump_path):
        v, cb, u = line.split()
        decisions.append((int(v), b"" if cb == "-" else cb.encode(), b"" if u == "-" else u.encode()))
    return json.loads(res.stdout.strip().splitlines()[-1]), decisions


def inflated(cwd, stem):
    return gzip.decompress(open(os.path.join(str(cwd), stem + ".filtered.bam"), "rb").read())


def subdir(tmp_path, name):
    d = tmp_path / name
    d.mkdir()
    return d


# ---- (a) the hand-built file with the whitelist merge: M merges into K and S is not kept, and a quota of 1 or 7 puts a merged cell's reads and its
# target's on different shards ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    d = tmp_path_factory.mktemp("sharded_hand")
    recs = hand_records(HAND)
    path = str(d / "hand.bam")
    bw.write_bam(path, REFS, recs, block=700)
    wl = whitelist(d)
    stats, dec = run(d, [path], merge="real:" + wl, min_after=2)                   # one context: the bytes every sharded run must give
    return path, recs, wl, dec, inflated(d, "hand")


@pytest.mark.parametrize("quota", [1, 7, 1000])
@pytest.mark.parametrize("devices", DEVICE_LISTS)
def test_hand_built_file(tmp_path, hand, devices, quota):
    path, recs, wl, dec_one, bytes_one = hand
    stats, dec = run_sharded(tmp_path, [path], devices, quota, merge="real:" + wl, min_after=2)
    assert stats["shards"] == devices.count(",") + 1
    acc = [r for r in HAND if r[3] == 0]
    assert len(dec) == len(acc)
    for k, (cb, umi, gene, _) in enumerate(acc):                                 # the answers follow from how the file was made
        if gene is None:
            assert dec[k][0] == NO_GENE
        elif cb == S:
            assert dec[k][0] == CELL_NOT_KEPT
        elif cb in (K, M) and "N" not in umi:
            assert dec[k] == (WRITTEN, K.encode(), umi.encode())                 # M's reads under K's barcode, wherever K's cell lives
    assert dec == dec_one
    check_output(tmp_path, "hand", header_of(path), recs, stats, dec)
    assert inflated(tmp_path, "hand") == bytes_one


# ---- (b) 20 000 varied records in small windows, a shard boundary every 3 001 reads: several windows cross one ------------------------------------
@pytest.fixture(scope="module")
def varied_one(tmp_path_factory, varied):
    path, recs, header = varied
    d = tmp_path_factory.mktemp("sharded_varied_one")
    stats, dec = run(d, [path], min_after=10, env=SMALL_WINDOWS)
    return stats, dec, inflated(d, "varied")


@pytest.mark.parametrize("devices", DEVICE_LISTS)
def test_varied_file_with_boundaries_inside_windows(tmp_path, varied, varied_one, devices):
    path, recs, header = varied
    stats_one, dec_one, bytes_one = varied_one
    stats, dec = run_sharded(tmp_path, [path], devices, 3001, min_after=10, env=SMALL_WINDOWS)
    verdicts = [d[0] for d in dec]
    assert verdicts.count(WRITTEN) >= 2000 and verdicts.count(CELL_NOT_KEPT) >= 2000 and verdicts.count(NO_GENE) >= 1000      # else this proves nothing
    assert 24 <= len({d[1] for d in dec if d[0] == WRITTEN}) <= 60
    assert stats["windows"] >= 3 and stats["batches"] >= 3 and stats["shards"] == devices.count(",") + 1
    assert len(dec) > 3001 * (stats["shards"] - 1)                               # every shard holds reads, and a window of thousands crosses a boundary
    assert dec == dec_one
    check_output(tmp_path, "varied", header, recs, stats, dec)
    assert inflated(tmp_path, "varied") == bytes_one
    for key in ("name", "total_reads", "written", "wrong_genes", "wrong_umis", "inflated_bytes"):
        assert stats[key] == stats_one[key]


# ---- (c) two inputs: a shard boundary at the file boundary (the second file's decoder sits with the second shard) and one read behind it ----------
@pytest.fixture(scope="module")
def two_files_one(tmp_path_factory, two_files):
    a, b, recs_a, recs_b = two_files
    d = tmp_path_factory.mktemp("sharded_two_one")
    stats, dec = run(d, [a, b], min_after=2)
    return dec, inflated(d, "first")


@pytest.mark.parametrize("beyond", [0, 1])
@pytest.mark.parametrize("devices", DEVICE_LISTS)
def test_two_inputs_with_a_boundary_at_the_file_boundary(tmp_path, two_files, two_files_one, devices, beyond):
    a, b, recs_a, recs_b = two_files
    dec_one, bytes_one = two_files_one
    first_accepted = len(recs_a) - 1
    stats, dec = run_sharded(tmp_path, [a, b], devices, first_accepted + beyond, min_after=2)
    assert len(dec) == first_accepted + len(recs_b) and dec == dec_one
    check_output(tmp_path, "first", header_of(a), recs_a + recs_b, stats, dec)
    assert inflated(tmp_path, "first") == bytes_one
    assert sorted(f for f in os.listdir(str(tmp_path)) if f.endswith(".bam")) == ["first.filtered.bam"]


# ---- (d) what is refused ---------------------------------------------------------------------------------------------------------------------------
def test_the_switch_off_refuses_as_before(tmp_path, two_files):
    a, b, _, _ = two_files
    res = run_sharded(tmp_path, [a, b], "0,0", 0, min_after=2, dump=False, env={"DROPEST_FILTER_SWITCH_OFF": "1"}, expect_failure=True)
    refused(res, tmp_path, "Filtered BAM output (-F)", "shard")
    # ... in the words of the one-context tool on the same container
    old = run(subdir(tmp_path, "one"), [a, b], min_after=2, dump=False, env={"DROPEST_DEVICES": "0,0"}, expect_failure=True)
    errors = lambda r: [line for line in r.stderr.splitlines() if line.startswith("ERROR:")]
    assert old.returncode == 1 and len(errors(res)) == 1 and errors(old) == errors(res)


def test_read_parameter_files_are_refused(tmp_path):
    rows = [(K, "AAAACCCC", "G1"), (K, "GGGGTTTT", "G2"), (S, "ACACACAC", "G1")]
    recs = [bw.record(0, 10 + i, "p%d" % i, tags=[("GX", "Z", g)]) for i, (_, _, g) in enumerate(rows)]
    path, params = str(tmp_path / "r.bam"), str(tmp_path / "params.gz")
    bw.write_bam(path, REFS, recs)
    with gzip.open(params, "wt") as f:
        for i, (cb, umi, _) in enumerate(rows):
            f.write("p%d %s %s %s %s\n" % (i, cb, umi, "I" * len(cb), "I" * len(umi)))
    res = run_sharded(tmp_path, [path], "0,0", 2, mode="params:" + params, min_after=1, dump=False, expect_failure=True)
    refused(res, tmp_path, "Filtered BAM output (-F)", "read-parameter files (-r)")


# ---- (e) a container that splits on its own: one device, UMIs so long that cell id + gene + UMI pass the 64-bit sort key --------------------------
def split_records(n, umi_len, seed=5, n_big=40, n_small=300):
    """40 barcodes with most of the reads (kept under min_genes_after_merge = 10), 300 with the rest, 40 genes, UMIs of umi_len bases"""
    rng = np.random.default_rng(seed)
    genes = ["GENE%d" % i for i in range(40)]
    big = ["".join(rng.choice(list("ACGT"), 12)) for _ in range(n_big)]
    small = ["".join(rng.choice(list("ACGT"), 12)) for _ in range(n_small)]
    recs = []
    for i in range(n):
        cb = big[int(rng.integers(0, n_big))] if rng.random() < 0.7 else small[int(rng.integers(0, n_small))]
        umi = "".join(rng.choice(list("ACGT"), umi_len))
        g = None if i % 9 == 0 else genes[int(rng.integers(0, len(genes)))]
        tags = [("CB", "Z", cb), ("UB", "Z", umi)] + ([("GX", "Z", g)] if g else [])
        recs.append(bw.record(i % 4, i, "s%d" % i, flag=4 if i % 50 == 1 else 0, tags=tags))
    return recs


def test_a_container_that_splits_on_its_own(tmp_path):
    """25-base UMIs (51 bits) + 6 bits of gene + 9 bits of cell id do not fit one context's key: the facade splits the stream over shards of the one
    device (settled on an MI355X: four of them), whose read corrections key (column of some 40, gene, UMI) in 64 bits -- so -F goes through the shards' code"""
    recs = split_records(6000, 25)
    path = str(tmp_path / "split.bam")
    bw.write_bam(path, REFS, recs, block=2_000)                                  # ~390 blocks: half a dozen windows of 64
    stats, dec = run_sharded(tmp_path, [path], "0", 0, min_after=10, env=SMALL_WINDOWS)
    assert stats["shards"] > 1 and stats["windows"] >= 3
    verdicts = [d[0] for d in dec]
    assert verdicts.count(WRITTEN) >= 3000 and verdicts.count(CELL_NOT_KEPT) >= 1000 and verdicts.count(NO_GENE) >= 500
    # (the 40 barcodes with ~100 reads each are kept; one with ~6 reads reaches ten genes now and then)
    assert 40 <= len({d[1] for d in dec if d[0] == WRITTEN}) <= 80 and all(len(d[2]) == 25 for d in dec if d[0] == WRITTEN)
    check_output(tmp_path, "split", header_of(path), recs, stats, dec)


def test_a_split_whose_read_corrections_are_refused(tmp_path):
    """One base more: the container still splits and merges, but the shards' read corrections cannot key (column, gene, UMI) in 64 bits -- so not
    every stream that splits gets its file.  The shards' refusal reaches the caller in their words and no file is left behind."""
    recs = split_records(6000, 26)
    path = str(tmp_path / "split.bam")
    bw.write_bam(path, REFS, recs, block=12_345)
    res = run_sharded(tmp_path, [path], "0", 0, min_after=10, dump=False, expect_failure=True)
    refused(res, tmp_path, "Filtered BAM output (-F)", "shard 0: read corrections", "wider than 64 bits")
    assert json.loads(res.stdout.strip().splitlines()[-1])["shards"] > 1
