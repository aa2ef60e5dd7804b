"""What the filtered BAM output (-F) pass costs on the device BAM path, on the two files bench.py's BAM leg generates (scripts/bench_bam_tagged.py
writes them), against the -b ingest of the same files on the same box: tests/cpp/bam_tagged once per run for `ingest_ms` with -b, then
tests/cpp/bam_filtered (no barcode merge, min_genes_after_merge 10, the Simple UMI merge with its targets kept) for the wall time of
write_filtered_bam_files and its split into the decoder's kernels and copies, the tag kernels (rank, plan, scan, emit) and the compressor's
launches, all by device events.  --devices runs the same pass over a sharded container as well (tests/cpp/bam_filtered_sharded, in the same loop:
the one-context run beside it is its yardstick), once per "devices:quota" pair -- `--devices 0,0:0 0,0,0,0:1000000`; quota 0 = the container's own
rule, which puts the one boundary of two shards near the middle of the stream.  A sharded run's numbers carry `decisions_ms`, the one-off host
time of the shards' read corrections inside the pass (BamController::FilteredFile::decisions_ms).

Prints one JSON line.  python scripts/bench_bam_filtered.py [--reads 250000] [--copies 64] [--runs 2] [--devices 0,0:0 ...]"""
import argparse
import json
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=250_000)
    ap.add_argument("--copies", type=int, default=64)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--devices", nargs="*", default=[], help="device list:shard quota, e.g. 0,0:0")
    a = ap.parse_args()
    from bench_bam_tagged import run, write_files
    from dropest_amd.build import build_facade
    build_facade()
    tagged, filtered = os.path.join(ROOT, "tests", "cpp", "bam_tagged"), os.path.join(ROOT, "tests", "cpp", "bam_filtered")
    sharded = os.path.join(ROOT, "tests", "cpp", "bam_filtered_sharded")
    tmp = tempfile.mkdtemp()
    out = {}
    try:
        for label, bam, reads in write_files(tmp, a.reads, a.copies):
            r = {"reads": reads, "input_MB": round(os.path.getsize(bam) / 1e6, 1), "runs": []}
            for _ in range(a.runs):
                b = run([tagged, os.path.join(tmp, "out"), "filled", str(a.threads), bam], tmp)
                os.remove(os.path.join(tmp, b["files"][0]["name"]))
                f = run([filtered, "filled", "none", "0", "10", "simple", "1", bam], tmp)
                assert f["total_reads"] == reads
                os.remove(os.path.join(tmp, f["name"]))
                r["runs"].append({
                    "tagged_ingest_ms": round(b["ingest_ms"], 1), "tagged_tag_kernels_ms": round(b["files"][0]["tag_ms"], 1), "tagged_deflate_ms": round(b["files"][0]["deflate_ms"], 1),
                    "filtered_pass_ms": round(f["filtered_ms"], 1), "x_tagged_ingest": round(f["filtered_ms"] / b["ingest_ms"], 2),
                    "decode_ms": round(f["decode_ms"], 1), "tag_kernels_ms": round(f["tag_ms"], 1), "deflate_ms": round(f["deflate_ms"], 1),
                    "written": f["written"], "windows": f["windows"], "batches": f["batches"],
                    "inflated_MB_written": round(f["inflated_bytes"] / 1e6, 1), "compressed_MB_written": round(f["compressed_bytes"] / 1e6, 1),
                    "plain_ingest_ms": round(f["ingest_ms"], 1)})
                for pair in a.devices:
                    devices, quota = pair.split(":")
                    g = run([sharded, "filled", "none", "0", "10", "simple", "1", devices, quota, bam], tmp)
                    assert g["total_reads"] == reads and g["written"] == f["written"] and g["inflated_bytes"] == f["inflated_bytes"]
                    os.remove(os.path.join(tmp, g["name"]))
                    r["runs"][-1][pair] = {"filtered_pass_ms": round(g["filtered_ms"], 1), "x_one_context": round(g["filtered_ms"] / f["filtered_ms"], 2),
                                           "decode_ms": round(g["decode_ms"], 1), "tag_kernels_ms": round(g["tag_ms"], 1), "deflate_ms": round(g["deflate_ms"], 1),
                                           "decisions_ms": round(g["decisions_ms"], 1), "shards": g["shards"], "windows": g["windows"], "batches": g["batches"], "plain_ingest_ms": round(g["ingest_ms"], 1)}
            out[label] = r
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
