"""What tagged BAM output (-b) costs on the device BAM path, on the two files bench.py's BAM leg generates (one sequence and no qualities: deflates
~10.8 x; random bases and binned qualities: ~3.2 x, as a real 10x BAM).

1. (--parent-tool PATH: a bam_to_counts built from the parent commit)  ingest_ms of the UNCHANGED tool, parent against this tree, alternating,
   five runs each per file: both medians and the spread (max - min) of the parent's own runs.
2. tests/cpp/bam_tagged with -b against the same ingest without it (DROPEST_NO_TAGGED=1), three runs each per file: ingest_ms, the inflated and
   compressed bytes written, the output's size against the input's, the plan + scan + emit kernels and the compressor's launches by device
   events, and for the tag kernels bytes read + written over time as a share of the HBM peak (8 TB/s on an MI355X).

Prints one JSON line.  python scripts/bench_bam_tagged.py [--parent-tool PATH] [--reads 250000] [--copies 64]"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK_GB_PER_S = 8000.0


def write_files(tmp, n_reads, copies):
    """bench.py: measure_bam_ingest's synth.bam and synth_real.bam"""
    import bam_writer as bw
    from dropest_amd import capi
    from dropest_amd.synth import SynthStream
    s = SynthStream(n_reads=n_reads, n_cells=500, n_genes=5000, umi_len=10)
    cb, umi, gene, aux = s.generate_host()
    cbs = {int(c): capi.unpack_code(c) for c in np.unique(cb)}
    recs = []
    for i in range(n_reads):
        tags = [("CB", "Z", cbs[int(cb[i])]), ("UB", "Z", capi.unpack_code(umi[i]))]
        if gene[i] != capi.NO_GENE:
            tags.append(("GX", "Z", "ENSG%011d" % gene[i]))
        recs.append(bw.record(int(aux[i]) & 0xFFFF, i, "A00000:1:HXXXX:1:1101:%d:%d" % (i, i), seq="ACGT" * 24 + "AC", tags=tags))
    refs = [("chr%d" % i, 10_000_000) for i in range(25)]
    bam = os.path.join(tmp, "synth.bam")
    bw.write_bam(bam, refs, recs, repeat=copies)
    rng = np.random.default_rng(5)
    nib = rng.choice(np.array([1, 2, 4, 8], np.uint8), (n_reads, 98))
    packed_seq = ((nib[:, 0::2] << 4) | nib[:, 1::2]).astype(np.uint8)
    quals = rng.choice(np.array([37, 25, 11, 2], np.uint8), (n_reads, 98), p=[0.75, 0.12, 0.08, 0.05])
    recs_real = []
    for i, r in enumerate(recs):
        r = bytearray(r)
        o = 36 + r[12] + 4
        r[o:o + 49] = packed_seq[i].tobytes(); r[o + 49:o + 147] = quals[i].tobytes()
        recs_real.append(bytes(r))
    bam_real = os.path.join(tmp, "synth_real.bam")
    bw.write_bam(bam_real, refs, recs_real, repeat=max(1, copies // 2))
    return [("deflates_10x", bam, n_reads * copies), ("deflates_3x", bam_real, n_reads * max(1, copies // 2))]


def run(cmd, cwd, env=None):
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=cwd, env=dict(os.environ, **(env or {})), timeout=900)
    if res.returncode:
        raise RuntimeError("%s: %s" % (" ".join(cmd[:3]), res.stderr[-400:]))
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tool", default=None)
    ap.add_argument("--reads", type=int, default=250_000)
    ap.add_argument("--copies", type=int, default=64)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    if a.parent_tool:
        a.parent_tool = os.path.abspath(a.parent_tool)
    from dropest_amd.build import build_facade
    build_facade()
    counts, tagged = os.path.join(ROOT, "tests", "cpp", "bam_to_counts"), os.path.join(ROOT, "tests", "cpp", "bam_tagged")
    tmp = tempfile.mkdtemp()
    out = {}
    try:
        for label, bam, reads in write_files(tmp, a.reads, a.copies):
            r = {"reads": reads, "input_MB": round(os.path.getsize(bam) / 1e6, 1)}
            if a.parent_tool:
                ms = {"parent": [], "this": []}
                for _ in range(5):
                    for who, tool in (("parent", a.parent_tool), ("this", counts)):
                        st = run([tool, os.path.join(tmp, "out"), "filled", "20", "100", "-", str(a.threads), bam], tmp, {"DROPEST_BAM_DEVICE": "1"})
                        assert st["saved"] == reads
                        ms[who].append(st["ingest_ms"])
                r["unchanged_tool"] = {"parent_ingest_ms": ms["parent"], "this_ingest_ms": ms["this"], "parent_median_ms": round(statistics.median(ms["parent"]), 1),
                                       "this_median_ms": round(statistics.median(ms["this"]), 1), "parent_spread_ms": round(max(ms["parent"]) - min(ms["parent"]), 1)}
            with_b, without = [], []
            for _ in range(3):
                without.append(run([tagged, os.path.join(tmp, "out"), "filled", str(a.threads), bam], tmp, {"DROPEST_NO_TAGGED": "1"})["ingest_ms"])
                st = run([tagged, os.path.join(tmp, "out"), "filled", str(a.threads), bam], tmp)
                assert st["saved"] == reads == st["files"][0]["records"]
                with_b.append(st)
            best = min(with_b, key=lambda s: s["ingest_ms"])
            f = best["files"][0]
            r["tagged"] = {
                "ingest_ms_without_b": [round(x, 1) for x in without], "ingest_ms_with_b": [round(s["ingest_ms"], 1) for s in with_b],
                "x_ingest": round(statistics.median(s["ingest_ms"] for s in with_b) / statistics.median(without), 2),
                "inflated_MB_written": round(f["inflated_bytes"] / 1e6, 1), "compressed_MB_written": round(f["compressed_bytes"] / 1e6, 1),
                "output_over_input": round(f["compressed_bytes"] / os.path.getsize(bam), 2), "windows": f["windows"], "deflate_batches": f["batches"],
                "tag_kernels_ms": round(f["tag_ms"], 2), "deflate_kernels_ms": round(f["deflate_ms"], 1),
                "tag_GB_per_s_read_plus_written": round((f["tag_bytes_in"] + f["tag_bytes_out"]) / 1e6 / f["tag_ms"], 1),
                "tag_share_of_hbm_peak": round((f["tag_bytes_in"] + f["tag_bytes_out"]) / 1e6 / f["tag_ms"] / HBM_PEAK_GB_PER_S, 3),
                "deflate_GB_per_s_in": round(f["inflated_bytes"] / 1e6 / f["deflate_ms"], 1),
            }
            os.remove(os.path.join(tmp, f["name"]))
            out[label] = r
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
