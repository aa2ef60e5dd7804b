"""Developer tool: what tagged and filtered BAM output (-b, -F) cost under -r read-parameter files on the device BAM path
(BamController::set_device_source_output), on bench_bam_params.py's file of reads with unique names, in one job:
  1. tests/cpp/bam_sources_output: the plain -r ingest, -b under -r and -F under -r, alternating: wall time, the tag kernels and the compressor's
     launches by device events, the read corrections;
  2. the replay alone (dropest_read_params_replay_begin + _end on a table of that many rows);
  3. with --parent-tools DIR (the tests/cpp of a build of the parent commit): bam_tagged and bam_filtered of the parent against this build's on the
     two files of bench.py's BAM leg, alternating -- the paths that did not change.
usage: bench_bam_params_output.py [n_reads] [--runs K] [--threads T] [--parent-tools DIR] [--reads R --copies C]   -> one JSON line per measurement"""
import argparse
import ctypes as C
import gzip
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np                                   # noqa: E402
import bam_writer as bw                              # noqa: E402
from dropest_amd import capi                         # noqa: E402
from dropest_amd.build import FILTERED_TOOL, SOURCES_OUTPUT_TOOL, TAGGED_TOOL, build_facade   # noqa: E402
from dropest_amd.synth import SynthStream            # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("n_reads", nargs="?", type=float, default=1e6)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--parent-tools", default=None)
ap.add_argument("--reads", type=int, default=250_000)
ap.add_argument("--copies", type=int, default=64)
args = ap.parse_args()
n = int(args.n_reads)
build_facade()
tmp = tempfile.mkdtemp()


def spread(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


def tool(cmd, env=None):
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp, env=dict(os.environ, **(env or {})), timeout=900)
    if res.returncode:
        raise SystemExit("%s: %s" % (" ".join(cmd[:3]), res.stderr[-600:]))
    return json.loads(res.stdout.strip().splitlines()[-1])


try:
    s = SynthStream(n_reads=n, n_cells=500, n_genes=5000, umi_len=10)
    cb, umi, gene, aux = s.generate_host()
    refs = [("chr%d" % i, 10_000_000) for i in range(25)]
    cb_of = {int(c): capi.unpack_code(c) for c in np.unique(cb)}
    recs, rows = [], []
    for i in range(n):
        c, u = cb_of[int(cb[i])], capi.unpack_code(umi[i])
        tags = [("GX", "Z", "ENSG%011d" % gene[i])] if gene[i] != capi.NO_GENE else []
        name = "A00000:1:HXXXX:1:1101:%d:%d" % (i, i)
        recs.append(bw.record(int(aux[i]) & 0xFFFF, i, name, seq="ACGT" * 24 + "AC", tags=tags))
        rows.append("@%s %s %s %s %s" % (name, c, u, "F" * len(c), "F" * len(u)))
    bam, params = os.path.join(tmp, "r.bam"), os.path.join(tmp, "p.gz")
    bw.write_bam(bam, refs, recs)
    text = ("\n".join(rows) + "\n").encode()
    with gzip.open(params, "wb", compresslevel=1) as f:
        f.write(text)
    shape = dict(reads=n, threads=args.threads, runs=args.runs, bam_mb=round(os.path.getsize(bam) / 1e6, 1), params_text_mb=round(len(text) / 1e6, 1))
    # 1. plain ingest, -b and -F under -r, alternating
    DEV = {"DROPEST_BAM_DEVICE": "1"}
    got = {"plain": [], "b": [], "F": []}
    for _ in range(args.runs):
        for which, sources in (("plain", "1"), ("b", "1b"), ("F", "1F")):
            got[which].append(tool([SOURCES_OUTPUT_TOOL, os.path.join(tmp, "out"), "params:" + params, "0", sources, "1", "20", "100", "-", str(args.threads), "-", "0", bam], DEV))
    tb, fl = [g["tagged"][0] for g in got["b"]], [g["filtered"] for g in got["F"]]
    assert all(t["records"] == g["saved"] for t, g in zip(tb, got["b"])) and all(f["total_reads"] == g["saved"] for f, g in zip(fl, got["F"]))
    print(json.dumps(dict(shape, what="-b and -F under -r", saved=got["plain"][0]["saved"], written_by_F=fl[0]["written"],
                          plain_ingest_ms=spread([g["ingest_ms"] for g in got["plain"]]), b_ingest_ms=spread([g["ingest_ms"] for g in got["b"]]),
                          b_tag_kernels_ms=spread([t["tag_ms"] for t in tb]), b_compressor_ms=spread([t["deflate_ms"] for t in tb]), b_inflated_mb=round(tb[0]["inflated_bytes"] / 1e6, 1),
                          F_pass_ms=spread([f["filtered_ms"] for f in fl]), F_tag_kernels_ms=spread([f["tag_ms"] for f in fl]), F_compressor_ms=spread([f["deflate_ms"] for f in fl]),
                          F_decode_ms=spread([f["decode_ms"] for f in fl]), F_read_corrections_ms=spread([f["decisions_ms"] for f in fl]))), flush=True)
    # 2. the replay alone: a fresh claim array put in place and the old one put back
    L = capi.lib()
    L.dropest_bgzf_last_error.restype = C.c_char_p
    L.dropest_read_params_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.dropest_read_params_add_text.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int]
    for name in ("build", "replay_begin", "replay_end"):
        getattr(L, "dropest_read_params_" + name).argtypes = [C.c_void_p]
    L.dropest_read_params_destroy.argtypes = [C.c_void_p]
    L.dropest_read_params_destroy.restype = None
    buf = np.frombuffer(text, np.uint8)
    starts = np.concatenate(([0], np.flatnonzero(buf == 10)[:-1] + 1)).astype(np.uint64)
    h = C.c_void_p()
    if L.dropest_read_params_create(0, 0, C.byref(h)) or L.dropest_read_params_add_text(h, buf.ctypes.data, len(buf), starts.ctypes.data, len(starts), 0) or L.dropest_read_params_build(h):
        raise SystemExit(L.dropest_bgzf_last_error())
    replay_ms = []
    for _ in range(args.runs + 1):
        t1 = time.perf_counter()
        if L.dropest_read_params_replay_begin(h) or L.dropest_read_params_replay_end(h):
            raise SystemExit(L.dropest_bgzf_last_error())
        replay_ms.append((time.perf_counter() - t1) * 1e3)
    L.dropest_read_params_destroy(h)
    print(json.dumps(dict(shape, what="replay begin + end", first_ms=round(replay_ms[0], 3), later_ms=spread(replay_ms[1:]))), flush=True)
    # 3. the paths that did not change: the parent's bam_tagged and bam_filtered against this build's
    if args.parent_tools:
        from bench_bam_tagged import write_files
        parent = os.path.abspath(args.parent_tools)
        for label, path, reads in write_files(tmp, args.reads, args.copies):
            ms = {"tagged": {"parent": [], "this": []}, "filtered": {"parent": [], "this": []}}
            for _ in range(args.runs):
                for who, tagged, filtered in (("parent", os.path.join(parent, "bam_tagged"), os.path.join(parent, "bam_filtered")), ("this", TAGGED_TOOL, FILTERED_TOOL)):
                    ms["tagged"][who].append(tool([tagged, os.path.join(tmp, "out"), "filled", str(args.threads), path])["ingest_ms"])
                    ms["filtered"][who].append(tool([filtered, "filled", "none", "0", "10", "simple", "1", path])["filtered_ms"])
            for which, v in ms.items():
                print(json.dumps(dict(what="unchanged bam_" + which, file=label, reads=reads, parent_ms=spread(v["parent"]), this_ms=spread(v["this"]),
                                      parent_spread_ms=round(max(v["parent"]) - min(v["parent"]), 1))), flush=True)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
