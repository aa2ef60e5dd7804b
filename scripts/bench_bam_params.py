"""Developer tool: -r (read-parameter files) and -P (gene = chromosome name) on the device BAM path against the host reader, in one job:
  1. the read-parameter table alone (dropest_read_params_*): build time and rows per second;
  2. tests/cpp/bam_sources on a BAM with its parameter file: device ingest (the switch on, DROPEST_BAM_DEVICE=1) against the host reader;
  3. the same for -P on a read-name file;
  4. with --parent-tool: tests/cpp/bam_to_counts of a build of the parent commit against this build's on the read-name file, alternating -- the
     path that did not change.
usage: bench_bam_params.py [n_reads] [--runs K] [--threads T] [--parent-tool PATH/bam_to_counts]   -> one JSON line per measurement"""
import argparse
import ctypes as C
import gzip
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                   # noqa: E402
import bam_writer as bw                              # noqa: E402
from dropest_amd import capi                         # noqa: E402
from dropest_amd.build import BAM_TOOL, SOURCES_TOOL, build_facade   # noqa: E402
from dropest_amd.synth import SynthStream            # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("n_reads", nargs="?", type=float, default=1e6)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--parent-tool", default=None)
args = ap.parse_args()
n = int(args.n_reads)
build_facade()
tmp = tempfile.mkdtemp()
t0 = time.time()
s = SynthStream(n_reads=n, n_cells=500, n_genes=5000, umi_len=10)
cb, umi, gene, aux = s.generate_host()
refs = [("chr%d" % i, 10_000_000) for i in range(25)]
cb_of = {int(c): capi.unpack_code(c) for c in np.unique(cb)}
recs_r, recs_n, rows = [], [], []
for i in range(n):
    c, u = cb_of[int(cb[i])], capi.unpack_code(umi[i])
    tags = [("GX", "Z", "ENSG%011d" % gene[i])] if gene[i] != capi.NO_GENE else []
    name = "A00000:1:HXXXX:1:1101:%d:%d" % (i, i)
    recs_r.append(bw.record(int(aux[i]) & 0xFFFF, i, name, seq="ACGT" * 24 + "AC", tags=tags))
    recs_n.append(bw.record(int(aux[i]) & 0xFFFF, i, "%s!%s#%s" % (name, c, u), seq="ACGT" * 24 + "AC", tags=tags))
    rows.append("@%s %s %s %s %s" % (name, c, u, "F" * len(c), "F" * len(u)))
bam_r, bam_n, params = os.path.join(tmp, "r.bam"), os.path.join(tmp, "n.bam"), os.path.join(tmp, "p.gz")
bw.write_bam(bam_r, refs, recs_r); bw.write_bam(bam_n, refs, recs_n)
text = ("\n".join(rows) + "\n").encode()
with gzip.open(params, "wb", compresslevel=1) as f:
    f.write(text)
print("wrote %d reads: %.1f + %.1f MB of BAM, %.1f MB of parameter text, %.1f s" % (n, os.path.getsize(bam_r) / 1e6, os.path.getsize(bam_n) / 1e6, len(text) / 1e6, time.time() - t0), file=sys.stderr)
shape = dict(reads=n, threads=args.threads, runs=args.runs, bam_mb=round(os.path.getsize(bam_r) / 1e6, 1), params_text_mb=round(len(text) / 1e6, 1))


def spread(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3))


# 1. the table alone: the text and its line starts to the device, rows, insert, canonical rows
L = capi.lib()
L.dropest_bgzf_last_error.restype = C.c_char_p
L.dropest_read_params_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
L.dropest_read_params_add_text.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int]
L.dropest_read_params_build.argtypes = [C.c_void_p]
L.dropest_read_params_destroy.argtypes = [C.c_void_p]
L.dropest_read_params_destroy.restype = None
buf = np.frombuffer(text, np.uint8)
t_lines = time.perf_counter()
starts = np.concatenate(([0], np.flatnonzero(buf == 10)[:-1] + 1)).astype(np.uint64)
lines_ms = (time.perf_counter() - t_lines) * 1e3
build_ms = []
for _ in range(args.runs + 1):
    h = C.c_void_p()
    t1 = time.perf_counter()
    if L.dropest_read_params_create(0, 0, C.byref(h)) or L.dropest_read_params_add_text(h, buf.ctypes.data, len(buf), starts.ctypes.data, len(starts), 0) or L.dropest_read_params_build(h):
        raise SystemExit(L.dropest_bgzf_last_error())
    build_ms.append((time.perf_counter() - t1) * 1e3)
    L.dropest_read_params_destroy(h)
build_ms = build_ms[1:]      # (the first one loads the kernels)
print(json.dumps(dict(shape, what="table build (add_text + build)", ms=spread(build_ms), mrows_per_s=round(n / statistics.median(build_ms) / 1e3, 2), line_starts_numpy_ms=round(lines_ms, 1))), flush=True)


def ingest(tool, argv, env):
    res = subprocess.run([tool] + argv, capture_output=True, text=True, env=dict(os.environ, **env))
    if res.returncode:
        raise SystemExit(res.stderr)
    st = json.loads(res.stdout.strip().splitlines()[-1])
    if env.get("DROPEST_BAM_DEVICE") and "(taken: 1)" not in res.stderr:
        raise SystemExit("the device path did not take the file:\n" + res.stderr)
    return st


out = os.path.join(tmp, "out")
DEV = {"DROPEST_BAM_DEVICE": "1", "DROPEST_BAM_TRACE": "1"}
# 2. and 3. device ingest against the host reader, alternating
for what, mode, bam, chromosome_gene in (("-r", "params:" + params, bam_r, "0"), ("-P", "name", bam_n, "1")):
    argv = [out, mode, chromosome_gene, "1", "20", "100", "-", str(args.threads), "-", "0", bam]
    got = {"device": [], "host": [], "device_load": [], "host_load": []}
    for _ in range(args.runs):
        for path, env in (("device", DEV), ("host", {})):
            st = ingest(SOURCES_TOOL, argv, env)
            got[path].append(st["ingest_ms"]); got[path + "_load"].append(st["load_params_ms"])
    print(json.dumps(dict(shape, what="ingest under " + what, device_ms=spread(got["device"]), host_reader_ms=spread(got["host"]),
                          inflate_parameter_files_ms=spread(got["device_load"] + got["host_load"]),
                          device_mreads_per_s=round(n / statistics.median(got["device"]) / 1e3, 2), host_mreads_per_s=round(n / statistics.median(got["host"]) / 1e3, 2))), flush=True)
# 4. the path that did not change: read-name mode through bam_to_counts, the parent's build against this one
if args.parent_tool:
    argv = [out, "name", "20", "100", "-", str(args.threads), bam_n]
    got = {"parent": [], "this": []}
    for _ in range(args.runs):
        for which, tool in (("parent", args.parent_tool), ("this", BAM_TOOL)):
            got[which].append(ingest(tool, argv, DEV)["ingest_ms"])
    print(json.dumps(dict(shape, what="unchanged name-mode device ingest", parent_ms=spread(got["parent"]), this_ms=spread(got["this"]))), flush=True)
import shutil; shutil.rmtree(tmp, ignore_errors=True)      # noqa: E702
