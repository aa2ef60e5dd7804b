"""The device BGZF compressor (include/dropest_deflate.h) on the three payload kinds of an .rds body, 256 MB each by default: big-endian int32 row
indices, big-endian doubles of small counts, random bytes.  Per kind: kernel GB/s of input by HIP events (mean of `--repeats` runs after a
warm-up call), output / input, and zlib level 4 on a 16 MB sample of the same bytes cut into the same 65 280-byte chunks and into 2 MB
members (what the host writer does).  One JSON line per kind.   python scripts/bench_deflate.py [--mb 256] [--repeats 3]"""
import argparse
import ctypes as C
import json
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dropest_amd import capi


def payloads(n_bytes):
    rng = np.random.default_rng(1)
    cols = np.sort(rng.integers(0, 30_000, (n_bytes // 4 // 2000, 2000)), axis=1)            # ascending row indices inside each column
    yield "int32_row_indices", cols.astype(">i4").tobytes()
    yield "doubles_small_counts", np.minimum(rng.geometric(0.6, n_bytes // 8), 200).astype(">f8").tobytes()
    yield "random", rng.integers(0, 256, n_bytes, dtype=np.uint8).tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    L = capi.lib()
    P = C.POINTER
    L.dropest_bgzf_deflate_buffer.restype = C.c_int
    L.dropest_bgzf_deflate_buffer.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, P(C.c_uint64), P(C.c_uint64), P(C.c_double), C.c_int, C.c_int]
    L.dropest_bgzf_deflate_bound.restype = C.c_uint64
    L.dropest_bgzf_deflate_bound.argtypes = [C.c_uint64]
    L.dropest_deflate_last_error.restype = C.c_char_p
    for name, data in payloads(a.mb << 20):
        src = np.frombuffer(data, np.uint8)
        out = np.zeros(L.dropest_bgzf_deflate_bound(len(data)), np.uint8)
        n_out, n_mem, ms = C.c_uint64(), C.c_uint64(), C.c_double()
        for reps in (1, a.repeats):
            if L.dropest_bgzf_deflate_buffer(0, src.ctypes.data, len(data), out.ctypes.data, len(out), C.byref(n_out), C.byref(n_mem), C.byref(ms), reps, 0):
                raise SystemExit(L.dropest_deflate_last_error().decode())
        sample = data[:16 << 20]
        z_chunks = sum(len(zlib.compress(sample[o:o + 65_280], 4)) + 12 for o in range(0, len(sample), 65_280))
        z_pieces = sum(len(zlib.compress(sample[o:o + (2 << 20)], 4)) + 12 for o in range(0, len(sample), 2 << 20))
        print(json.dumps({"payload": name, "input_MB": len(data) / 1e6, "kernel_ms": round(ms.value, 3), "kernel_GBps": round(len(data) / ms.value / 1e6, 2),
                          "members": n_mem.value, "out_over_in": round(n_out.value / len(data), 4),
                          "zlib4_65280_over_in": round(z_chunks / len(sample), 4), "zlib4_2MB_over_in": round(z_pieces / len(sample), 4)}), flush=True)


if __name__ == "__main__":
    main()
