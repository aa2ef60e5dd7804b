"""Writes tests/golden/libdeflate_bgzf.gz: BGZF blocks whose DEFLATE payloads libdeflate made (levels 1, 6, 9, 12 over the GPU suite's kinds()
data and BAM-like records), for tests/test_deflate_writer_cpu.py and tests/test_gpu_inflate_edges.py.  libdeflate is loaded through ctypes
from a shared library already on the machine (--lib, default: the one ctypes.util finds); nothing is fetched.  The file checks itself: its
expected bytes are gzip.decompress(file).

    python scripts/make_libdeflate_fixture.py [--lib PATH] [--version TEXT]"""
import argparse
import glob
import os
import struct
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import deflate_writer as dw      # noqa: E402


def guess_version(path):
    """libdeflate has no version call: the package record next to the library, if any"""
    real = os.path.realpath(path)
    for meta in glob.glob(os.path.join(os.path.dirname(os.path.dirname(real)), "conda-meta", "libdeflate-*.json")):
        return os.path.basename(meta)[len("libdeflate-"):].rsplit("-", 1)[0]
    status = "/var/lib/dpkg/status"
    if os.path.exists(status):
        block = [b for b in open(status, errors="replace").read().split("\n\n") if b.startswith("Package: libdeflate0")]
        for line in block[0].splitlines() if block else []:
            if line.startswith("Version:"):
                return line.split()[1]
    return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--version", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "libdeflate_bgzf.gz"))
    a = ap.parse_args()
    ld = dw.libdeflate(a.lib)
    if ld is None:
        sys.exit("no libdeflate shared library found (give --lib)")
    version = a.version or guess_version(ld.path)
    blocks = []
    for level, data in dw.libdeflate_samples(np.random.default_rng(2024), size=12_000):
        payload = ld.compress(data, level)
        blocks.append(dw.bgzf(payload, len(data), zlib.crc32(data) & 0xFFFFFFFF))
    blocks.append(dw.bgzf(b"\x03\x00", 0, 0))                                  # the BGZF end-of-file block
    blob = b"".join(blocks)
    assert len(blob) <= 256 << 10, len(blob)
    open(a.out, "wb").write(blob)
    print("libdeflate %s (%s): %d blocks, %d bytes -> %s" % (version, ld.path, len(blocks), len(blob), a.out))
    assert struct.unpack_from("<H", blob, 16)[0] + 1 == len(blocks[0])


if __name__ == "__main__":
    main()
