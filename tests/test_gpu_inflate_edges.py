"""The BGZF inflate kernels (csrc/k_inflate_par.h, the default; csrc/k_inflate.h, DROPEST_INFLATE_PAR=0) on the DEFLATE corpus of
tests/deflate_writer.py: streams zlib's encoder never writes -- 15-bit codes, every code length, degenerate codes, every code-length repeat
form, hundreds of blocks per BGZF block, ISIZE = 65 536, the 48-bit match and the end-of-block symbol across the parallel kernel's chunk and
span boundaries at every offset, matches that make its window slide -- and malformed streams.  Checked at the level of
dropest_bgzf_inflate_buffer, with and without the CRC-32 check: in the BAM path a block the kernel gets wrong is inflated again on the host,
so only here does a kernel error show as an error.

A valid block: status 0 and the encoder's bytes.  A malformed block: a nonzero status, and its neighbours in the same launch whole and in
place.  An INCOMPLETE code whose unused patterns the stream never reaches: decoded, like the host decoder does (the policy of
tests/test_deflate_writer_cpu.py).  Also: libdeflate's own streams (the committed fixture, and fresh ones when the library is on the
machine), and a BAM file written in libdeflate's forms through the device decoder with no block handed back to the host."""
import ctypes as C
import gzip
import os
import struct
import subprocess
import sys
import tempfile
import zlib

import numpy as np
import pytest

import deflate_writer as dw
import test_gpu_bgzf as tg

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
OUT_BUDGET = 3 << 20          # inflated bytes per call (test_gpu_bgzf.inflate's output buffer holds 4 MB at least)


def batches(cases):
    """the cases that fit a BGZF block, malformed ones between valid ones, cut into calls of at most OUT_BUDGET inflated bytes"""
    good = [c for c in cases if c.fits_bgzf and c.verdict != dw.MALFORMED]
    bad = [c for c in cases if c.fits_bgzf and c.verdict == dw.MALFORMED]
    order = []
    for k, c in enumerate(good):
        order.append(c)
        if k < len(bad):
            order.append(bad[k])
    order += bad[len(good):]
    out, cur, size = [], [], 0
    for c in order:
        n = len(c.data) if c.data is not None else c.out_size
        if cur and size + n > OUT_BUDGET:
            out.append(cur); cur, size = [], 0
        cur.append(c); size += n
    return out + [cur] if cur else out


def check_cases(cases, repeats):
    """every batch through one dropest_bgzf_inflate_buffer call -> a list of failures (case name, what)"""
    fails = []
    for batch in batches(cases):
        blocks = [c.block() for c in batch]
        isizes = [struct.unpack_from("<I", b, len(b) - 4)[0] for b in blocks]
        out, status, _ = tg.inflate(b"".join(blocks), repeats)
        assert len(status) == len(batch)
        off = np.concatenate([[0], np.cumsum(isizes)])
        for k, c in enumerate(batch):
            if c.refused_by_device:
                if status[k] == 0:
                    fails.append((c.name, "taken"))
            elif status[k] != 0:
                fails.append((c.name, "status %d" % status[k]))
            elif out[off[k]:off[k + 1]] != c.data:
                fails.append((c.name, "bytes differ"))
    return fails


def check_all(repeats):
    """the corpus, the libdeflate fixture and a wrong CRC-32 under a valid payload"""
    fails = check_cases(dw.corpus(), repeats)
    blob = open(os.path.join(HERE, "golden", "libdeflate_bgzf.gz"), "rb").read()
    out, status, _ = tg.inflate(blob, repeats)
    if status.any() or out != gzip.decompress(blob):
        fails.append(("libdeflate fixture", np.flatnonzero(status).tolist()))
    good = [c for c in dw.corpus() if c.name == "all_286_and_30_symbols"][0]
    wrong = dw.Case("crc", good.payload, good.data, bad_crc=(zlib.crc32(good.data) ^ 1) & 0xFFFFFFFF)
    out, status, _ = tg.inflate(good.block() + wrong.block() + good.block(), repeats)
    want = [0, 10, 0] if repeats >= 0 else [0, 0, 0]
    if list(status) != want or out[:len(good.data)] != good.data or out[-len(good.data):] != good.data:
        fails.append(("wrong crc", list(status)))
    return fails


def test_parallel_kernel_with_crc():
    fails = check_all(1)
    assert not fails, fails


def test_parallel_kernel_without_crc():
    fails = check_all(-1)
    assert not fails, fails


_SERIAL_CHILD = r"""
import sys
sys.path.insert(0, %(here)r); sys.path.insert(0, %(root)r)
import test_gpu_inflate_edges as t
fails = t.check_all(1) + [("no crc",) + f for f in t.check_all(-1)]
print("serial kernel fails:", fails)
"""


def test_serial_kernel_with_and_without_crc():
    """csrc/k_inflate.h (read once per process: a fresh one)"""
    r = subprocess.run([sys.executable, "-c", _SERIAL_CHILD % dict(here=HERE, root=os.path.dirname(HERE))], capture_output=True, text=True, timeout=400,
                       env=dict(os.environ, DROPEST_INFLATE_PAR="0"))
    assert r.returncode == 0 and "serial kernel fails: []" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_fresh_libdeflate_streams():
    ld = dw.libdeflate()
    if ld is None:
        pytest.skip("no libdeflate shared library on this machine: the fresh-stream leg needs one (the committed fixture is checked anyway)")
    blocks, want = [], []
    for level, data in dw.libdeflate_samples(np.random.default_rng(43)):
        payload = ld.compress(data, level)
        if len(payload) + 26 > 65_536:
            continue
        blocks.append(dw.bgzf(payload, len(data), zlib.crc32(data) & 0xFFFFFFFF)); want.append(data)
    assert len(blocks) > 30
    for repeats in (1, -1):
        out, status, _ = tg.inflate(b"".join(blocks), repeats)
        assert not status.any(), np.flatnonzero(status)
        assert out == b"".join(want)


def test_bam_in_libdeflate_forms_through_the_device_decoder():
    """a fuzzed file in 65 536-byte blocks of many dynamic DEFLATE blocks each (single distance codes, literal-only pieces, code-length runs
    across the boundary): the device decoder against the record model with no block refused (check_against_model: refused == 0 -- a block
    the kernel got wrong would be inflated on the host and the leg would prove nothing), and every block through the host decoder"""
    import test_gpu_bam_decoder_model as tm
    from dropest_amd.build import FACADE_LIB
    recs = tm.fuzz_records(808, 3000, big=False)
    with tempfile.TemporaryDirectory() as d:
        f = tm.BamFile(os.path.join(d, "l.bam"), recs, 65_536, compress=dw.libdeflate_like(5))
    isizes = [b[3] - b[2] for b in f.blocks]
    assert isizes.count(65_536) >= 5, isizes
    L = tm.lib()
    cfg = tm.CASES[0][1]
    dicts, pairs, names = tm.dictionaries("half")
    for per in ([1, 200_000], [1 << 40]):
        dec = tm.make_decoder(L, cfg, dicts, pairs, names)
        try:
            res = tm.run_file(L, dec, f, per, "window")
            assert all(r[0]["refused"] == 0 for r in res)
            tm.check_against_model(f, res, cfg, dicts)
        finally:
            L.dropest_bam_decoder_destroy(dec)
    H = C.CDLL(FACADE_LIB)
    H.dropest_test_fast_inflate.restype = C.c_int
    H.dropest_test_fast_inflate.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64]
    raw = gzip.decompress(f.blob)
    for c0, c1, u0, u1 in f.blocks:
        out = np.zeros(u1 - u0 + 1, np.uint8)
        assert H.dropest_test_fast_inflate(f.blob[c0 + 18:c1 - 8], c1 - c0 - 26, out.ctypes.data, u1 - u0) == 1
        assert out[:u1 - u0].tobytes() == raw[u0:u1]
