"""BGZF blocks written on the device (include/dropest_deflate.h, csrc/k_deflate.h) through dropest_bgzf_deflate_buffer.

Every member of every case: zlib takes it as a gzip member and gives the chunk back; BSIZE, ISIZE and the CRC-32 are what Python computes; the
whole stream goes back through dropest_bgzf_inflate_buffer with the CRC check on -- through the parallel inflate kernel here and through the
serial one in a fresh process (DROPEST_INFLATE_PAR=0 is read once per process) -- with every status 0; a second call gives the same bytes.
The cases are the encoder's edges: lengths around the minimum and maximum match and around the chunk size, runs, periods, the distance limit,
a chunk that ends inside a run, Huffman trees deeper than 15, one and no distance code, data that does not compress.  Sizes are stated, not
measured: a run of zeros is full-length matches (under 1 %), and the doubles an .rds file is made of come out smaller than zlib's level 4
does under fixed codes on the same chunks, which needs both the matches and the dynamic codes to work."""
import ctypes as C
import functools
import gzip
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from dropest_amd import capi

import test_gpu_bgzf as tg

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CHUNK = 65_280
P = C.POINTER


def lib():
    L = capi.lib()
    L.dropest_bgzf_deflate_buffer.restype = C.c_int
    L.dropest_bgzf_deflate_buffer.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, P(C.c_uint64), P(C.c_uint64), P(C.c_double), C.c_int, C.c_int]
    L.dropest_bgzf_deflate_bound.restype = C.c_uint64
    L.dropest_bgzf_deflate_bound.argtypes = [C.c_uint64]
    L.dropest_deflate_last_error.restype = C.c_char_p
    return L


def deflate(data, flags=0, out_cap=None, canary=16):
    """-> (rc, stream bytes or None, members, bytes needed, the whole output array)"""
    L = lib()
    src = np.frombuffer(data, np.uint8) if len(data) else np.zeros(1, np.uint8)
    cap = L.dropest_bgzf_deflate_bound(len(data)) if out_cap is None else out_cap
    out = np.full(cap + canary, 0x5A, np.uint8)
    n_out, n_mem, ms = C.c_uint64(), C.c_uint64(), C.c_double()
    rc = L.dropest_bgzf_deflate_buffer(0, src.ctypes.data, len(data), out.ctypes.data, cap, C.byref(n_out), C.byref(n_mem), C.byref(ms), 1, flags)
    assert (out[cap:] == 0x5A).all()
    return rc, (out[:n_out.value].tobytes() if rc == 0 else None), n_mem.value, n_out.value, out


def members_of(stream):
    out, at = [], 0
    while at < len(stream):
        assert stream[at:at + 4] == b"\x1f\x8b\x08\x04" and stream[at + 10:at + 16] == b"\x06\x00BC\x02\x00", at
        bsize = struct.unpack_from("<H", stream, at + 16)[0] + 1
        assert at + bsize <= len(stream)
        out.append(stream[at:at + bsize])
        at += bsize
    return out


def de_bruijn(k, n):
    """every n-gram over k symbols exactly once (cyclic): no match of length n anywhere in one period"""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return bytes(seq)


def fibonacci_counts(n_values, total=None):
    """value k appears fib(k) times; with `total`, the values the budget has no Fibonacci number for share what is left"""
    fib = [1, 1]
    while len(fib) < n_values:
        fib.append(fib[-1] + fib[-2])
    if total is None:
        return fib
    keep = 0
    while keep < n_values and sum(fib[:keep + 1]) + (n_values - keep - 1) <= total:
        keep += 1
    rest = total - sum(fib[:keep])
    tail = n_values - keep
    return fib[:keep] + [rest // tail + (1 if j < rest % tail else 0) for j in range(tail)]


def mixed(n, seed):
    """records with a shared shape: matches, literals and a skewed alphabet at once"""
    rng = np.random.default_rng(seed)
    recs = []
    while sum(map(len, recs)) < n:
        recs.append(b"read%d\tGENE%04d\t%s\n" % (len(recs), int(rng.integers(0, 40)), bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 12))))
    return b"".join(recs)[:n]


def doubles_payload():
    return np.minimum(np.random.default_rng(20261018).geometric(0.6, 1_000_000), 200).astype(">f8").tobytes()


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(7)
    rnd = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    c = {}
    for n in (0, 1, 2, 3, 257, 258, 259, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1):
        c["len_%d" % n] = mixed(n, n)
    c["zeros"] = bytes(CHUNK)
    c["ff"] = b"\xff" * CHUNK
    for per in range(1, 10):
        c["period_%d" % per] = (rnd(per) * (20_000 // per + 1))[:20_000]
    block = rnd(300)                                   # zeros in between: they leave the hash table's entries for the block alone
    c["distance_32768"] = block + bytes(32_768 - 300) + block
    c["distance_32769"] = block + bytes(32_769 - 300) + block
    c["runs_258_259_260"] = b"".join(rnd(50) + bytes([65 + k]) * n for k, n in enumerate((258, 259, 260, 258, 3, 4, 2, 700))) + rnd(50)
    c["chunk_ends_inside_a_run"] = rnd(CHUNK - 100) + b"A" * 100 + b"B" * 40 + rnd(500)
    c["random_1mb"] = rnd(1 << 20)
    for name, counts in (("fibonacci_22", fibonacci_counts(22)), ("fibonacci_40", fibonacci_counts(40, CHUNK))):
        v = np.concatenate([np.full(f, 3 + 5 * k, np.uint8) for k, f in enumerate(counts)])
        rng.shuffle(v)
        c[name] = v.tobytes()
    v = np.repeat(np.arange(256, dtype=np.uint8), CHUNK // 256)
    rng.shuffle(v)
    c["all_256_values"] = v.tobytes()
    c["one_distance"] = bytes(range(256)) * 4
    c["no_match"] = de_bruijn(12, 3)
    c["libdeflate_fixture"] = gzip.decompress(open(os.path.join(HERE, "golden", "libdeflate_bgzf.gz"), "rb").read())
    c["doubles"] = doubles_payload()
    assert len(c["fibonacci_40"]) == CHUNK and len(c["fibonacci_22"]) == 46_367 and len(c["all_256_values"]) == CHUNK
    return c


@functools.lru_cache(maxsize=None)
def stream_of(name):
    rc, stream, n_members, _, _ = deflate(cases()[name])
    assert rc == 0, lib().dropest_deflate_last_error()
    return stream, n_members


def inflate_fails(names, repeats=1):
    """every case's stream back through dropest_bgzf_inflate_buffer (the kernel this process was started for)"""
    fails = []
    for name in names:
        data, (stream, _) = cases()[name], stream_of(name)
        if not stream:
            continue
        out, status, _ = tg.inflate(stream, repeats)
        if status.any() or out != data:
            fails.append((name, np.flatnonzero(status).tolist()[:8]))
    return fails


@pytest.mark.parametrize("name", list(cases()))
def test_members(name):
    data, (stream, n_members) = cases()[name], stream_of(name)
    mem = members_of(stream)
    assert len(mem) == n_members == (len(data) + CHUNK - 1) // CHUNK
    for k, m in enumerate(mem):
        chunk = data[k * CHUNK:(k + 1) * CHUNK]
        assert zlib.decompress(m, wbits=31) == chunk, k
        assert struct.unpack("<II", m[-8:]) == (zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk)), k
        assert len(m) <= len(chunk) + 5 + 26, k
    assert gzip.decompress(stream) == data                       # the members as one stream, the way a .rds file is read
    assert not inflate_fails([name])
    assert deflate(data)[1] == stream                            # the same bytes on every run


def test_serial_inflate_kernel_reads_every_case():
    child = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_deflate as t; print('serial kernel fails:', t.inflate_fails(list(t.cases())))" \
            % (HERE, os.path.dirname(HERE))
    r = subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, timeout=300, env=dict(os.environ, DROPEST_INFLATE_PAR="0"))
    assert r.returncode == 0 and "serial kernel fails: []" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_random_bytes_are_stored():
    for m in members_of(stream_of("random_1mb")[0]):
        isize = struct.unpack("<I", m[-4:])[0]
        assert len(m) == isize + 5 + 26 and m[18] == 1 and struct.unpack_from("<HH", m, 19) == (isize, isize ^ 0xFFFF)


def test_zeros_are_full_length_matches():
    assert len(stream_of("zeros")[0]) * 100 < CHUNK


def test_distance_limit():
    """the second copy of the block is a match at 32 768 and literals at 32 769 (300 random bytes: about 300 bytes of payload against a few)"""
    assert len(stream_of("distance_32768")[0]) + 200 < len(stream_of("distance_32769")[0])


def test_doubles_beat_zlib_level_4_under_fixed_codes():
    data = cases()["doubles"]
    fixed = 0
    for at in range(0, len(data), CHUNK):
        z = zlib.compressobj(4, zlib.DEFLATED, 31, 8, zlib.Z_FIXED)
        fixed += len(z.compress(data[at:at + CHUNK]) + z.flush())
    mine = len(stream_of("doubles")[0])
    print("doubles: device %d bytes, zlib level 4 Z_FIXED %d bytes" % (mine, fixed))
    assert mine < fixed


def test_end_of_file_block():
    data = cases()["len_259"]
    rc, stream, n_members, _, _ = deflate(data, flags=1)
    assert rc == 0 and n_members == 2
    eof = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    assert stream == stream_of("len_259")[0] + eof
    rc, stream, n_members, _, _ = deflate(b"", flags=1)
    assert rc == 0 and n_members == 1 and stream == eof


def test_capacity_one_byte_short():
    data = cases()["len_%d" % (2 * CHUNK + 1)]
    stream, _ = stream_of("len_%d" % (2 * CHUNK + 1))
    rc, got, _, needed, out = deflate(data, out_cap=len(stream) - 1)
    assert rc == 1 and got is None and needed == len(stream)
    assert b"too small" in lib().dropest_deflate_last_error()
    assert (out == 0x5A).all()                                    # nothing of the caller's buffer was touched, the bytes behind the capacity least of all
    rc, got, _, _, _ = deflate(data, out_cap=len(stream))
    assert rc == 0 and got == stream
