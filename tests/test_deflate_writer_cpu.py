"""The DEFLATE corpus of tests/deflate_writer.py (streams zlib's encoder never writes) checked against zlib, then through the BAM reader's
host decoder (dropest_amd/csrc/host/fast_inflate.h).  The writer is judged first -- every VALID case must give exactly its bytes from zlib,
every MALFORMED or INCOMPLETE case must be refused by zlib -- so that an encoder bug cannot pass for a decoder bug.  The host decoder must
take every valid case (a refusal silently hands real files to zlib: correct, but the fast path is lost without anyone noticing) and refuse
every malformed one.

Policy for INCOMPLETE codes (a Huffman code with unused bit patterns that the stream never reaches -- zlib refuses the header; libdeflate
decodes such streams): the project's decoders check codes for over-subscription only, so they decode these streams and give the encoded
bytes.  The host decoder and both device kernels must agree on that (tests/test_gpu_inflate_edges.py); a stream that REACHES an unused
pattern is malformed for all of them."""
import ctypes as C
import gzip
import os
import struct
import zlib

import numpy as np
import pytest

import deflate_writer as dw
from dropest_amd.build import FACADE_LIB, build_facade

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "libdeflate_bgzf.gz")


@pytest.fixture(scope="module")
def lib():
    build_facade()
    L = C.CDLL(FACADE_LIB)
    L.dropest_test_fast_inflate.restype = C.c_int
    L.dropest_test_fast_inflate.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64]
    return L


def host_inflate(L, comp, n):
    out = np.full(n + 16, 0xAB, np.uint8)                       # (the decoder may not write past n)
    ok = L.dropest_test_fast_inflate(comp, len(comp), out.ctypes.data, n)
    assert (out[n:] == 0xAB).all()
    return bool(ok), out[:n].tobytes()


def test_writer_against_zlib():
    cases = dw.corpus()
    seen = {dw.VALID: 0, dw.MALFORMED: 0, dw.INCOMPLETE: 0}
    for c in cases:
        seen[c.verdict] += 1
        try:
            got, err = zlib.decompress(c.payload, -15), None
        except zlib.error as e:
            got, err = None, e
        if c.verdict == dw.VALID:
            assert err is None and got == c.data, (c.name, err)
        elif c.name.startswith("wrong_isize"):
            assert got is not None and len(got) != len(c.data), c.name          # (a valid stream: the size asked for is the fault)
        else:
            assert err is not None, (c.name, c.verdict)
    assert seen[dw.VALID] > 150 and seen[dw.MALFORMED] > 25 and seen[dw.INCOMPLETE] >= 3, seen
    assert all(c.fits_bgzf for c in cases if not c.name.startswith("stored_65535")), [c.name for c in cases if not c.fits_bgzf]


def test_writer_pieces():
    """the encoder's own parts: canonical codes (RFC 1951 3.2.2's example), length / distance symbols at their edges, complete codes"""
    assert dw.canonical([3, 3, 3, 3, 3, 2, 4, 4]) == [2, 3, 4, 5, 6, 0, 14, 15]
    assert dw.len_symbol(258) == (285, 0, 0) and dw.len_symbol(257) == (284, 30, 5) and dw.len_symbol(3) == (257, 0, 0)
    assert dw.dist_symbol(32_768) == (29, 8191, 13) and dw.dist_symbol(1) == (0, 0, 0)
    for n, fixed in ((286, None), (30, None), (286, {65: 1}), (19, None)):
        assert dw.kraft(dw.complete_lengths(n, fixed)) == 32768
    ll, dl = dw.geometry_code()
    assert ll[ord("A")] == 1 and ll[284] == 15 and dl[29] == 15 and sorted(set(ll) - {0}) == list(range(1, 16))
    syms, ll, dl = dw._cl_sequence(False)
    assert {s for s, _ in syms} >= {16, 17, 18} and (16, 3) in syms and (16, 0) in syms and (17, 7) in syms and (18, 127) in syms


def test_host_decoder_on_the_corpus(lib):
    wrong = []
    for c in dw.corpus():
        ok, got = host_inflate(lib, c.payload, c.out_size)
        if c.verdict == dw.MALFORMED:
            if ok and not (c.bad_crc is not None):
                wrong.append((c.name, "taken"))
        elif not ok or got != c.data:
            wrong.append((c.name, "refused" if not ok else "bytes differ"))
    assert not wrong, wrong


def test_host_decoder_every_corpus_block_in_bgzf_form(lib):
    """the same cases as the BAM reader sees them: cut out of BGZF blocks by ISIZE, the CRC-32 of the result equal to the trailer's"""
    for c in dw.corpus():
        if not c.fits_bgzf or c.verdict == dw.MALFORMED:
            continue
        blk = c.block()
        bsize = struct.unpack_from("<H", blk, 16)[0] + 1
        crc, isize = struct.unpack_from("<II", blk, bsize - 8)
        ok, got = host_inflate(lib, blk[18:bsize - 8], isize)
        assert ok and zlib.crc32(got) == crc, c.name


def _golden_blocks():
    blob = open(GOLDEN, "rb").read()
    at, out = 0, []
    while at < len(blob):
        bsize = struct.unpack_from("<H", blob, at + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", blob, at + bsize - 8)
        out.append((blob[at + 18:at + bsize - 8], isize, crc))
        at += bsize
    return blob, out


def test_libdeflate_fixture_through_the_host_decoder(lib):
    """BGZF blocks libdeflate wrote (levels 1, 6, 9, 12; scripts/make_libdeflate_fixture.py): the fixture checks itself through gzip"""
    blob, blocks = _golden_blocks()
    want = gzip.decompress(blob)
    assert len(blocks) >= 30 and len(want) > 500_000
    got = []
    for payload, isize, crc in blocks:
        ok, b = host_inflate(lib, payload, isize)
        assert ok and zlib.crc32(b) == crc
        got.append(b)
    assert b"".join(got) == want


def test_fresh_libdeflate_streams_through_the_host_decoder(lib):
    ld = dw.libdeflate()
    if ld is None:
        pytest.skip("no libdeflate shared library on this machine: the fresh-stream leg needs one (the committed fixture is checked anyway)")
    for level, data in dw.libdeflate_samples(np.random.default_rng(41)):
        comp = ld.compress(data, level)
        ok, got = host_inflate(lib, comp, len(data))
        assert ok and got == data, level
