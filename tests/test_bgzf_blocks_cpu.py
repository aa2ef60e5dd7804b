"""The BGZF block walks of the BAM readers (dropest_amd/csrc/host/bgzf_blocks.h) on the host alone: read_block (the host reader, the header of the
device path), whole_blocks over bytes in memory, FileWalk::walk_blocks / whole_blocks_of_file through pread (the device path's window reader, with
the four stretches).  All four read a block's header with one parse_header and keep verdicts of their own; tests/cpp/test_bgzf_blocks.cpp is
compiled with the header alone (address and undefined-behaviour sanitizers, where the compiler has them) and answers a script of calls, and every
answer is compared with the block table this file reads from the BAM file itself, or with the error text that caller gives.  The same for the
device decoder's table (BlockTable: filled from bytes by the walk of dropest_bgzf_scan, or from a caller's table that is checked first)."""
import os
import struct
import subprocess
import zlib

import pytest

from bam_writer import record, write_bam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = 2 ** 62


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bgzf") / "test_bgzf_blocks")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "cpp", "test_bgzf_blocks.cpp"), "-o", out, "-pthread"]
    if subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True).returncode:
        subprocess.check_call(cmd)             # (a compiler without the sanitizers' runtime)
    return out


def ask(exe, path, commands):
    """One run of the program: commands -> [(o, stretched, error, table)]"""
    script = path + ".script"
    with open(script, "w") as f:
        f.write("".join(c + "\n" for c in commands))
    res = subprocess.run([exe, path, script], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert res.returncode == 0, res.stderr[-2000:]
    rows = [ln.split("\t") for ln in res.stdout.split("\n")[:-1]]
    assert len(rows) == len(commands)
    return [(int(o), int(s), e, [tuple(int(x) for x in b.split(",")) for b in t.split(";") if b]) for o, s, e, t in rows]


def extra_block(extra, bc=None):
    """compress= hook of write_bam: a block with the extra field given (bc: what the BC subfield says instead of the block's size - 1)"""
    def compress(data):
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        cdata = c.compress(data) + c.flush()
        total = 12 + len(extra(0)) + len(cdata) + 8
        return (b"\x1f\x8b\x08\x04" + b"\x00" * 4 + b"\x00\xff" + struct.pack("<H", len(extra(0))) + extra(total - 1 if bc is None else bc)
                + cdata + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))
    return compress


BC = lambda v: b"BC" + struct.pack("<HH", 2, v)
TWO_SUBFIELDS = extra_block(lambda v: b"XY" + struct.pack("<H", 2) + b"\x01\x02" + BC(v))                  # XLEN 12
LONG_EXTRA = extra_block(lambda v: b"XY" + struct.pack("<H", 60) + bytes(60) + BC(v))                      # XLEN 70: beyond the 52 bytes read ahead
NO_BC = extra_block(lambda v: b"XY" + struct.pack("<H", 2) + struct.pack("<H", v))
BC_OF_FOUR = extra_block(lambda v: b"BC" + struct.pack("<H", 4) + struct.pack("<I", v))
SMALL_BC = extra_block(BC, bc=10)                                                                          # 11 bytes: less than header + trailer


def bad_magic(data):
    return b"\x1e" + extra_block(BC)(data)[1:]


def only_block(k, special):
    """the k-th block of the file from `special`, the others as htslib writes them"""
    calls = [0]

    def compress(data):
        calls[0] += 1
        return special(data) if calls[0] == k + 1 else extra_block(BC)(data)
    return compress


def records(n):
    return [record(i % 3, 100 + i, "r%d!ACGTACGTACGT#ACGTAC" % i, seq="ACGT" * 6, tags=[("GX", "Z", "G%d" % (i % 50))]) for i in range(n)]


REFS = [("chr1", 100000), ("chr2", 100000), ("chr3", 100000)]


def blocks_of(path):
    """[(start, end, offset of the deflate stream, its length, ISIZE, CRC)] read from the file: the model the walks are compared with"""
    raw, at, out = open(path, "rb").read(), 0, []
    while at < len(raw):
        assert raw[at:at + 4] == b"\x1f\x8b\x08\x04"
        xlen, x, bsize = struct.unpack_from("<H", raw, at + 10)[0], 0, None
        while x + 4 <= xlen:
            sl = struct.unpack_from("<H", raw, at + 12 + x + 2)[0]
            if raw[at + 12 + x:at + 14 + x] == b"BC" and sl == 2:
                bsize = struct.unpack_from("<H", raw, at + 12 + x + 4)[0] + 1
            x += 4 + sl
        crc, isize = struct.unpack_from("<II", raw, at + bsize - 8)
        out.append((at, at + bsize, at + 12 + xlen, bsize - 12 - xlen - 8, isize, crc))
        at += bsize
    return out


GOOD = {"b3": (3, 1500, None), "b61": (61, 2000, None), "b997": (997, 5000, None), "bFF00": (0xFF00, 20000, None),
        "two_subfields": (997, 2000, TWO_SUBFIELDS), "long_extra": (997, 2000, LONG_EXTRA)}


@pytest.fixture(scope="module")
def good(tmp_path_factory):
    d = tmp_path_factory.mktemp("bams")
    out = {}
    for name, (block, n, compress) in GOOD.items():
        path = str(d / (name + ".bam"))
        write_bam(path, REFS, records(n), block=block, compress=compress)
        out[name] = (path, blocks_of(path))
    return out


def table(blocks):
    return [b[2:] for b in blocks]


STRETCH = "-1 64 1 1 0"         # block_cap avg_block least_bytes least_blocks one_walker: every window takes the four stretches


@pytest.mark.parametrize("name", list(GOOD))
def test_every_walk_reads_the_same_table(exe, good, name):
    path, blocks = good[name]
    size = blocks[-1][1]
    assert len(blocks) >= 4
    for first in (0, len(blocks) // 3):     # the whole file, and from a block inside it (as a window of the device path begins)
        at = blocks[first][0]
        rb, wbt, walk, one, four = ask(exe, path, ["rb %d %d" % (size, at), "wbt %d %d" % (size, at), "walk %d 0 %d %d -1" % (at, size - at, size - at),
                                                   "wbf %d %d %d -1 16384 8388608 8192 0" % (at, size - at, size - at), "wbf %d %d %d %s" % (at, size - at, size - at, STRETCH)])
        for o, stretched, error, got in (rb, wbt, walk, one, four):
            assert error == "" and got == table(blocks[first:])
        assert rb[0] == size and wbt[0] == size and walk[0] == one[0] == four[0] == size - at
        assert not one[1]
        # the stretches are begun at blocks found by the sixteen bytes htslib writes (XLEN 6): other extra fields leave the window to one walker
        assert four[1] == (0 if name in ("two_subfields", "long_extra") else 1)


def test_stretches_that_cannot_meet_leave_the_window_to_one_walker(exe, tmp_path):
    path = str(tmp_path / "few.bam")
    write_bam(path, REFS, records(900), block=0xFF00)
    blocks = blocks_of(path)
    assert len(blocks) == 3                  # two of records and the empty one that ends the file: no four stretches in that
    size = blocks[-1][1]
    (o, stretched, error, got), = ask(exe, path, ["wbf 0 %d %d %s" % (size, size, STRETCH)])
    assert (o, stretched, error, got) == (size, 0, "", table(blocks))


def test_cut_offs(exe, good):
    path, blocks = good["b997"]
    size, starts = blocks[-1][1], [b[0] for b in blocks]
    first_len = blocks[0][1]
    cuts = [1, first_len - 1, first_len, first_len + 1, blocks[7][0], blocks[7][0] + 1, size // 2, size, size + 1000]
    answers = ask(exe, path, ["wb %d 0 %d -1" % (size, w) for w in cuts] + ["walk 0 0 %d %d -1" % (u, size) for u in cuts] + ["wbf 0 %d %d -1 16384 8388608 8192 0" % (size, w) for w in cuts]
                  + ["wbf 0 %d %d %s" % (size, w, STRETCH) for w in cuts])
    for k, (o, stretched, error, got) in enumerate(answers):
        cut = cuts[k % len(cuts)]
        expect = [b for b in blocks if b[0] < cut or b[0] == 0]      # at least one block, none that begins at or beyond the cut
        assert error == "" and o == expect[-1][1]
        if k >= len(cuts):
            assert got == table(expect)
    caps = [1, 2, 9]
    answers = ask(exe, path, ["wb %d 0 %d %d" % (size, size, c) for c in caps] + ["walk 0 0 %d %d %d" % (size, size, c) for c in caps]
                  + ["wbf 0 %d %d %d 16384 8388608 8192 0" % (size, size, c) for c in caps] + ["wbf 0 %d %d %d 64 1 1 0" % (size, size, c) for c in caps])
    for k, (o, stretched, error, got) in enumerate(answers):
        assert error == "" and o == blocks[caps[k % len(caps)] - 1][1]
    # a window inside the file: `avail` ends it whatever lies behind, offsets are the window's
    at, end = starts[5], blocks[11][1]
    (o, _, error, got), = ask(exe, path, ["walk %d 0 %d %d -1" % (at, ALL, end - at + 17)])
    assert (o, error, got) == (end - at, "", table(blocks[5:12]))


@pytest.mark.parametrize("name", list(GOOD))
def test_truncated_files(exe, good, name):
    """Every prefix around the last two block boundaries.  From the walks' own conditions: a block that is not whole is not in the table; read_block
    then throws by how much of it is there (fewer than 12 bytes: not BGZF; fewer than the header: truncated header; else truncated block); the
    others stop in front of it without a word (a prefix with whole blocks in it is not an error to them)."""
    path, blocks = good[name]
    size = blocks[-1][1]
    blocks = blocks[-6:]                 # (the walks begin a few blocks in front of the cut: at, as offset or as the window's place in the file)
    at = blocks[0][0]
    lengths = sorted({n for b in (blocks[-2][1], size) for n in range(b - 20, b + 21) if n <= size})
    commands = []
    for n in lengths:
        commands += ["rb %d %d" % (n, at), "wbt %d %d" % (n, at), "wb %d %d %d -1" % (n, at, n), "walk %d 0 %d %d -1" % (at, n - at, n - at),
                     "wbf %d %d %d -1 16384 8388608 8192 0" % (at, n - at, n - at), "wbf %d %d %d %s" % (at, n - at, n - at, STRETCH)]
    answers = ask(exe, path, commands)
    for k, n in enumerate(lengths):
        whole = [b for b in blocks if b[1] <= n]
        end = whole[-1][1]
        rest = n - end
        xlen = [b[2] - b[0] - 12 for b in blocks if b[0] == end][0] if rest else 0      # of the block that is cut
        rb, wbt, wb, walk, one, four = answers[6 * k:6 * k + 6]
        assert rb == (end, 0, "" if not rest else "Not a BGZF/BAM file: FILE" if rest < 12 else "Truncated BGZF header: FILE" if rest < 12 + xlen else "Truncated BGZF block: FILE", table(whole)), n
        assert wbt == (end, 0, "Truncated BGZF block" if rest else "", table(whole)), n     # (asked for the block at `end` alone, where nothing whole is)
        assert wb == (end - at, 0, "", []), n
        for o, stretched, error, got in (walk, one, four):
            assert (o, error, got) == (end - at, "", table(whole)), n
    (o, _, error, got), = ask(exe, path, ["walk 0 0 10 10 -1"])      # nothing whole at all
    assert (o, error, got) == (0, "", [])
    assert [a[:3] for a in ask(exe, path, ["wb 10 0 10 -1", "wbf 0 10 10 -1 16384 8388608 8192 0"])] == [(0, 0, "Truncated BGZF block")] * 2


BAD = {   # what the third block is -> the error of read_block / whole_blocks / walk_blocks and whole_blocks_of_file
    "no_bc": (NO_BC, "BGZF block without BC subfield: FILE", "BGZF block without BC subfield", "BGZF block without BC subfield"),
    "bc_of_four": (BC_OF_FOUR, "BGZF block without BC subfield: FILE", "BGZF block without BC subfield", "BGZF block without BC subfield"),
    "bad_magic": (bad_magic, "Not a BGZF/BAM file: FILE", "Not a BGZF/BAM file", "Not a BGZF/BAM file"),
    # whole_blocks believes the eleven bytes and finds no block behind them; walk_blocks alone sees that the size cannot hold the header
    "small_bc": (SMALL_BC, "Corrupt BGZF block size: FILE", "Not a BGZF/BAM file", "BGZF block without BC subfield"),
}


@pytest.mark.parametrize("name", list(BAD))
def test_malformed_blocks_and_each_walks_words_for_them(exe, tmp_path, name):
    special, e_read, e_whole, e_walk = BAD[name]
    path = str(tmp_path / (name + ".bam"))
    write_bam(path, REFS, records(300), block=997, compress=only_block(2, special))
    size = os.path.getsize(path)
    good_two = blocks_of_prefix(path, 2)
    rb, wb, walk, one, four = ask(exe, path, ["rb %d 0" % size, "wb %d 0 %d -1" % (size, size), "walk 0 0 %d %d -1" % (size, size), "wbf 0 %d %d -1 16384 8388608 8192 0" % (size, size),
                                              "wbf 0 %d %d %s" % (size, size, STRETCH)])
    assert rb == (good_two[-1][1], 0, e_read, table(good_two))
    assert wb == (0, 0, e_whole, [])
    assert (walk[0], walk[2]) == (0, e_walk) and (one[0], one[2]) == (0, e_walk) and (four[0], four[1], four[2]) == (0, 0, e_walk)


def blocks_of_prefix(path, n):
    """the first n blocks (those of a file whose later blocks blocks_of cannot read)"""
    raw, at, out = open(path, "rb").read(), 0, []
    for _ in range(n):
        bsize = struct.unpack_from("<H", raw, at + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", raw, at + bsize - 8)
        out.append((at, at + bsize, at + 18, bsize - 26, isize, crc))
        at += bsize
    return out


def test_isize_beyond_64_kb_is_walk_blocks_alone_to_reject(exe, tmp_path):
    def large(data):
        b = extra_block(BC)(data)
        return b[:-4] + struct.pack("<I", 65537)
    path = str(tmp_path / "isize.bam")
    write_bam(path, REFS, records(300), block=997, compress=only_block(2, large))
    size = os.path.getsize(path)
    rb, wb, walk = ask(exe, path, ["rb %d 0" % size, "wb %d 0 %d -1" % (size, size), "walk 0 0 %d %d -1" % (size, size)])
    assert rb[0] == size and rb[2] == "" and rb[3][2][2] == 65537 and wb[:3] == (size, 0, "")
    assert (walk[0], walk[2]) == (0, "BGZF block with ISIZE beyond 64 KB")


def test_parse_header_reads_within_its_bytes(exe, tmp_path):
    # a BC subfield whose two bytes lie beyond XLEN (4): only the window-size probe of the device path takes it (bsize_cut)
    path = str(tmp_path / "cut.bin")
    open(path, "wb").write(b"\x1f\x8b\x08\x04" + bytes(6) + struct.pack("<H", 4) + b"BC" + struct.pack("<HH", 2, 99) + bytes(8))
    a = [r[2] for r in ask(exe, path, ["hdr 0 %d" % n for n in (0, 11, 12, 15, 16, 17, 18, 26)])]
    assert a == ["0,0,0,0,0", "0,0,0,0,0", "1,0,4,0,0", "1,0,4,0,0", "1,1,4,0,0", "1,1,4,0,0", "1,1,4,0,100", "1,1,4,0,100"]


# ---- BlockTable: the table of the device path (dropest_bgzf_scan, the decoder's windows and uploads) --------------------------------------
def table5(blocks):
    """(offset of the deflate stream, its length, ISIZE, CRC, offset out) as BlockTable holds them"""
    out, total = [], 0
    for b in blocks:
        out.append(b[2:] + (total,))
        total += b[4]
    return out


def filled(blocks, end=None):
    """the answer for whole, sound blocks: used, ok, "n=..,total=..", the table"""
    return (blocks[-1][1] if end is None and blocks else end or 0, 1, "n=%d,total=%d" % (len(blocks), sum(b[4] for b in blocks)), table5(blocks))


def test_block_table_from_bytes(exe, good, tmp_path):
    path, blocks = good["b3"]
    size = blocks[-1][1]
    eof = blocks[-1]
    assert eof[1] - eof[0] == 28 and eof[4] == 0                      # the 28 bytes that end a file
    k = len(blocks) // 2
    cuts = [blocks[k][0] + c for c in (1, 11, 12, 17)] + [blocks[k][2], blocks[k][2] + 1, blocks[k][1] - 9, blocks[k][1] - 1]      # inside the 18 header bytes, inside the payload and the trailer
    answers = ask(exe, path, ["tab 0 0", "tab %d %d" % (size, eof[0]), "tab %d 0" % size, "tab %d %d" % (size, blocks[k][0])] + ["tab %d 0" % c for c in cuts])
    assert answers[0] == (0, 1, "n=0,total=0", [])                    # no byte: no block, and nothing wrong
    assert answers[1] == (28, 1, "n=1,total=0", [eof[2:] + (0,)])
    assert answers[2] == filled(blocks)
    assert answers[3] == filled(blocks[k:], size - blocks[k][0])      # from a block inside the file: offsets out begin at 0 (offsets in: the program adds FROM)
    for a in answers[4:]:                                             # a block that is cut off ends the table without a word: `used` says how far it reaches
        assert a == filled(blocks[:k])
    # an extra subfield in front of BC, an extra field beyond 64 bytes
    for name in ("two_subfields", "long_extra"):
        path, blocks = good[name]
        assert ask(exe, path, ["tab %d 0" % blocks[-1][1]]) == [filled(blocks)]


def bc_beyond_xlen(data):
    """XLEN 4: the BC subfield's two data bytes are the first two of what follows the extra field"""
    b = extra_block(BC)(data)
    return b[:10] + struct.pack("<H", 4) + b[12:]


def isize(v):
    return lambda data: extra_block(BC)(data)[:-4] + struct.pack("<I", v)


BAD_TABLE = {  # the third block -> what dropest_bgzf_scan says of it (%d: the offset of the block's first byte)
    "bc_of_four": (BC_OF_FOUR, "BGZF block without a BC subfield at offset %d"),
    "no_bc": (NO_BC, "BGZF block without a BC subfield at offset %d"),
    "bc_beyond_xlen": (bc_beyond_xlen, "BGZF block without a BC subfield at offset %d"),
    "small_bc": (SMALL_BC, "BGZF block without a BC subfield at offset %d"),
    "isize_65537": (isize(65537), "BGZF block with ISIZE beyond 64 KB at offset %d"),
    "bad_magic": (bad_magic, "not a BGZF block header at offset %d"),
}


@pytest.mark.parametrize("name", list(BAD_TABLE))
def test_block_table_of_malformed_blocks(exe, tmp_path, name):
    special, error = BAD_TABLE[name]
    path = str(tmp_path / (name + ".bam"))
    write_bam(path, REFS, records(300), block=997, compress=only_block(2, special))
    size = os.path.getsize(path)
    two = blocks_of_prefix(path, 2)
    at = two[-1][1]
    header = 12 + struct.unpack_from("<H", open(path, "rb").read(), at + 10)[0]
    whole, inside, before = ask(exe, path, ["tab %d 0" % size, "tab %d 0" % (at + max(header, 18)), "tab %d 0" % (at + max(header, 18) - 1)])
    assert whole == (0, 0, error % at, [])                            # nothing of a window with such a block is kept
    assert inside == (filled(two) if name == "isize_65537" else whole)      # (judged by its trailer: the header alone is a block cut off)
    assert before == filled(two)                                      # the header not whole, or fewer than 18 bytes of it: a block cut off


def test_block_table_takes_isize_65536(exe, tmp_path):
    path = str(tmp_path / "isize.bam")
    write_bam(path, REFS, records(300), block=997, compress=only_block(2, isize(65536)))
    raw = open(path, "rb").read()
    (used, ok, said, got), = ask(exe, path, ["tab %d 0" % len(raw)])
    assert (used, ok) == (len(raw), 1) and got[2][2] == 65536 and got[3][4] == got[2][4] + 65536


def test_block_table_from_a_callers_table(exe, good):
    """A sound table is taken as it is (the CRCs the program made up show it); one that is not -- blocks that overlap, a last block short of the
    bytes' end, an ISIZE beyond 64 KB, an array missing -- leaves the walk to decide, whose table is the file's.  What is checked is what the
    kernel relies on (room for a header in front of each block, ends within the bytes): a block left out in the middle is no offence."""
    path, blocks = good["b997"]
    size = blocks[-1][1]
    answers = dict(zip(("good", "gap", "overlap", "short", "big", "null"), ask(exe, path, ["cal %d 0 %s" % (size, how) for how in ("good", "gap", "overlap", "short", "big", "null")])))
    plus_one = lambda rows: [r[:3] + ((r[3] + 1) & 0xFFFFFFFF,) + r[4:] for r in rows]
    assert answers["good"] == filled(blocks)[:3] + (plus_one(table5(blocks)),)
    left_out = blocks[:1] + blocks[2:]
    assert answers["gap"] == (size, 1, "n=%d,total=%d" % (len(left_out), sum(b[4] for b in left_out)), plus_one(table5(left_out)))
    for how in ("overlap", "short", "big", "null"):
        assert answers[how] == filled(blocks), how
    # ... and from a block inside the file, as a window begins
    at = blocks[5][0]
    (used, ok, said, got), = ask(exe, path, ["cal %d %d short" % (size, at)])
    assert (used, ok, got) == (size - at, 1, table5(blocks[5:]))
