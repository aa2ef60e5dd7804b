"""Minimal BAM writer (SAMv1 §4: BGZF container + BAM records), TEST INFRASTRUCTURE for the native BAM reader
(dropest_amd/csrc/host/bam_ingest.cpp) and the device decoder.  Records may straddle BGZF blocks (the byte stream is cut at `block` bytes,
chosen per file)."""
import struct
import zlib

_SEQ = {c: i for i, c in enumerate("=ACMGRSVTWYHKDBN")}


def _bgzf_block(data, level=6):
    comp = zlib.compressobj(level, zlib.DEFLATED, -15)
    cdata = comp.compress(data) + comp.flush()
    bsize = len(cdata) + 25
    return (b"\x1f\x8b\x08\x04" + b"\x00" * 4 + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize)
            + cdata + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


_B_SUB = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}     # B array subtype -> struct code (SAMv1 §4.2.4)
_NUM = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}


def _tag(tag, typ=None, value=None):
    """(tag, type, value) -> the bytes of one aux field.  Z / H: a string (NUL added); A: one character; c C s S i I f: a number;
    B: a list of int16, or (subtype, list) for any of the seven subtypes.  A bare bytes object is written as it stands (unknown types,
    values cut short: whatever a test needs)."""
    if isinstance(tag, (bytes, bytearray)):
        return bytes(tag)
    t = tag.encode() + typ.encode()
    if typ in ("Z", "H"):
        return t + (value if isinstance(value, bytes) else value.encode()) + b"\x00"
    if typ == "A":
        return t + (value if isinstance(value, bytes) else value.encode())[:1]
    if typ in _NUM:
        return t + struct.pack(_NUM[typ], value)
    if typ == "B":                     # value = list of int16, or (subtype, list)
        sub, vals = value if isinstance(value, tuple) else ("s", value)
        return t + sub.encode() + struct.pack("<I", len(vals)) + struct.pack("<%d%s" % (len(vals), _B_SUB[sub]), *vals)
    raise ValueError(typ)


_CIGAR = {c: i for i, c in enumerate("MIDNSHP=X")}


def record(ref_id, pos, name, flag=0, mapq=255, seq="ACGT" * 10, tags=(), cigar=None, qual=None, next_ref=-1, next_pos=-1, l_read_name=None):
    """cigar: list of (length, op) -- default one M over the whole read (an empty list: no CIGAR at all).  name: str or bytes (NUL added).
    qual: the quality bytes (default 0xFF each).  l_read_name: the field as written, whatever the name's length (the record's bytes stay
    as they are: block_size counts them).  tags: (tag, type, value) triples or raw bytes (see _tag)."""
    n = len(seq)
    ops = [(n, "M")] if cigar is None else cigar
    cigar = b"".join(struct.pack("<I", (ln << 4) | (_CIGAR[op] if isinstance(op, str) else op)) for ln, op in ops)
    packed = bytearray((n + 1) // 2)
    for i, c in enumerate(seq):
        packed[i // 2] |= _SEQ[c] << (4 if i % 2 == 0 else 0)
    nm = (name if isinstance(name, bytes) else name.encode()) + b"\x00"
    body = struct.pack("<iiBBHHHIiii", ref_id, pos, len(nm) if l_read_name is None else l_read_name, mapq, 4680, len(ops), flag, n, next_ref, next_pos, 0)
    body += nm + cigar + bytes(packed) + (b"\xff" * n if qual is None else bytes(qual)) + b"".join(_tag(*t) if isinstance(t, tuple) else _tag(t) for t in tags)
    return struct.pack("<I", len(body)) + body


def write_bam(path, refs, records, block=0xFF00, header_text="@HD\tVN:1.6\tSO:unsorted\n", repeat=1, compress=None):
    """compress: bytes -> one BGZF block (default: zlib at level 6); the end-of-file block is always zlib's"""
    compress = compress or _bgzf_block
    text = header_text + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, ln) for n, ln in refs)
    raw = b"BAM\x01" + struct.pack("<I", len(text)) + text.encode() + struct.pack("<I", len(refs))
    for n, ln in refs:
        raw += struct.pack("<I", len(n) + 1) + n.encode() + b"\x00" + struct.pack("<I", ln)
    if repeat > 1:      # the records `repeat` times over (benchmarks): the header in blocks of its own, the records' blocks written again and again
        body = b"".join(records)
        blocks = [compress(body[o:o + block]) for o in range(0, len(body), block)]
        with open(path, "wb") as f:
            for o in range(0, len(raw), block):
                f.write(compress(raw[o:o + block]))
            for _ in range(repeat):
                for b in blocks:
                    f.write(b)
            f.write(_bgzf_block(b""))
        return
    raw += b"".join(records)
    with open(path, "wb") as f:
        for o in range(0, len(raw), block):
            f.write(compress(raw[o:o + block]))
        f.write(_bgzf_block(b""))       # EOF marker block
