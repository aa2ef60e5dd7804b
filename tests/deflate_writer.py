"""A bit-level RFC 1951 encoder (TEST INFRASTRUCTURE, pure Python: no zlib on the encoding side) and the corpus of DEFLATE streams that
zlib's encoder never writes but htslib / libdeflate files may hold: codes of 15 bits and of every length, degenerate codes, code-length
sequences with every repeat form, hundreds of blocks per BGZF block, ISIZE = 65 536, symbols placed across the parallel kernel's chunk and
span boundaries, matches that make its window slide -- and malformed streams every decoder must refuse.

Every case records the bytes it encodes and a verdict: VALID (zlib gives exactly those bytes), MALFORMED (zlib refuses it, and so must
the project's decoders) or INCOMPLETE (a Huffman code with unused bit patterns that the stream never reaches: zlib refuses the header,
tests/test_deflate_writer_cpu.py pins what the project's decoders do).  tests/test_deflate_writer_cpu.py checks every case against zlib
before any decoder is judged by it."""
import struct
import zlib

import numpy as np

VALID, MALFORMED, INCOMPLETE = "valid", "malformed", "incomplete"

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def len_symbol(n):
    """length 3..258 -> (symbol, extra value, extra bits); 258 is symbol 285"""
    k = 28 if n == 258 else max(i for i in range(28) if LEN_BASE[i] <= n)
    return 257 + k, n - LEN_BASE[k], LEN_EXTRA[k]


def dist_symbol(d):
    k = max(i for i in range(30) if DIST_BASE[i] <= d)
    return k, d - DIST_BASE[k], DIST_EXTRA[k]


class BitWriter:
    """bits LSB first (RFC 1951 3.1.1); Huffman codes most significant bit first"""
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value, n):
        assert 0 <= value < (1 << n) or n == 0
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def put_code(self, code, length):
        self.put(int("{:0{}b}".format(code, length)[::-1], 2), length)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    @property
    def nbits(self):
        return len(self.out) * 8 + self.n

    def getvalue(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canonical(lens):
    """code lengths -> the canonical codes (RFC 1951 3.2.2); None for unused symbols.  Over-subscribed lengths are coded anyway (the
    malformed cases need them): codes then wrap and collide, which is what a decoder must refuse."""
    bl = [0] * 16
    for ln in lens:
        if ln:
            bl[ln] += 1
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = []
    for ln in lens:
        if ln:
            out.append(nxt[ln] & ((1 << ln) - 1)); nxt[ln] += 1
        else:
            out.append(None)
    return out


def kraft(lens):
    """sum of 2^-len in units of 2^-15: 32768 = complete, less = incomplete, more = over-subscribed"""
    return sum(1 << (15 - ln) for ln in lens if ln)


def complete_lengths(n, fixed=None, symbols=None, max_len=15):
    """A complete code over `symbols` (default: all n) of an n-symbol alphabet: fixed {symbol: length} first, the others filled so that the
    Kraft sum is exactly 1 (as short as the budget allows, front to back)."""
    fixed = dict(fixed or {})
    symbols = list(range(n)) if symbols is None else list(symbols)
    lens = [0] * n
    budget = 1 << max_len
    for s, ln in fixed.items():
        lens[s] = ln
        budget -= 1 << (max_len - ln)
    rest = [s for s in symbols if s not in fixed]
    if not fixed and len(rest) == 1:      # (one symbol: the single code of one bit, which zlib takes as well)
        lens[rest[0]] = 1
        return lens
    assert 0 <= len(rest) <= budget, (len(rest), budget)
    cost = {s: 1 for s in rest}
    left = budget - len(rest)
    for s in rest:
        while cost[s] <= left and cost[s] < (1 << (max_len - 1)):
            left -= cost[s]; cost[s] *= 2
    assert left == 0, left
    for s in rest:
        lens[s] = max_len - (cost[s].bit_length() - 1)
    assert kraft(lens) == 1 << max_len
    return lens


def huffman_lengths(freq, limit):
    """code lengths of a Huffman code for freq (0 = unused), at most `limit` bits (frequencies halved until it fits); one used symbol: length 1"""
    import heapq
    freq = list(freq)
    used = [i for i, f in enumerate(freq) if f]
    lens = [0] * len(freq)
    if len(used) == 1:
        lens[used[0]] = 1
        return lens
    while True:
        heap = [(freq[i], i, [i]) for i in used]
        heapq.heapify(heap)
        depth = [0] * len(freq)
        uid = len(freq)
        while len(heap) > 1:
            fa, _, a = heapq.heappop(heap)
            fb, _, b = heapq.heappop(heap)
            for s in a + b:
                depth[s] += 1
            heapq.heappush(heap, (fa + fb, uid, a + b)); uid += 1
        if max(depth) <= limit:
            return depth
        freq = [(f + 1) // 2 if f else 0 for f in freq]


# ---- tokens -----------------------------------------------------------------------------------------------------------------------------
# an int 0..255: a literal; ("M", length, distance): a match; ("S", symbol, extra value, extra bits): a raw literal/length symbol (the caller
# writes the distance after a length symbol as ("D", symbol, extra value, extra bits)); EOB is written by the block unless eob=False
def expand(tokens, history=b""):
    """the bytes the tokens decode to behind `history` (raw symbols taken as a decoder reads them); None where a decoder must refuse"""
    out = bytearray(history)
    pend = None
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif t[0] == "M":
            _, ln, d = t
            if d > len(out) or d < 1:
                return None
            for _ in range(ln):
                out.append(out[-d])
        elif t[0] == "S":
            s, v = t[1], t[2]
            if s < 256:
                out.append(s)
            elif s == 256 or s > 285:
                return None
            else:
                pend = LEN_BASE[s - 257] + v
        elif t[0] == "D":
            s, v = t[1], t[2]
            if s > 29 or pend is None:
                return None
            d = DIST_BASE[s] + v
            if d > len(out):
                return None
            for _ in range(pend):
                out.append(out[-d])
            pend = None
    return bytes(out[len(history):])


def tokens_use(tokens):
    """(literal/length symbol counts, distance symbol counts) of the tokens, EOB included"""
    lf, df = [0] * 288, [0] * 32
    for t in tokens:
        if isinstance(t, int):
            lf[t] += 1
        elif t[0] == "M":
            lf[len_symbol(t[1])[0]] += 1; df[dist_symbol(t[2])[0]] += 1
        elif t[0] == "S":
            lf[t[1]] += 1
        else:
            df[t[1]] += 1
    lf[256] += 1
    return lf, df


def _put_tokens(w, tokens, lcodes, llens, dcodes, dlens, eob=True):
    for t in tokens:
        if isinstance(t, int):
            w.put_code(lcodes[t], llens[t])
        elif t[0] == "M":
            s, v, n = len_symbol(t[1])
            w.put_code(lcodes[s], llens[s]); w.put(v, n)
            s, v, n = dist_symbol(t[2])
            w.put_code(dcodes[s], dlens[s]); w.put(v, n)
        elif t[0] == "S":
            w.put_code(lcodes[t[1]], llens[t[1]]); w.put(t[2], t[3])
        else:
            w.put_code(dcodes[t[1]], dlens[t[1]]); w.put(t[2], t[3])
    if eob:
        w.put_code(lcodes[256], llens[256])


def cl_symbols(seq, mode="zlib"):
    """code lengths -> code-length symbols [(symbol, extra value)].  mode: plain (no repeats), zlib (runs of 0 as 17/18, runs of a length
    as the length then 16s, the longest repeats first), min (every repeat at its minimum count: 16 x3, 17 x3, 18 x11)"""
    out, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if mode == "plain":
            out += [(v, 0)] * run
        elif v == 0:
            while run >= 3:
                if mode == "min":
                    n = 11 if run >= 11 else 3
                else:
                    n = min(run, 138) if run >= 11 else min(run, 10)
                out.append((18, n - 11) if n >= 11 else (17, n - 3)); run -= n
            out += [(0, 0)] * run
        else:
            out.append((v, 0)); run -= 1
            while run >= 3:
                n = 3 if mode == "min" else min(run, 6)
                out.append((16, n - 3)); run -= n
            out += [(v, 0)] * run
        i = j
    return out


def _cl_expand(syms):
    """what a decoder reads from code-length symbols: the lengths, or None (a 16 first)"""
    out = []
    for s, v in syms:
        if s < 16:
            out.append(s)
        elif s == 16:
            if not out:
                return None
            out += [out[-1]] * (3 + v)
        else:
            out += [0] * ((3 if s == 17 else 11) + v)
    return out


class Deflate:
    """One raw DEFLATE stream, block after block."""
    def __init__(self):
        self.w = BitWriter()
        self.header_ok = True      # every dynamic header's code-length symbols describe HLIT + HDIST lengths exactly

    def stored(self, data, final=False, ln=None, nlen=None):
        self.w.put(int(final), 1); self.w.put(0, 2); self.w.align()
        ln = len(data) if ln is None else ln
        self.w.put(ln, 16); self.w.put((~ln & 0xFFFF) if nlen is None else nlen, 16)
        for b in data:
            self.w.put(b, 8)
        return self

    def fixed(self, tokens, final=False, eob=True):
        self.w.put(int(final), 1); self.w.put(1, 2)
        _put_tokens(self.w, tokens, canonical(FIXED_LIT), FIXED_LIT, canonical(FIXED_DIST), FIXED_DIST, eob)
        return self

    def btype3(self, final=True):
        self.w.put(int(final), 1); self.w.put(3, 2)
        return self

    def dynamic(self, tokens, lit_lens=None, dist_lens=None, final=False, hlit=None, hdist=None, hclen=None, cl_mode="zlib", cross=False,
                cl_syms=None, cl_lens=None, eob=True):
        """lit_lens / dist_lens: the codes (default: Huffman codes of the tokens' use, 15 bits at most).  hlit / hdist / hclen: the header's
        counts (default: as few as the lengths need; more = zeros written).  cl_mode: how the lengths are written (cl_symbols); cross: one
        run-length pass over literal AND distance lengths (runs cross from one into the other, as libdeflate writes them).  cl_syms: the
        code-length symbols as given (malformed headers); cl_lens: the code-length code as given."""
        lf, df = tokens_use(tokens)
        if lit_lens is None:
            lit_lens = huffman_lengths(lf[:286], 15)
        if dist_lens is None:
            dist_lens = huffman_lengths(df[:30], 15) if any(df) else [0]
        lit_lens, dist_lens = list(lit_lens), list(dist_lens)
        if hlit is None:
            hlit = max(257, max(i + 1 for i, ln in enumerate(lit_lens) if ln))
        if hdist is None:
            hdist = max([1] + [i + 1 for i, ln in enumerate(dist_lens) if ln])
        ll = (lit_lens + [0] * 288)[:hlit]
        dl = (dist_lens + [0] * 32)[:hdist]
        if cl_syms is None:
            cl_syms = cl_symbols(ll + dl, cl_mode) if cross else cl_symbols(ll, cl_mode) + cl_symbols(dl, cl_mode)
        if cl_lens is None:
            cf = [0] * 19
            for s, _ in cl_syms:
                cf[s] += 1
            cl_lens = huffman_lengths(cf, 7)
            if sum(1 for c in cl_lens if c) == 1:      # (one symbol: a second one so that the code is complete -- zlib wants that here)
                cl_lens[next(i for i in range(19) if not cl_lens[i])] = 1
        if hclen is None:
            hclen = max(4, max(CL_ORDER.index(i) + 1 for i in range(19) if cl_lens[i]))
        w = self.w
        w.put(int(final), 1); w.put(2, 2)
        w.put(hlit - 257, 5); w.put(hdist - 1, 5); w.put(hclen - 4, 4)
        for i in range(hclen):
            w.put(cl_lens[CL_ORDER[i]], 3)
        ccodes = canonical(cl_lens)
        for s, v in cl_syms:
            w.put_code(ccodes[s], cl_lens[s])
            if s >= 16:
                w.put(v, {16: 2, 17: 3, 18: 7}[s])
        lens = _cl_expand(cl_syms)
        ok = lens is not None and len(lens) == hlit + hdist
        self.header_ok = self.header_ok and ok
        if ok:      # (a malformed header's symbols are still written with the codes below)
            ll, dl = lens[:hlit], lens[hlit:]
        llens = (ll + [0] * 288)[:288]
        dlens = (dl + [0] * 32)[:32]
        _put_tokens(w, tokens, canonical(llens), llens, canonical(dlens), dlens, eob)
        return self

    def bits(self, value, n):
        self.w.put(value, n)
        return self

    @property
    def nbits(self):
        return self.w.nbits

    def getvalue(self):
        return self.w.getvalue()


def bgzf(payload, isize, crc, bad_isize=None, bad_crc=None):
    """one BGZF block (SAMv1 4.1) around a raw DEFLATE payload; isize / crc: of the bytes it inflates to; bad_*: values written instead"""
    bsize = len(payload) + 26
    assert bsize <= 65536, bsize
    return (b"\x1f\x8b\x08\x04" + b"\x00" * 4 + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize - 1)
            + payload + struct.pack("<II", crc if bad_crc is None else bad_crc, isize if bad_isize is None else bad_isize))


class Case:
    """payload: raw DEFLATE; data: what it inflates to (VALID / INCOMPLETE), or the size a decoder is asked for (MALFORMED: data may be
    bytes of that size, or None); bad_isize / bad_crc: a BGZF trailer that lies (the payload itself may be valid)"""
    def __init__(self, name, payload, data, verdict=VALID, bad_isize=None, bad_crc=None):
        self.name, self.payload, self.data, self.verdict = name, payload, data, verdict
        self.bad_isize, self.bad_crc = bad_isize, bad_crc

    @property
    def out_size(self):
        return len(self.data) if self.data is not None else 1000

    @property
    def fits_bgzf(self):
        return len(self.payload) + 26 <= 65536 and self.out_size <= 65536

    def block(self):
        d = self.data if self.data is not None else bytes(self.out_size)
        return bgzf(self.payload, len(d), zlib.crc32(d) & 0xFFFFFFFF, self.bad_isize, self.bad_crc)

    @property
    def refused_by_device(self):
        """what the kernels must refuse (a wrong CRC only when they check it)"""
        return self.verdict == MALFORMED

    def __repr__(self):
        return "Case(%s, %s, %d -> %d)" % (self.name, self.verdict, len(self.payload), self.out_size)


# ---- the corpus -------------------------------------------------------------------------------------------------------------------------
def _random_tokens(rng, lit_lens, dist_lens, n_min=0, limit=65_536):
    """tokens that use EVERY symbol of the two codes (literal bytes first until the longest distance has history, then the length symbols
    each with a distance symbol, round robin, random extra bits), at least n_min bytes of output, at most `limit`"""
    lits = [s for s in range(256) if lit_lens[s]]
    lsyms = [s for s in range(257, 286) if s < len(lit_lens) and lit_lens[s]]
    dsyms = [s for s in range(30) if s < len(dist_lens) and dist_lens[s]]
    need = max([DIST_BASE[s] + (1 << DIST_EXTRA[s]) - 1 for s in dsyms] + [0]) if lsyms else 0
    toks = []
    order = list(rng.permutation(lits))
    while len(toks) < max(need, len(lits), 1):
        toks.append(int(order[len(toks) % len(order)]))
    pos = len(toks)
    k = 0
    todo_d = list(dsyms)
    for s in (list(rng.permutation(lsyms)) + [None] * max(0, len(dsyms) - len(lsyms))) if lsyms and dsyms else []:
        if s is None:
            s = lsyms[k % len(lsyms)]
        ds = todo_d[k % len(todo_d)]
        k += 1
        le = LEN_EXTRA[s - 257]
        ln = LEN_BASE[s - 257] + int(rng.integers(0, 1 << le))
        de = DIST_EXTRA[ds]
        d = min(DIST_BASE[ds] + int(rng.integers(0, 1 << de)), pos)
        if pos + ln > limit:
            break
        toks.append(("M", ln, d)); pos += ln
    while pos < n_min:
        toks.append(int(lits[int(rng.integers(0, len(lits)))])); pos += 1
    return toks


def _case(name, stream, data, verdict=VALID, **kw):
    assert data is not None or verdict == MALFORMED, name
    assert stream.header_ok or verdict == MALFORMED, name
    return Case(name, stream.getvalue(), data, verdict, **kw)


def corpus_code_lengths(rng):
    out = []
    # every length 1..15 on both alphabets, 15-bit codes used (16 symbols each: lengths 1..14 and two of 15)
    for variant in range(3):
        lsyms = list(rng.choice(np.r_[np.arange(256), np.arange(257, 286)], 15, replace=False)) + [256]
        rng.shuffle(lsyms)
        ll = [0] * 286
        for i, s in enumerate(lsyms):
            ll[int(s)] = min(i + 1, 15)
        dsyms = list(rng.choice(30, 16, replace=False))
        if variant == 2:
            dsyms = list(range(29, 13, -1))                  # the far distances on the long codes
        dl = [0] * 30
        for i, s in enumerate(dsyms):
            dl[int(s)] = min(i + 1, 15)
        if not any(ll[s] for s in range(256)):
            continue
        toks = _random_tokens(rng, ll, dl)
        d = expand(toks)
        out.append(_case("lengths_1_to_15_v%d" % variant, Deflate().dynamic(toks, ll, dl, final=True, cross=variant == 1), d))
    # a 1-bit literal code
    ll = complete_lengths(286, {ord("A"): 1}, symbols=[ord("A"), 256] + list(range(257, 286)) + [ord("b"), ord("c")])
    dl = complete_lengths(30)
    toks = _random_tokens(rng, ll, dl)
    out.append(_case("one_bit_literal", Deflate().dynamic(toks, ll, dl, final=True), expand(toks)))
    # all 286 + 30 symbols in one code
    ll = complete_lengths(286)
    dl = complete_lengths(30)
    toks = _random_tokens(rng, ll, dl, limit=65_536)
    out.append(_case("all_286_and_30_symbols", Deflate().dynamic(toks, ll, dl, final=True, hclen=19), expand(toks)))
    # the longest match: a 15-bit length symbol 284 + 5 extra bits + a 15-bit distance symbol 29 + 13 extra bits = 48 bits
    ll, dl = geometry_code()
    w = Deflate()
    toks = [ord("A")] * 32768 + [("S", 284, 31, 5), ("D", 29, 8191, 13), ("S", 284, 0, 5), ("D", 29, 0, 13)]
    w.dynamic(toks, ll, dl, final=True)
    out.append(_case("longest_match_48_bits", w, expand(toks)))
    return out


def geometry_code():
    """literal 'A' a 1-bit code; 'B' 2 bits; EOB 14 bits; length symbols 284 / 285 and distance symbol 29 of 15 bits (the 48-bit match)"""
    ll = [0] * 286
    order = [ord("A"), ord("B"), ord("C"), ord("D"), ord("E"), ord("F"), ord("G"), ord("H"), 257, 258, 265, 270, ord("I"), 256, 284, 285]
    for i, s in enumerate(order):
        ll[s] = min(i + 1, 15)
    dl = [0] * 30
    for i, s in enumerate([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 20, 24, 28, 29, 26]):
        dl[s] = min(i + 1, 15)
    assert kraft(ll) == 32768 and kraft(dl) == 32768
    return ll, dl


def corpus_degenerate(rng):
    out = []
    # one distance code of length 1 (libdeflate)
    ll = complete_lengths(286, symbols=list(range(0, 256, 3)) + [256, 260, 270, 285])
    dl = [0] * 30; dl[int(rng.integers(0, 30))] = 1
    ds = dl.index(1)
    toks = [int(x) for x in rng.choice(list(range(0, 256, 3)), DIST_BASE[ds] + (1 << DIST_EXTRA[ds]))]
    for _ in range(50):
        toks.append(("M", int(rng.choice([6, 258, 24])), DIST_BASE[ds] + int(rng.integers(0, 1 << DIST_EXTRA[ds])))); toks.append(0)
    out.append(_case("single_distance_code", Deflate().dynamic(toks, ll, dl, final=True), expand(toks)))
    dl2 = [0] * 30; dl2[0] = 1      # distance 1 only: runs
    toks = [6] + [("M", 258, 1), 9] * 40
    out.append(_case("single_distance_code_d1", Deflate().dynamic(toks, ll, dl2, final=True), expand(toks)))
    # HDIST = 1 with length 0: a literal-only block
    toks = [int(x) for x in rng.choice(list(range(0, 256, 3)), 3000)]
    out.append(_case("no_distance_code", Deflate().dynamic(toks, ll, [0], final=True, hdist=1), expand(toks)))
    # a literal/length code of end-of-block only (an empty dynamic block) between blocks with data
    eob_only = [0] * 257; eob_only[256] = 1
    a, b = bytes(rng.integers(0, 256, 700, dtype=np.uint8)), bytes(rng.integers(0, 256, 900, dtype=np.uint8))
    w = Deflate().dynamic(list(a)).dynamic([], eob_only, [0]).dynamic([], eob_only, [0], hdist=30, hlit=286).dynamic(list(b), final=True)
    out.append(_case("eob_only_blocks_between_data", w, a + b))
    w = Deflate().dynamic([], eob_only, [1]).stored(b"").dynamic([], eob_only, [0], final=True)
    out.append(_case("eob_only_blocks_nothing_else", w, b""))
    return out




def _cl_sequence(after_18):
    """code-length symbols with every repeat form zlib never writes, HLIT 286 / HDIST 30 (both codes complete):
    literals 0..167 zero (18 at 138 and 11, 17 at 10 and 3, a 16 right after a 17 -- or after an 18 -- repeating the zero), 168..177 six bits,
    178..285 seven bits with the last run a 16 that crosses into the distance lengths (284, 285, d0, d1); distances 0..3 seven bits, 4..5
    six, 6..23 five, 24..29 four (16 at 3 and 6)"""
    if after_18:
        syms = [(18, 127), (16, 0), (17, 7), (18, 5), (0, 0)]                               # 138 + 3 + 10 + 16 + 1 = 168
    else:
        syms = [(18, 127), (18, 0), (17, 7), (17, 0), (16, 0), (16, 0)]                     # 138 + 11 + 10 + 3 + 3 + 3 = 168
    syms += [(6, 0), (16, 3), (16, 0)]                                                      # 10 x 6
    syms += [(7, 0)] + [(16, 3)] * 17 + [(7, 0)] * 3 + [(16, 1)]                            # 103 + 3 + 4 (crossing): 108 literal + 2 distance
    syms += [(7, 0), (7, 0), (6, 0), (6, 0), (5, 0), (16, 3), (16, 3), (16, 2), (4, 0), (16, 2)]
    lens = _cl_expand(syms)
    assert len(lens) == 316, len(lens)
    ll, dl = lens[:286], lens[286:]
    assert kraft(ll) == 32768 and kraft(dl) == 32768 and dl[:2] == [7, 7] and ll[284:] == [7, 7]
    return syms, ll, dl


def corpus_code_length_code(rng):
    out = []
    data = rng.choice(np.frombuffer(b"ACGTN\n", np.uint8), 5000).tobytes()
    toks = list(data[:40]) + [("M", 40, 40)] + list(data[80:]) + [("M", 258, 1), ("M", 3, 5000)]
    want = expand(toks)
    lf, df = tokens_use(toks)
    ll, dl = huffman_lengths(lf[:286], 15), huffman_lengths(df[:30], 15)
    for mode in ("plain", "zlib", "min"):
        for cross in (False, True):
            for hclen in (None, 19):
                w = Deflate().dynamic(toks, ll, dl, final=True, hclen=hclen, cl_mode=mode, cross=cross, hlit=286 if cross else None)
                out.append(_case("cl_%s_%s_hclen%s" % (mode, "cross" if cross else "split", hclen), w, want))
    # HCLEN 5 (16, 17, 18, 0, 8): a literal-only code of 256 codes of 8 bits, HDIST 1 with length 0
    ll8 = [8] * 255 + [0, 8]
    toks8 = [int(x) for x in rng.integers(0, 255, 3000)]
    out.append(_case("hclen_5", Deflate().dynamic(toks8, ll8, [0], final=True, hdist=1, hclen=5), bytes(toks8)))
    for after_18 in (False, True):
        syms, ll, dl = _cl_sequence(after_18)
        toks = _random_tokens(rng, ll, dl)
        out.append(_case("cl_repeat_forms_%s" % ("after_18" if after_18 else "after_17"),
                         Deflate().dynamic(toks, ll, dl, final=True, hlit=286, hdist=30, cl_syms=syms), expand(toks)))
    return out


def _small_block(rng, w, final=False):
    """a small dynamic block of a code of its own (random alphabet, random lengths); -> the bytes it adds"""
    alpha = [int(x) for x in rng.choice(256, int(rng.integers(2, 40)), replace=False)]
    lsyms = alpha + [256] + [int(x) for x in rng.choice(np.arange(257, 286), int(rng.integers(0, 6)), replace=False)]
    ll = complete_lengths(286, symbols=[int(s) for s in rng.permutation(lsyms)])
    dl = complete_lengths(30, symbols=[int(x) for x in rng.choice(10, int(rng.integers(1, 6)), replace=False)]) if len(lsyms) > len(alpha) + 1 else [0]
    toks = [alpha[int(i)] for i in rng.integers(0, len(alpha), int(rng.integers(30, 90)))]
    pos = len(toks)
    for s in range(257, 286):
        if ll[s]:
            ds = next(d for d in range(30) if d < len(dl) and dl[d])
            toks.append(("S", s, 0, LEN_EXTRA[s - 257])); toks.append(("D", ds, 0, DIST_EXTRA[ds]))
            toks.append(alpha[0])
    w.dynamic(toks, ll, dl, final=final)
    return toks


def corpus_blocks(rng):
    out = []
    # hundreds of small dynamic blocks in one BGZF block, each with a code of its own
    for n_blocks in (120, 250):
        w, toks = Deflate(), []
        for k in range(n_blocks):
            toks += _small_block(rng, w, final=k == n_blocks - 1)
        out.append(_case("dynamic_blocks_%d" % n_blocks, w, expand(toks)))
    # empty stored blocks; stored blocks of 65 535 bytes (raw streams: no BGZF block holds one) and the largest a BGZF block holds
    big = bytes(rng.integers(0, 256, 65_535, dtype=np.uint8))
    out.append(_case("stored_empty", Deflate().stored(b"").stored(b"").fixed([1, 2, 3]).stored(b"", final=True), b"\x01\x02\x03"))
    out.append(_case("stored_65535", Deflate().stored(big, final=True), big))
    out.append(_case("stored_65535_behind_a_literal", Deflate().fixed([7]).stored(big).stored(b"", final=True), b"\x07" + big))
    out.append(_case("stored_65505", Deflate().stored(big[:65_505], final=True), big[:65_505]))
    # ISIZE = 65 536
    for variant in range(3):
        d = bytes(rng.integers(0, 256, 1000, dtype=np.uint8))
        if variant == 0:
            toks = list(d) + [("M", 258, 1000)] * 250 + [("M", 36, 1000)]
            w = Deflate().dynamic(toks, final=True)
        elif variant == 1:
            toks = list(d[:31]) + [("M", 258, 31)] * 253 + [("M", 231, 1)]
            w = Deflate().fixed(toks[:100]).stored(b"").dynamic(toks[100:], final=True)
        else:
            dd = rng.choice(np.frombuffer(b"ACGT", np.uint8), 65_536).tobytes()
            toks = list(dd)
            w = Deflate().dynamic(toks[:30_000]).stored(b"").dynamic(toks[30_000:], final=True)
        want = expand(toks)
        assert len(want) == 65_536, len(want)
        out.append(_case("isize_65536_v%d" % variant, w, want))
    # 63, 64 and 65 literals waiting in front of a stored block, a match, end-of-block
    for n in (63, 64, 65, 127, 128, 129):
        lits = [int(x) for x in rng.integers(0, 256, n)]
        tail = bytes(rng.integers(0, 256, 77, dtype=np.uint8))
        out.append(_case("lits_%d_then_stored" % n, Deflate().dynamic(lits).stored(tail, final=True), bytes(lits) + tail))
        toks = lits + [("M", 40, n)] + lits[:5]
        out.append(_case("lits_%d_then_match" % n, Deflate().dynamic(toks, final=True), expand(toks)))
        out.append(_case("lits_%d_then_eob_then_fixed" % n, Deflate().dynamic(lits).fixed([("M", 10, n - 3) if n > 3 else 1], final=True),
                         expand(lits + [("M", 10, n - 3)])))
    # a final end-of-block whose last bit is the last bit of the payload (1-bit literals as padding to a whole byte)
    ll, dl = geometry_code()
    for pad in range(8):
        w = Deflate()
        toks = [ord("A")] * pad
        w.dynamic(toks, ll, dl, final=True)
        if w.nbits % 8 == 0:
            out.append(_case("eob_last_bit_of_payload", w, expand(toks)))
    return out


def corpus_geometry(rng):
    """the parallel kernel's chunks (512 bits of the block body) and spans (64 chunks): 1-bit literals as padding put the 48-bit match, the
    end-of-block symbol and a length's extra bits across a chunk boundary and across the span boundary at every offset 0..63.  (Empty fixed
    blocks in front shift the body against the input's words.)"""
    ll, dl = geometry_code()
    A = ord("A")
    out = []
    # the 48-bit match ending on the far side of a chunk boundary at every offset: one block per 16 offsets, every match at the next boundary
    for shift in range(4):
        for k0 in range(0, 64, 16):
            w = Deflate()
            for _ in range(shift):
                w.fixed([])
            body0 = None
            toks = [A] * 32_768
            pos_bits = 32_768
            for k in range(k0, k0 + 16):
                boundary = (pos_bits // 512 + 1) * 512
                pad = boundary - k - pos_bits
                toks += [A] * pad
                toks += [("S", 284, 31, 5), ("D", 29, 8191 - k, 13)]
                pos_bits = boundary - k + 48
            toks += [A] * 3
            w.dynamic(toks, ll, dl, final=True)
            out.append(_case("match48_chunks_shift%d_k%d" % (shift, k0), w, expand(toks)))
    # ... and across the span boundary (bit 32 768 of the body), at every offset; a second span behind it
    for k in range(64):
        w = Deflate()
        toks = [A] * (32_768 - k) + [("S", 284, k % 32, 5), ("D", 29, 8191 - k, 13), ord("B"), ("M", 258, 1)] + [A] * 40
        w.dynamic(toks, ll, dl, final=True)
        out.append(_case("match48_span_k%d" % k, w, expand(toks)))
    # the end-of-block symbol (14 bits) across a chunk / the span boundary, as lane 63's last symbol, as a span's first symbol; a block body of
    # exactly one span; the next block behind it
    for k in list(range(0, 20)) + [31, 32, 33, 63]:
        for at in (512 * 7, 32_768):
            w = Deflate()
            toks = [A] * (at - k)
            w.dynamic(toks, ll, dl)
            w.fixed([ord("z"), ("M", 5, 1)], final=True)
            out.append(_case("eob_at_%d_minus_%d" % (at, k), w, expand(toks + [ord("z"), ("M", 5, 1)])))
    eob_len = ll[256]
    w = Deflate()
    toks = [A] * (32_768 - eob_len)
    w.dynamic(toks, ll, dl).dynamic(toks[:100], ll, dl, final=True)
    out.append(_case("body_of_exactly_one_span", w, expand(toks + toks[:100])))
    # length extra bits across a boundary: symbol 270 (2 extra bits) and 265 (1) at every offset of a chunk's last bits
    toks = [A] * 2000
    pos_bits = 2000
    for k in range(20):
        boundary = (pos_bits // 512 + 1) * 512
        toks += [A] * (boundary - k - pos_bits)
        toks += [("S", 270, k % 4, 2), ("D", 0, 0, 0), ("S", 265, k % 2, 1), ("D", 1, 0, 0)]
        pos_bits = boundary - k + ll[270] + 2 + dl[0] + ll[265] + 1 + dl[1]
    out.append(_case("length_extra_bits_across_chunks", Deflate().dynamic(toks, ll, dl, final=True), expand(toks)))
    return out


def corpus_matches(rng):
    out = []
    hist = bytes(rng.integers(0, 256, 33_000, dtype=np.uint8))
    # length 258 as 285 and as 284 + 31; distance 32 768 with length 258; overlapping chains; matches to the block's first byte
    toks = list(hist) + [("S", 285, 0, 0), ("D", 29, 8191, 13), ("S", 284, 31, 5), ("D", 29, 8191, 13), ("M", 258, 32_768), ("M", 258, 32_767)]
    out.append(_case("len258_both_forms_dist32768", Deflate().dynamic(toks, final=True), expand(toks)))
    toks = list(hist[:5]) + [("M", 258, d) for d in (1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 100, 257)] + [("M", 3, 1), ("M", 4, 3), ("M", 10, 9)]
    out.append(_case("overlapping_chains", Deflate().dynamic(toks, final=True), expand(toks)))
    toks, pos = [9, 8, 7], 3
    for k in range(300):                            # every match reaches back to the block's first byte (distance == position)
        ln = 3 + (k * 37) % 256
        if pos + ln > 32_768:
            break
        toks.append(("M", ln, pos)); pos += ln
    out.append(_case("match_to_first_byte", Deflate().fixed(toks, final=True), expand(toks)))
    # distances swept at destinations that make the window of phase (D) slide: a literal history, then long runs of matches (many matches per
    # span, so that a batch spans the window) at distances inside, in front of and across the window's start
    sweeps = [list(range(1000, 1051)), list(range(4080, 4111)), [8191, 8192, 8193, 16_384, 32_767, 32_768]]
    for si, ds in enumerate(sweeps):
        for lens_kind in ("long", "mixed"):
            toks = list(hist[:32_800])
            pos = 32_800
            k = 0
            while pos < 65_000:
                d = ds[k % len(ds)]
                ln = 258 if lens_kind == "long" else int(rng.choice([3, 4, 9, 31, 100, 258, 200]))
                ln = min(ln, 65_536 - pos)
                if ln < 3:
                    break
                toks.append(("M", ln, d)); pos += ln; k += 1
                if lens_kind == "mixed" and k % 5 == 0 and pos < 65_536:
                    toks.append(int(rng.integers(0, 256))); pos += 1
            out.append(_case("dist_sweep_%d_%s" % (si, lens_kind), Deflate().dynamic(toks, final=True), expand(toks)))
    return out


def corpus_malformed(rng):
    """streams every decoder must refuse (zlib does)"""
    out = []
    M = MALFORMED
    d = bytes(rng.integers(0, 256, 500, dtype=np.uint8))
    for s in (286, 287):
        toks = list(d[:50]) + [("S", s, 0, 0), ("D", 0, 0, 0)] + list(d[50:])
        out.append(_case("fixed_litlen_%d" % s, Deflate().fixed(toks, final=True), d + b"\0" * 3, M))
    for s in (30, 31):
        toks = list(d[:50]) + [("S", 260, 0, 0), ("D", s, 0, 0)] + list(d[50:])
        out.append(_case("fixed_dist_%d" % s, Deflate().fixed(toks, final=True), d + b"\0" * 6, M))
    toks = list(d[:50]) + [("M", 10, 51)] + list(d[50:])
    out.append(_case("distance_before_first_byte", Deflate().fixed(toks, final=True), d + bytes(10), M))
    out.append(_case("distance_at_position_0", Deflate().fixed([("M", 3, 1)] + list(d), final=True), d + bytes(3), M))
    toks = list(d)
    for hlit, hdist in ((287, 30), (288, 30), (286, 31), (286, 32)):
        ll = complete_lengths(286, symbols=list(range(256)) + [256, 257])
        ll = ll + [0] * 2
        dl = [1, 1] + [0] * 30
        cs = cl_symbols((ll + [0] * 288)[:hlit], "plain") + cl_symbols((dl + [0] * 32)[:hdist], "plain")
        out.append(_case("hlit%d_hdist%d" % (hlit, hdist), Deflate().dynamic(toks, ll, dl, final=True, hlit=hlit, hdist=hdist, cl_syms=cs), d, M))
    # over-subscribed literal/length, distance and code-length codes
    ll = complete_lengths(286, symbols=list(range(256)) + [256, 257])
    ll_over = list(ll); ll_over[258] = 15
    out.append(_case("oversubscribed_litlen", Deflate().dynamic(toks, ll_over, [1, 1], final=True), d, M))
    out.append(_case("oversubscribed_dist", Deflate().dynamic(toks, ll, [1, 1, 1], final=True), d, M))
    dl_over = complete_lengths(30, symbols=range(29))
    dl_over[29] = 15                                       # (one 15-bit code too many)
    assert kraft(dl_over) > 32768
    out.append(_case("oversubscribed_dist_by_one_15_bit_code", Deflate().dynamic(toks, ll, dl_over, final=True), d, M))
    cf = [0] * 19
    for s, _ in cl_symbols(ll + [1, 1], "zlib"):
        cf[s] += 1
    cll = huffman_lengths(cf, 7)
    cll_over = list(cll); cll_over[next(i for i in range(19) if not cll[i])] = 1
    out.append(_case("oversubscribed_codelength", Deflate().dynamic(toks, ll, [1, 1], final=True, cl_lens=cll_over, hclen=19), d, M))
    # 16 as the first code-length symbol; a repeat past HLIT + HDIST; no end-of-block length
    cs = cl_symbols(ll, "zlib") + cl_symbols([1, 1], "zlib")
    out.append(_case("sixteen_first", Deflate().dynamic(toks, ll, [1, 1], final=True, hlit=286, hdist=2, cl_syms=[(16, 0)] + cs[1:]), d, M))
    out.append(_case("repeat_past_end", Deflate().dynamic(toks, ll, [1, 1], final=True, hlit=286, hdist=2, cl_syms=cs[:-2] + [(1, 0), (16, 3)]), d, M))
    out.append(_case("zero_run_past_end", Deflate().dynamic(toks, ll, [1, 1], final=True, hlit=286, hdist=2, cl_syms=cs[:-2] + [(18, 20)]), d, M))
    ll_no_eob = complete_lengths(286, symbols=list(range(256)) + [257, 258])
    out.append(_case("no_eob_length", Deflate().dynamic(toks, ll_no_eob, [1, 1], final=True, eob=False), d, M))
    # a stream that reaches a bit pattern outside an incomplete code: the single distance code (zlib takes the header) and a wider one
    ll2 = complete_lengths(286, symbols=list(range(256)) + [256, 260])
    out.append(_case("single_dist_code_other_pattern", _flip_last_dist_bit(d, ll2), d[:100] + bytes(6), M))
    ll_inc = list(ll); ll_inc[257] = 0                      # one 15-bit... an unused pattern at the top of the literal/length code
    out.append(_case("unused_litlen_pattern_reached", _reach_unused(d, ll_inc), d, M))
    # BTYPE 3; LEN / NLEN that disagree; a truncated payload; a wrong ISIZE
    out.append(_case("btype3", Deflate().fixed(list(d[:10])).btype3(), d[:10] + bytes(5), M))
    out.append(_case("stored_nlen", Deflate().stored(d, final=True, nlen=(~len(d) & 0xFFFF) ^ 0x100), d, M))
    full = Deflate().dynamic(list(d) * 4, final=True).getvalue()
    for cut in (1, 2, len(full) // 2):
        out.append(Case("truncated_%d" % cut, full[:-cut], d * 4, M))
    out.append(Case("stored_truncated", Deflate().stored(d, final=True).getvalue()[:-3], d, M))
    out.append(Case("wrong_isize_short", Deflate().fixed(list(d), final=True).getvalue(), d[:-1], M))
    out.append(Case("wrong_isize_long", Deflate().fixed(list(d), final=True).getvalue(), d + b"\0", M))
    out.append(Case("no_final_block", Deflate().fixed(list(d)).getvalue(), d, M))
    return [c for c in out if c is not None]


def _flip_last_dist_bit(d, ll2):
    """a single distance code (symbol 5, code '0'), and the stream's distance bit '1': a pattern the code does not have"""
    dl = [0] * 5 + [1]
    lc = canonical(ll2 + [0, 0])
    hdr = Deflate().dynamic([], ll2, dl, final=True)      # the header (and an EOB): its bits up to the EOB, then the body by hand
    n_hdr = hdr.nbits - ll2[256]
    w = Deflate()
    w.w.put(int.from_bytes(hdr.getvalue(), "little") & ((1 << n_hdr) - 1), n_hdr)
    for b in d[:100]:
        w.w.put_code(lc[b], ll2[b])
    w.w.put_code(lc[260], ll2[260])
    w.w.put(1, 1); w.w.put(0, 1)
    w.w.put_code(lc[256], ll2[256])
    return w


def _reach_unused(d, ll_inc):
    """an incomplete literal/length code and a stream that reaches one of its unused patterns (all ones: the top of a canonical code)"""
    w = Deflate()
    lc = canonical(ll_inc + [0, 0])
    hdr = Deflate().dynamic([], ll_inc, [1, 1], final=True)
    n_hdr = hdr.nbits - ll_inc[256]
    v = int.from_bytes(hdr.getvalue(), "little")
    w.w.put(v & ((1 << n_hdr) - 1), n_hdr)
    for b in d[:100]:
        w.w.put_code(lc[b], ll_inc[b])
    w.w.put((1 << 15) - 1, 15)
    w.w.put_code(lc[256], ll_inc[256])
    return w


def corpus_incomplete(rng):
    """incomplete codes whose unused patterns the stream never reaches: zlib refuses the header (it takes an incomplete code only when it is a
    single code of one bit); the project's decoders check for over-subscription only and decode such streams -- the policy the tests pin"""
    out = []
    d = bytes(rng.integers(0, 256, 3000, dtype=np.uint8))
    lit_syms = sorted(set(d))
    ll = complete_lengths(286, symbols=lit_syms + [256, 258, 270])
    inc = list(ll); inc[270] = 0                                  # one code missing: incomplete literal/length code
    toks = list(d) + [("M", 4, 100)]
    out.append(_case("incomplete_litlen", Deflate().dynamic(toks, inc, [0] * 13 + [1, 1], final=True), expand(toks), INCOMPLETE))
    out.append(_case("incomplete_dist", Deflate().dynamic(toks, ll, [0] * 13 + [2, 2, 2], final=True), expand(toks), INCOMPLETE))
    out.append(_case("incomplete_dist_single_2bit", Deflate().dynamic(toks, ll, [0] * 13 + [2], final=True), expand(toks), INCOMPLETE))
    cf = [0] * 19
    cs = cl_symbols(ll + [1, 1], "plain")
    for s, _ in cs:
        cf[s] += 1
    cll = huffman_lengths(cf, 7)
    cll_inc = [c + 1 if c else 0 for c in cll]                     # every code-length code one bit longer: half the patterns unused
    assert max(cll_inc) <= 7
    out.append(_case("incomplete_codelength", Deflate().dynamic(toks[:-1], ll, [1, 1], final=True, hlit=286, hdist=2, cl_syms=cs, cl_lens=cll_inc, hclen=19),
                     expand(toks[:-1]), INCOMPLETE))
    return out


_CORPUS = {}


def corpus(seed=1):
    """every case, in a fixed order (made once per process: ~10 s of pure Python)"""
    if seed not in _CORPUS:
        _CORPUS[seed] = _make_corpus(seed)
    return _CORPUS[seed]


def _make_corpus(seed):
    rng = np.random.default_rng(seed)
    out = []
    for part in (corpus_code_lengths, corpus_degenerate, corpus_code_length_code, corpus_blocks, corpus_geometry, corpus_matches,
                 corpus_malformed, corpus_incomplete):
        out += part(rng)
    names = [c.name for c in out]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return out


# ---- libdeflate (the encoder behind htslib's BGZF), when a shared library of it is on the machine -------------------------------------
class LibDeflate:
    def __init__(self, path):
        import ctypes as C
        self.path = path
        L = C.CDLL(path)
        L.libdeflate_alloc_compressor.restype = C.c_void_p
        L.libdeflate_alloc_compressor.argtypes = [C.c_int]
        L.libdeflate_deflate_compress.restype = C.c_size_t
        L.libdeflate_deflate_compress.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t]
        L.libdeflate_free_compressor.argtypes = [C.c_void_p]
        self.L, self.C = L, C

    def compress(self, data, level):
        """raw DEFLATE of data at libdeflate's level 1..12"""
        c = self.L.libdeflate_alloc_compressor(level)
        assert c, level
        try:
            buf = self.C.create_string_buffer(len(data) + len(data) // 8 + 1024)
            n = self.L.libdeflate_deflate_compress(c, data, len(data), buf, len(buf))
            assert n, "libdeflate: no room"
            return buf.raw[:n]
        finally:
            self.L.libdeflate_free_compressor(c)


def libdeflate(path=None):
    """LibDeflate over the machine's shared library (ctypes), or None when there is none"""
    import ctypes.util
    path = path or ctypes.util.find_library("deflate")
    if not path:
        return None
    try:
        return LibDeflate(path)
    except (OSError, AttributeError):
        return None


LIBDEFLATE_LEVELS = (1, 6, 9, 12)


def libdeflate_samples(rng, size=None):
    """(level, data) pairs: the GPU suite's kinds() at every libdeflate level of LIBDEFLATE_LEVELS, plus BAM-like records (size: bytes kept of
    each kind, None = all)"""
    import test_gpu_bgzf as tg
    import bam_writer as bw
    data = tg.kinds(rng)
    recs = b"".join(bw.record(int(rng.integers(0, 8)), int(rng.integers(0, 1 << 27)), "A00123:8:H7:%d:%d" % (i % 4, i), flag=int(rng.choice([0, 16, 256])),
                              seq="".join(rng.choice(list("ACGTN"), 91)), qual=bytes(int(q) for q in rng.choice([2, 12, 23, 37], 91)),
                              tags=[("CB", "Z", "".join(rng.choice(list("ACGT"), 16)) + "-1"), ("UB", "Z", "".join(rng.choice(list("ACGT"), 12))),
                                    ("GX", "Z", "ENSG%011d" % int(rng.integers(0, 30000))), ("xf", "i", int(rng.integers(0, 30)))]) for i in range(300))
    data["bam_records"] = recs[:65_000]
    out = []
    for level in LIBDEFLATE_LEVELS:
        for name, d in data.items():
            out.append((level, d if size is None or name == "bam_records" else d[:size]))
    return out


# ---- a libdeflate-like BGZF compressor for whole files (tests/bam_writer.write_bam's `compress`) ------------------------------------
def lz77(data, min_len=4):
    """greedy LZ77 tokens of data (4-byte hash of the last position, matches up to 258 bytes and 32 768 back)"""
    last, toks, i, n = {}, [], 0, len(data)
    mv = memoryview(data)
    while i < n:
        key = bytes(mv[i:i + 4]) if i + 4 <= n else None
        j = last.get(key) if key is not None else None
        if key is not None:
            last[key] = i
        if j is not None and i - j <= 32_768:
            ln = 4
            while ln < 258 and i + ln < n and data[j + ln] == data[i + ln]:
                ln += 1
            if ln >= min_len:
                toks.append(("M", ln, i - j)); i += ln
                continue
        toks.append(data[i]); i += 1
    return toks


def libdeflate_like(seed):
    """data -> one BGZF block in forms libdeflate writes and zlib does not: many dynamic blocks per BGZF block (a code each), every fourth
    one with its matches cut to a single distance symbol (a single distance code of one bit), every fourth literal-only with HDIST 1 and
    length 0, code-length runs across the literal / distance boundary, an empty stored block now and then"""
    rng = np.random.default_rng(seed)

    def compress(data):
        toks, pos, at = lz77(data), 0, []
        for t in toks:
            at.append(pos)
            pos += 1 if isinstance(t, int) else t[1]
        w, k, piece = Deflate(), 0, 0
        while True:
            n = int(rng.integers(40, 600))
            lo, k = k, min(k + n, len(toks))
            part = toks[lo:k]
            final = k >= len(toks)
            kind = piece % 4
            if kind in (1, 3):
                ds = [dist_symbol(t[2])[0] for t in part if not isinstance(t, int)]
                keep = max(set(ds), key=ds.count) if ds and kind == 1 else None
                new = []
                for j, t in enumerate(part):
                    if isinstance(t, int) or dist_symbol(t[2])[0] == keep:
                        new.append(t)
                    else:            # the match's bytes as literals
                        new += list(data[at[lo + j]:at[lo + j] + t[1]])
                part = new
            w.dynamic(part, final=final, cross=piece % 2 == 0, hdist=1 if kind == 3 else None)
            if piece % 9 == 5 and not final:
                w.stored(b"")
            piece += 1
            if final:
                break
        return bgzf(w.getvalue(), len(data), zlib.crc32(data) & 0xFFFFFFFF)
    return compress
