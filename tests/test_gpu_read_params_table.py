"""The read-parameter table of -r alone, through its C-ABI (include/dropest_bgzf.h: dropest_read_params_*): every row as the device validated,
packed and hashed it, the canonical row of every name, and look-ups, against the plain model (read_params_model.py)."""
import ctypes as C

import numpy as np
import pytest

from dropest_amd import capi

import read_params_model as m

pytestmark = pytest.mark.gpu
P = C.POINTER


class Row(C.Structure):
    _fields_ = [("hash", C.c_uint64), ("cb_code", C.c_uint64), ("umi_code", C.c_uint64), ("name_off", C.c_uint64), ("cb_off", C.c_uint64), ("umi_off", C.c_uint64),
                ("quality_off", C.c_uint64), ("name_len", C.c_uint32), ("cb_len", C.c_uint32), ("umi_len", C.c_uint32), ("quality_len", C.c_uint32),
                ("canonical", C.c_uint32), ("valid", C.c_uint8), ("pass_", C.c_uint8), ("empty", C.c_uint8), ("pad", C.c_uint8)]


def fnv1a(s):
    h = 1469598103934665603
    for c in s:
        h = ((h ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def slot_of(h, mask):
    return ((((h ^ (h >> 29)) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF) >> 40) & mask


def lib():
    L = capi.lib()
    L.dropest_bgzf_last_error.restype = C.c_char_p
    L.dropest_read_params_create.argtypes = [C.c_int, C.c_int, P(C.c_void_p)]
    L.dropest_read_params_add_text.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int]
    L.dropest_read_params_build.argtypes = [C.c_void_p]
    L.dropest_read_params_counts.argtypes = [C.c_void_p] + [P(C.c_uint64)] * 4
    L.dropest_read_params_rows_to_host.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    L.dropest_read_params_lookup.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.dropest_read_params_claims_to_host.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    L.dropest_read_params_reset_claims.argtypes = [C.c_void_p]
    L.dropest_read_params_destroy.argtypes = [C.c_void_p]
    L.dropest_read_params_destroy.restype = None
    return L


class Table:
    """texts: one bytes object per _add_text call."""

    def __init__(self, L, texts, min_phred=0, hash_bits=0):
        self.L, self.h = L, C.c_void_p()
        assert L.dropest_read_params_create(0, hash_bits, C.byref(self.h)) == 0, L.dropest_bgzf_last_error()
        mps = min_phred if isinstance(min_phred, (list, tuple)) else [min_phred] * len(texts)
        for text, mp in zip(texts, mps):
            offs = np.array(m.split_lines(text)[1], np.uint64)
            buf = np.frombuffer(text, np.uint8) if text else np.zeros(1, np.uint8)
            assert L.dropest_read_params_add_text(self.h, buf.ctypes.data, len(text), offs.ctypes.data if len(offs) else None, len(offs), mp) == 0, L.dropest_bgzf_last_error()
        assert L.dropest_read_params_build(self.h) == 0, L.dropest_bgzf_last_error()
        self.text = b"".join(texts)

    def counts(self):
        v = [C.c_uint64() for _ in range(4)]
        assert self.L.dropest_read_params_counts(self.h, *[C.byref(x) for x in v]) == 0
        return dict(zip(("rows", "valid", "malformed", "repeated"), (int(x.value) for x in v)))

    def rows(self):
        n = self.counts()["rows"]
        out = (Row * max(n, 1))()
        assert self.L.dropest_read_params_rows_to_host(self.h, 0, n, out) == 0, self.L.dropest_bgzf_last_error()
        return list(out)[:n]

    def lookup(self, names):
        off = np.zeros(len(names) + 1, np.uint64)
        off[1:] = np.cumsum([len(x) for x in names])
        pool = np.frombuffer(b"".join(names) + b"\0", np.uint8)
        out = np.zeros(max(len(names), 1), np.uint32)
        assert self.L.dropest_read_params_lookup(self.h, pool.ctypes.data, off.ctypes.data, len(names), out.ctypes.data) == 0, self.L.dropest_bgzf_last_error()
        return out[:len(names)].tolist()

    def close(self):
        self.L.dropest_read_params_destroy(self.h)


def check(L, texts, min_phred=0, hash_bits=0, absent=()):
    """Every row and every look-up of a table over `texts` against the model; returns (table rows, model)."""
    t = Table(L, texts, min_phred, hash_bits)
    want = m.Rows(texts, min_phred)
    assert t.counts() == want.counts()
    got = t.rows()
    assert len(got) == len(want.rows)
    text = t.text
    mask = (1 << hash_bits) - 1 if 0 < hash_bits < 64 else (1 << 64) - 1
    for k, (g, w) in enumerate(zip(got, want.rows)):
        if not isinstance(w, dict):
            assert (g.valid, g.empty, g.canonical) == (0, 1 if w is None else 0, m.NONE), k
            continue
        assert (g.valid, g.empty, g.pass_, g.canonical) == (1, 0, int(w["ok"]), w["canonical"]), k
        assert text[g.name_off:g.name_off + g.name_len] == w["name"] and text[g.cb_off:g.cb_off + g.cb_len] == w["cb"], k
        assert text[g.umi_off:g.umi_off + g.umi_len] == w["umi"] and text[g.quality_off:g.quality_off + g.quality_len] == w["quality"], k
        assert (g.cb_code, g.umi_code, g.hash) == (m.pack(w["cb"]), m.pack(w["umi"]), fnv1a(w["name"]) & mask), k
    names = sorted(want.first)
    asked = names + [b"@" + x for x in names] + list(absent)
    assert t.lookup(asked) == [want.lookup(x) for x in asked]
    t.close()
    return got, want


def _row(rng, name, n_cb=12, n_umi=8):
    cb = bytes(rng.choice(list(b"ACGT"), n_cb).tolist()); umi = bytes(rng.choice(list(b"ACGT"), n_umi).tolist())
    q1 = bytes(rng.integers(40, 74, n_cb, dtype=np.uint8).tolist()); q2 = bytes(rng.integers(40, 74, n_umi, dtype=np.uint8).tolist())
    return name + b" " + cb + b" " + umi + b" " + q1 + b" " + q2 + b"\n"


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_row_counts_around_a_wave_and_a_workgroup(n):
    L = lib()
    rng = np.random.default_rng(n)
    text = b"".join(_row(rng, (b"@" if i % 3 == 0 else b"") + b"read%d" % i) for i in range(n))
    got, want = check(L, [text], min_phred=41, absent=[b"", b"read", b"read%d" % n, b"@@read0"])
    assert want.counts()["valid"] == n and (n < 64 or 0 < sum(g.pass_ for g in got) < n)


def test_one_name_two_hundred_times():
    """every lane of the insert kernel on one slot: the first row is the canonical one"""
    L = lib()
    rng = np.random.default_rng(3)
    got, want = check(L, [b"".join(_row(rng, b"same") for _ in range(200))])
    assert [g.canonical for g in got] == [0] * 200 and want.counts()["repeated"] == 199


def test_three_hash_bits_make_chains_longer_than_a_wave_that_wrap():
    """hash_bits = 3: 150 distinct names on eight hash values in a table of 512 slots.  70 of them carry the value whose probes start at slot 486,
    so that chain runs over the table's end and is longer than a wave; the rest crowd the other seven starts."""
    L = lib()
    rng = np.random.default_rng(4)
    assert slot_of(4, 511) == 486
    wrap, rest, i = [], [], 0
    while len(wrap) < 70 or len(rest) < 80:
        name = b"n%d" % i; i += 1
        (wrap if fnv1a(name) & 7 == 4 else rest).append(name)
    names = wrap[:70] + rest[:80]
    order = rng.permutation(len(names))
    text = b"".join(_row(rng, names[k]) for k in order)
    got, want = check(L, [text], hash_bits=3, absent=[b"n%d" % k for k in range(i, i + 64)])
    assert want.counts() == dict(rows=150, valid=150, malformed=0, repeated=0) and {g.hash for g in got} <= set(range(8))


def test_long_names_short_names_and_prefixes():
    L = lib()
    rng = np.random.default_rng(5)
    names = [b"x", b"y" * 254, b"y" * 253, b"abc", b"abcd", b"ab", b"abcde", b"", b"a"]
    check(L, [b"".join(_row(rng, x) for x in names)], hash_bits=2, absent=[b"y" * 252, b"abcdef", b"b"])
    check(L, [b"".join(_row(rng, x) for x in names)], absent=[b"y" * 252, b"abcdef", b"b"])


def test_three_calls_with_repeats_across_calls():
    L = lib()
    rng = np.random.default_rng(6)
    a = b"".join(_row(rng, b"r%d" % i) for i in range(100))
    b = b"".join(_row(rng, b"r%d" % i) for i in range(50, 180))            # 50 names again
    c = b"".join(_row(rng, b"@r%d" % i) for i in range(0, 300, 7))[:-1]     # more of them, and no final newline
    got, want = check(L, [a, b, c], min_phred=[50, 60, 70])
    assert want.counts()["repeated"] == 50 + len([i for i in range(0, 300, 7) if i < 180])
    assert got[100].canonical == 50 and got[100 + 130].canonical == 0


def test_every_row_form():
    L = lib()
    forms = [b"r1 ACGT TTGA IIII JJJJ\n", b"@r2 ACGT TTGA IIII JJJJ\r\n", b"@@r3 ACGT TTGA IIII JJJJ\n", b"broken\n", b"a b c d\n", b"\n", b"\r\n", b"r4  TTGA IIII JJJJ\n",
             b"r5 ACGT  IIII JJJJ\n", b" ACGT TTGA IIII JJJJ\n", b"r6 AC TT II J J J\n", b"r7 AC TT  \n", b"r8 AC TT II \n", b"r9 ACNT TTGA 5555 5555\n",
             b"r10 AC NN 55 55\n", b"r11 " + b"A" * 31 + b" " + b"C" * 32 + b" I I\n", b"r12 AC TT 54 55\n", b"r13 AC TT 55 45\n", b"r14 AC TT 5\xff 55\n", b"r1 GGGG GGGG IIII IIII\n",
             b"acgt acgt acgt 55 55\n", b"r15 AC TT 55 55\r"]
    for min_phred in (0, 33, 34, 53):
        got, want = check(L, [b"".join(forms)], min_phred=min_phred, absent=[b"r4", b"r5", b"broken"])
        codes = {want.rows[k]["name"]: (g.cb_code, g.umi_code) for k, g in enumerate(got) if g.valid}
        assert codes[b"r9"][0] == 0 and codes[b"r10"][1] == 0 and codes[b"r11"][0] != 0 and codes[b"r11"][1] == 0 and codes[b"acgt"] == (0, 0)
    check(L, [b"".join(forms[:-1]), forms[-1], b"", b"\n"], min_phred=53)      # a last line without newline, an empty text, a lone newline


def test_claims_start_unclaimed_and_argument_checks():
    L = lib()
    rng = np.random.default_rng(8)
    t = Table(L, [b"".join(_row(rng, b"r%d" % i) for i in range(10))])
    claims = np.zeros(10, np.uint64)
    assert L.dropest_read_params_claims_to_host(t.h, 0, 10, claims.ctypes.data) == 0 and (claims == 0xFFFFFFFFFFFFFFFF).all()
    assert L.dropest_read_params_reset_claims(t.h) == 0
    assert L.dropest_read_params_claims_to_host(t.h, 5, 6, claims.ctypes.data) != 0 and b"outside" in L.dropest_bgzf_last_error()
    assert L.dropest_read_params_build(t.h) != 0 and L.dropest_read_params_add_text(t.h, None, 0, None, 0, 0) != 0
    t.close()
    h = C.c_void_p()
    assert L.dropest_read_params_create(0, 0, C.byref(h)) == 0
    assert L.dropest_read_params_counts(h, None, None, None, None) != 0 and b"not built" in L.dropest_bgzf_last_error()
    bad = np.array([5, 3], np.uint64); buf = np.zeros(8, np.uint8)
    assert L.dropest_read_params_add_text(h, buf.ctypes.data, 8, bad.ctypes.data, 2, 0) != 0
    L.dropest_read_params_destroy(h)
