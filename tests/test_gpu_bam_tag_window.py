"""dropest_bam_decoder_tag_window (include/dropest_bgzf.h; csrc/k_bamtag.h) through the C-ABI alone: the tagged records of a decoded window are,
byte for byte, the concatenation of tests/bam_tag_model.py's records -- over one window, over two windows cut at a BGZF block boundary inside a
record (in both window orders), after a reset; and refused once tagging is turned off."""
import ctypes as C
import gzip
import struct

import numpy as np
import pytest

from dropest_amd import capi

import bam_model as bm
import bam_tag_model as tm
import bam_writer as bw
from test_gpu_bam_decoder_cabi import Cfg, Window, tag16

pytestmark = pytest.mark.gpu
P = C.POINTER


class TagCfg(C.Structure):
    _fields_ = [("out_tag", C.c_uint16 * 5), ("type_tag", C.c_uint16), ("type_len", C.c_uint32 * 3), ("type_val", (C.c_uint8 * 24) * 3),
                ("gene_name_off", C.c_void_p), ("gene_name_pool", C.c_void_p), ("n_gene_names", C.c_uint32)]


def tag_cfg(out_cfg):
    t = TagCfg()
    for k, name in enumerate((out_cfg.gene, out_cfg.cb_raw, out_cfg.umi_raw, out_cfg.cb_quality, out_cfg.umi_quality)):
        t.out_tag[k] = tag16(name) if name else 0
    t.type_tag = tag16(out_cfg.read_type) if out_cfg.read_type else 0
    for k, v in enumerate((out_cfg.exonic, out_cfg.intronic, out_cfg.intergenic)):
        t.type_len[k] = len(v)
        for j, c in enumerate(v):
            t.type_val[k][j] = c
    return t


def parse_cfg(cfg):
    c = Cfg()
    for k, t in enumerate(cfg.tags):
        c.tag[k] = tag16(t) if t else 0
    c.filled_bam, c.min_phred, c.has_read_type, c.n_refs = int(cfg.filled_bam), cfg.min_phred, int(cfg.read_type), cfg.n_refs
    c.intronic_len, c.intergenic_len = len(cfg.intronic), len(cfg.intergenic)
    for j, ch in enumerate(cfg.intronic):
        c.intronic[j] = ch
    for j, ch in enumerate(cfg.intergenic):
        c.intergenic[j] = ch
    return c


_B_VALUES = {"c": -3, "C": 200, "s": -300, "S": 60000, "i": -70000, "I": 4000000000, "f": 1.5}


def _fillers():
    """every aux type, to stand between the edited tags: the scalars, Z, H, and B arrays of every subtype with 0, 1 and 300 values"""
    out = [("XA", "A", "q"), ("Xc", "c", -5), ("XC", "C", 250), ("Xs", "s", -3000), ("XS", "S", 65000), ("Xi", "i", -100000), ("XI", "I", 4000000000), ("Xf", "f", 2.5),
           ("XZ", "Z", "some text"), ("XH", "H", "1AE301")]
    for sub, v in _B_VALUES.items():
        for count in (0, 1, 300):
            out.append(("B" + sub, "B", (sub, [v] * count)))
    out.append(("XB", "B", ("C", list(b"CRZ\x00URZ\x00"))))      # a payload that reads like two of the edited tags: the walk must go by type
    return out


def make_records(filled, with_phred, seed, n=3000, uq="some"):
    rng = np.random.default_rng(seed)
    fill = _fillers()
    genes = ["GENE%d" % i for i in range(40)]
    recs = []
    for i in range(n):
        cb = "".join(rng.choice(list("ACGT"), 12)); umi = "".join(rng.choice(list("ACGT"), 8))
        if i % 211 == 0:
            cb = cb[:5] + "N" + cb[6:]
        if i % 223 == 0:
            umi = umi[:2] + "N" + umi[3:]
        g = None if i % 9 == 0 else genes[int(rng.integers(0, len(genes)))]
        rt = [None, "N", "I", "E"][i % 4] if g else None
        tags = []
        if i % 5 == 0:
            tags.append(("CR", "Z", "OLDOLD"))                                         # an edited tag first
        if filled:
            tags.append(("CB", "Z", cb))
        tags.append(fill[i % len(fill)])
        if i % 7 == 0:
            tags.append(("UR", "i", 77))                                               # ... in the middle, as a number
        if filled:
            tags.append(("UB", "Z", umi))
        tags.append(fill[(i * 7 + 3) % len(fill)])
        if i % 3 != 0 or uq != "some":                                                 # uq: "some" records have a UQ of 8, "all" have one, or strings of "two" lengths
            tags.append(("UQ", "Z", "".join(chr(33 + int(x)) for x in rng.integers(25 if with_phred else 2, 40, 6 if uq == "two" and i % 4 == 0 else 8))))
        if i % 6 == 1:
            tags.append(("CQ", "Z", "".join(chr(33 + int(x)) for x in rng.integers(25 if with_phred else 2, 40, 12))))      # (i % 6 in 2, 4, 5: UQ without CQ)
        if i % 31 == 0:
            tags.append(("CQ", "Z", ""))                                               # present but empty
        if g:
            tags.append(("GX", "Z", g))
        if rt:
            tags.append(("RE", "A" if i % 8 < 4 else "Z", rt))
        if i % 11 == 0:
            tags.append(("CR", "Z", "AGAIN"))                                          # ... and last, repeated
        if i % 301 == 7:
            tags.append(b"QQ?" + b"CRZbehind the stop\x00")                            # an unknown type: the walk stops, what follows stays
        name = ("r%d" % i) if filled else "r%d!%s#%s" % (i, cb, umi)
        flag, ref = 0, int(rng.integers(0, 4))
        if i % 97 == 1:
            flag = 4
        elif i % 97 == 2:
            flag = 0x100
        elif i % 97 == 3:
            ref = -1
        elif i % 97 == 4:
            if filled:
                tags = [t for t in tags if not (isinstance(t, tuple) and t[0] == "UB")]
            else:
                name = "r%d-no-separators" % i
        elif i % 97 == 5 and with_phred:
            tags = [t for t in tags if not (isinstance(t, tuple) and t[0] == "UQ")] + [("UQ", "Z", "II#IIIII")]      # below the limit
        elif i % 97 == 6:
            tags = []                                                                  # no aux data at all
        elif i % 97 == 7:
            suffix = "" if filled else "!%s#%s" % (cb, umi)
            name = "x#y!" + "n" * (254 - 4 - len(suffix)) + suffix                     # a 254-byte read name
        seq = "ACGT" * 10
        if i == 1500:                                                                  # 10 000 bases and 2 KB of aux: more than a BGZF block, more than any LDS stage
            seq = "ACGT" * 2500
            tags = tags[:2] + [("Y%d" % (k % 10), "Z", "filler %03d " % k * 4) for k in range(40)] + tags[2:]
        recs.append(bw.record(ref, i, name, flag=flag, seq=seq, tags=tags))
    return recs


def first_record(blob):
    """(offset of the BGZF block that holds the first record, bytes of the header inside that block, inflated length of the header)"""
    raw = gzip.decompress(blob)
    first, _ = bm.records_of(raw)
    at, cum = 0, 0
    while at < len(blob):
        bsize = struct.unpack_from("<H", blob, at + 16)[0] + 1
        isize = struct.unpack_from("<I", blob, at + bsize - 4)[0]
        if cum <= first < cum + isize:
            return at, first - cum
        cum += isize; at += bsize
    raise AssertionError("no block holds the first record")


def block_starts(comp):
    out, at = [], 0
    while at < len(comp):
        out.append(at)
        at += struct.unpack_from("<H", comp, at + 16)[0] + 1
    return out


class Decoder:
    def __init__(self, cfg):
        self.L = L = capi.lib()
        L.dropest_bgzf_last_error.restype = C.c_char_p
        L.dropest_bam_decoder_window.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, P(Window)]
        L.dropest_bam_decoder_window_inflate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, P(C.c_int)]
        L.dropest_bam_decoder_window_chain.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
        L.dropest_bam_decoder_window_finish.argtypes = [C.c_void_p, C.c_int, P(Window)]
        L.dropest_bam_decoder_reset.argtypes = [C.c_void_p, C.c_void_p]
        L.dropest_bam_decoder_set_tagging.argtypes = [C.c_void_p, C.c_void_p]
        L.dropest_bam_decoder_tag_window.argtypes = [C.c_void_p, P(C.c_void_p), P(C.c_uint64), P(C.c_uint64)]
        L.dropest_bam_decoder_tagged_to_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.dropest_bam_decoder_destroy.argtypes = [C.c_void_p]
        self.cfg = cfg
        self.dec = C.c_void_p()
        assert L.dropest_bam_decoder_create(0, C.byref(cfg), C.byref(self.dec)) == 0, L.dropest_bgzf_last_error()

    def close(self):
        self.L.dropest_bam_decoder_destroy(self.dec)

    def tagged(self):
        """tags the last window: (its bytes on the host, records written)"""
        ptr, ln, n = C.c_void_p(), C.c_uint64(), C.c_uint64()
        assert self.L.dropest_bam_decoder_tag_window(self.dec, C.byref(ptr), C.byref(ln), C.byref(n)) == 0, self.L.dropest_bgzf_last_error()
        buf = np.zeros(ln.value + 1, np.uint8)
        assert self.L.dropest_bam_decoder_tagged_to_host(self.dec, buf.ctypes.data, ln.value) == 0, self.L.dropest_bgzf_last_error()
        if ln.value:
            assert ptr.value and self.L.dropest_bam_decoder_tagged_to_host(self.dec, buf.ctypes.data, ln.value - 1) != 0      # too small a destination is refused
        return buf[:ln.value].tobytes(), n.value

    def window(self, comp, skip, final):
        w = Window()
        assert self.L.dropest_bam_decoder_window(self.dec, comp.ctypes.data, len(comp), skip, final, None, None, C.byref(w)) == 0, self.L.dropest_bgzf_last_error()
        return w


CASES = [   # filled, block, read-type tag, min_phred
    (True, 997, True, 0),
    (True, 12_345, False, 20),
    (False, 997, False, 0),
    (False, 12_345, True, 0),
]


@pytest.mark.parametrize("filled,block,read_type,phred", CASES)
def test_tagged_window_equals_the_model(tmp_path, filled, block, read_type, phred):
    refs = [("chr%d" % i, 1 << 20) for i in range(4)]
    recs = make_records(filled, phred > 0, seed=block + int(filled))
    cfg = bm.Cfg(tags=("CB", "UB", "CQ", "UQ", "GX", "RE"), filled_bam=filled, min_phred=33 + phred if phred else 0, read_type=True, intronic=b"N", intergenic=b"I", n_refs=len(refs))
    out_cfg = tm.OutCfg(read_type="RE", exonic=b"E", intronic=b"N", intergenic=b"I") if read_type else tm.OutCfg()
    rows = [bm.parse_record(r, cfg, bm.Dicts(chr_of_ref=[0] * 4)) for r in recs]
    counts = [sum(1 for r in rows if r.status == s) for s in range(5)]
    assert all(counts[s] > 0 for s in (0, 1, 2, 3)) and (counts[4] > 0) == (phred > 0 and filled)      # every status the mode can give
    model = [tm.tagged_record(r, cfg, out_cfg) for r in recs]
    assert [m is None for m in model] == [r.status != bm.OK for r in rows]
    want = b"".join(m for m in model if m is not None)
    path = str(tmp_path / "t.bam")
    bw.write_bam(path, refs, recs, block=block)
    blob = open(path, "rb").read()
    c0, u0 = first_record(blob)
    comp = np.frombuffer(blob[c0:], np.uint8)
    d = Decoder(parse_cfg(cfg))
    L = d.L
    try:
        # tagging is off until it is configured
        d.window(comp, u0, 1)
        ptr, ln, n = C.c_void_p(), C.c_uint64(), C.c_uint64()
        assert L.dropest_bam_decoder_tag_window(d.dec, C.byref(ptr), C.byref(ln), C.byref(n)) != 0 and b"not configured" in L.dropest_bgzf_last_error()
        t = tag_cfg(out_cfg)
        # 1. one window
        assert L.dropest_bam_decoder_reset(d.dec, C.byref(d.cfg)) == 0
        assert L.dropest_bam_decoder_set_tagging(d.dec, C.byref(t)) == 0, L.dropest_bgzf_last_error()
        w = d.window(comp, u0, 1)
        assert list(w.counts) == counts
        got, n_written = d.tagged()
        assert n_written == counts[bm.OK] == w.n_accepted
        assert len(got) == len(want) and got == want
        assert d.tagged() == (got, n_written)                                   # the window may be tagged again
        # ... output tags without a name are never written, and drop nothing: no gene tag, no UMI quality tag
        nameless = tm.OutCfg(gene="", cb_raw=out_cfg.cb_raw, umi_raw=out_cfg.umi_raw, cb_quality=out_cfg.cb_quality, umi_quality="", read_type=out_cfg.read_type,
                             exonic=out_cfg.exonic, intronic=out_cfg.intronic, intergenic=out_cfg.intergenic)
        t0 = tag_cfg(nameless)
        assert t0.out_tag[0] == 0 and t0.out_tag[4] == 0
        assert L.dropest_bam_decoder_set_tagging(d.dec, C.byref(t0)) == 0, L.dropest_bgzf_last_error()
        want0 = b"".join(m for m in (tm.tagged_record(r, cfg, nameless) for r in recs) if m is not None)
        assert want0 != want and d.tagged() == (want0, counts[bm.OK])
        assert L.dropest_bam_decoder_set_tagging(d.dec, C.byref(t)) == 0
        # 2. two windows, cut at a block boundary inside a record; the first is not the file's last
        starts = block_starts(comp.tobytes())
        cut = starts[len(starts) // 2]
        a, b = comp[:cut].copy(), comp[cut:].copy()
        assert L.dropest_bam_decoder_reset(d.dec, C.byref(d.cfg)) == 0
        assert L.dropest_bam_decoder_set_tagging(d.dec, C.byref(t)) == 0
        w1 = d.window(a, u0, 0)
        assert w1.tail_bytes > 0                                                 # the cut is inside a record
        g1, n1 = d.tagged()
        w2 = d.window(b, 0, 1)
        g2, n2 = d.tagged()
        assert n1 == w1.n_accepted and n2 == w2.n_accepted and n1 + n2 == counts[bm.OK] and n1 > 0 and n2 > 0
        assert g1 + g2 == want
        # ... and in the other window order: the inflate of window 2 is queued before window 1 is finished
        assert L.dropest_bam_decoder_reset(d.dec, C.byref(d.cfg)) == 0
        assert L.dropest_bam_decoder_set_tagging(d.dec, C.byref(t)) == 0
        s1, s2, v1, v2 = C.c_int(-1), C.c_int(-1), Window(), Window()
        assert L.dropest_bam_decoder_window_inflate(d.dec, a.ctypes.data, len(a), C.byref(s1)) == 0, L.dropest_bgzf_last_error()
        assert L.dropest_bam_decoder_window_inflate(d.dec, b.ctypes.data, len(b), C.byref(s2)) == 0, L.dropest_bgzf_last_error()
        assert L.dropest_bam_decoder_window_chain(d.dec, s1.value, u0, 0, None, None) == 0, L.dropest_bgzf_last_error()
        assert L.dropest_bam_decoder_window_finish(d.dec, s1.value, C.byref(v1)) == 0, L.dropest_bgzf_last_error()
        p1, m1 = d.tagged()
        assert L.dropest_bam_decoder_window_chain(d.dec, s2.value, 0, 1, None, None) == 0, L.dropest_bgzf_last_error()
        assert L.dropest_bam_decoder_window_finish(d.dec, s2.value, C.byref(v2)) == 0, L.dropest_bgzf_last_error()
        p2, m2 = d.tagged()
        assert (p1, m1, p2, m2) == (g1, n1, g2, n2)
        # 3. a reset turns tagging off (the gene names of a -g configuration were the dropped annotation's); configured again, the same bytes
        assert L.dropest_bam_decoder_reset(d.dec, C.byref(d.cfg)) == 0
        d.window(comp, u0, 1)
        assert L.dropest_bam_decoder_tag_window(d.dec, C.byref(ptr), C.byref(ln), C.byref(n)) != 0
        assert L.dropest_bam_decoder_set_tagging(d.dec, C.byref(t)) == 0
        assert d.tagged() == (want, counts[bm.OK])
        # 4. set_tagging(NULL): the call is refused with an error
        assert L.dropest_bam_decoder_set_tagging(d.dec, None) == 0
        assert L.dropest_bam_decoder_tag_window(d.dec, C.byref(ptr), C.byref(ln), C.byref(n)) != 0 and b"not configured" in L.dropest_bgzf_last_error()
        assert ptr.value is None and ln.value == 0 and n.value == 0
    finally:
        d.close()
