"""dropest_bam_decoder_set_filtering / _filter_window (include/dropest_bgzf.h; the filtered mode of csrc/k_bamtag.h) through the C-ABI alone: the
filtered records of a decoded window are, byte for byte, tests/bam_filter_model.py's over synthetic, seeded decisions given as host arrays -- over
one window, over two windows cut at a BGZF block boundary inside a record (in both window orders; the second window's decisions begin at the
first's accepted count), at the record counts where the workgroup (4 records) and the scan tile (4 096) end; and what the calls refuse."""
import ctypes as C

import numpy as np
import pytest

import bam_filter_model as fm
import bam_model as bm
import bam_tag_model as tm
import bam_writer as bw
from test_gpu_bam_decoder_cabi import Window, tag16
from test_gpu_bam_tag_window import Decoder, block_starts, first_record, make_records, parse_cfg, tag_cfg

pytestmark = pytest.mark.gpu
P = C.POINTER
ESC = 1 << 63
REFS = [("chr%d" % i, 1 << 20) for i in range(4)]


class FilterCfg(C.Structure):
    _fields_ = [("out_tag", C.c_uint16 * 2), ("on_device", C.c_uint32), ("cell_barcode", C.c_void_p), ("n_cells", C.c_uint32), ("n_side", C.c_uint32),
                ("side_off", C.c_void_p), ("side_pool", C.c_void_p)]


# the side strings of escaped codes: N in them, one of 70 bytes (more than one step of 64 lanes), one of 33 bases (more than a code holds)
SIDE = [b"ACGTNACGTACG", b"N", b"ACGTTGCAN" * 7 + b"ACGTACG", b"ACGTACGTACGTACGTACGTACGTACGTACGTA", b"TTNNGGAA", b""]
assert len(SIDE[2]) == 70 and len(SIDE[3]) == 33


def tables(seed, n_cells=64):
    """every cell's barcode code: plain ones of 1, 12, 16 and 31 bases, every escaped kind, and the code 1 (no barcode)"""
    rng = np.random.default_rng(seed)
    codes = []
    for c in range(n_cells):
        kind = c % 10
        if kind < 4:
            codes.append(fm.pack_code(bytes(rng.choice(list(b"ACGT"), (1, 12, 16, 31)[kind]).tolist())))
        elif kind < 9:
            codes.append(ESC | (kind - 4))
        else:
            codes.append(1 if c % 20 == 9 else ESC | 5)          # no characters, as a plain and as an escaped code
    return np.array(codes, np.uint64)


def decisions(seed, n, n_cells):
    """verdict (a third 0 at least), target cell, corrected UMI (plain of 8 and 12 bases, escaped, the code 1) for n accepted records"""
    rng = np.random.default_rng(seed)
    verdict = rng.integers(0, 5, n).astype(np.uint8)
    verdict[rng.random(n) < 0.25] = 0
    cell = rng.integers(0, n_cells, n).astype(np.uint32)
    cell[verdict == 1] = 0xFFFFFFFF; cell[verdict == 2] = 0xFFFFFFFF       # as dropest_read_corrections gives them: not looked at
    umi = np.zeros(n, np.uint64)
    for k in range(n):
        kind = int(rng.integers(0, 8))
        if kind < 3:
            umi[k] = fm.pack_code(bytes(rng.choice(list(b"ACGT"), 8).tolist()))
        elif kind < 6:
            umi[k] = fm.pack_code(bytes(rng.choice(list(b"ACGT"), 12).tolist()))
        elif kind == 6:
            umi[k] = ESC | int(rng.integers(0, len(SIDE)))
        else:
            umi[k] = 1
    return verdict, cell, umi


def as_strings(verdict, cell, umi, codes):
    return [(int(v), fm.code_string(int(codes[c]), SIDE) if c < len(codes) else b"", fm.code_string(int(u), SIDE)) for v, c, u in zip(verdict, cell, umi)]


class FilterDecoder(Decoder):
    def __init__(self, cfg):
        super().__init__(cfg)
        L = self.L
        L.dropest_bam_decoder_set_filtering.argtypes = [C.c_void_p, C.c_void_p]
        L.dropest_bam_decoder_filter_window.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, P(C.c_void_p), P(C.c_uint64), P(C.c_uint64)]
        self.keep = []

    def set_filtering(self, codes, side=SIDE, cb="CB", umi="UB", n_cells=None, n_side=None):
        f = FilterCfg()
        f.out_tag[0], f.out_tag[1] = (tag16(cb) if cb else 0), (tag16(umi) if umi else 0)
        off = np.cumsum([0] + [len(s) for s in side]).astype(np.uint32)
        pool = np.frombuffer(b"".join(side) + b"\0", np.uint8).copy()
        codes = np.ascontiguousarray(codes, np.uint64)
        f.on_device, f.cell_barcode, f.n_cells = 0, codes.ctypes.data, len(codes) if n_cells is None else n_cells
        f.n_side, f.side_off, f.side_pool = (len(side) if n_side is None else n_side), off.ctypes.data, pool.ctypes.data
        self.keep = [codes, off, pool]
        return self.L.dropest_bam_decoder_set_filtering(self.dec, C.byref(f))

    def filter_call(self, verdict, cell, umi, n=None):
        ptr, ln, nw = C.c_void_p(), C.c_uint64(), C.c_uint64()
        verdict, cell, umi = np.ascontiguousarray(verdict, np.uint8), np.ascontiguousarray(cell, np.uint32), np.ascontiguousarray(umi, np.uint64)
        # (an array of no element still has an address: n = 0 must not need one)
        rc = self.L.dropest_bam_decoder_filter_window(self.dec, verdict.ctypes.data if len(verdict) else None, cell.ctypes.data if len(cell) else None,
                                                      umi.ctypes.data if len(umi) else None, len(verdict) if n is None else n, 0, C.byref(ptr), C.byref(ln), C.byref(nw))
        return rc, ptr.value, ln.value, nw.value

    def filtered(self, verdict, cell, umi):
        """filters the last window: (its bytes on the host, records written)"""
        rc, ptr, ln, nw = self.filter_call(verdict, cell, umi)
        assert rc == 0, self.L.dropest_bgzf_last_error()
        assert (ptr is None) == (ln == 0)
        buf = np.zeros(ln + 1, np.uint8)
        assert self.L.dropest_bam_decoder_tagged_to_host(self.dec, buf.ctypes.data, ln) == 0, self.L.dropest_bgzf_last_error()
        return buf[:ln].tobytes(), nw


def bam_blob(tmp_path, recs, block):
    path = str(tmp_path / "f.bam")
    bw.write_bam(path, REFS, recs, block=block)
    blob = open(path, "rb").read()
    c0, u0 = first_record(blob)
    return np.frombuffer(blob[c0:], np.uint8), u0


def model_cfg(filled):
    return bm.Cfg(tags=("CB", "UB", "CQ", "UQ", "GX", "RE"), filled_bam=filled, min_phred=0, read_type=True, intronic=b"N", intergenic=b"I", n_refs=len(REFS))


OUT = fm.FilterOutCfg(read_type="RE", exonic=b"E", intronic=b"N", intergenic=b"I")


@pytest.mark.parametrize("filled", [True, False])
def test_filtered_window_equals_the_model(tmp_path, filled):
    recs = make_records(filled, False, seed=5 + int(filled))
    cfg = model_cfg(filled)
    n_ok = sum(1 for r in recs if bm.parse_record(r, cfg, bm.Dicts(chr_of_ref=[0] * 4)).status == bm.OK)
    codes = tables(11)
    verdict, cell, umi = decisions(12 + int(filled), n_ok, len(codes))
    assert (verdict == 0).sum() * 3 >= n_ok and all((verdict == v).any() for v in range(5))
    dec = as_strings(verdict, cell, umi, codes)
    want, want_n, used = fm.filtered_stream(recs, cfg, OUT, dec)
    assert used == n_ok and want_n == int((verdict == 0).sum())
    want_b = b"".join(m for m in (tm.tagged_record(r, cfg, OUT) for r in recs) if m is not None)
    comp, u0 = bam_blob(tmp_path, recs, 997 if filled else 12_345)
    d = FilterDecoder(parse_cfg(cfg))
    L = d.L
    try:
        t = tag_cfg(OUT)
        assert L.dropest_bam_decoder_set_tagging(d.dec, C.byref(t)) == 0, L.dropest_bgzf_last_error()
        assert d.set_filtering(codes) == 0, L.dropest_bgzf_last_error()
        # 1. one window
        w = d.window(comp, u0, 1)
        assert w.n_accepted == n_ok
        got, n_written = d.filtered(verdict, cell, umi)
        assert n_written == want_n
        assert len(got) == len(want) and got == want
        assert d.filtered(verdict, cell, umi) == (got, n_written)                # the window may be filtered again
        assert d.tagged() == (want_b, n_ok)                                      # ... and tagged afterwards: the -b bytes
        assert d.filtered(verdict, cell, umi) == (got, n_written)
        # 2. two windows, cut at a block boundary inside a record
        starts = block_starts(comp.tobytes())
        cut = starts[len(starts) // 2]
        a, b = comp[:cut].copy(), comp[cut:].copy()

        def configure():
            assert L.dropest_bam_decoder_reset(d.dec, C.byref(d.cfg)) == 0
            assert L.dropest_bam_decoder_set_tagging(d.dec, C.byref(t)) == 0
            assert d.set_filtering(codes) == 0

        configure()
        w1 = d.window(a, u0, 0)
        assert w1.tail_bytes > 0
        n1 = w1.n_accepted
        g1, m1 = d.filtered(verdict[:n1], cell[:n1], umi[:n1])
        w2 = d.window(b, 0, 1)
        assert n1 + w2.n_accepted == n_ok and n1 > 0 and w2.n_accepted > 0
        g2, m2 = d.filtered(verdict[n1:], cell[n1:], umi[n1:])
        assert m1 + m2 == want_n and g1 + g2 == want
        # ... and in the other window order: the inflate of window 2 is queued before window 1 is finished
        configure()
        s1, s2, v1, v2 = C.c_int(-1), C.c_int(-1), Window(), Window()
        assert L.dropest_bam_decoder_window_inflate(d.dec, a.ctypes.data, len(a), C.byref(s1)) == 0, L.dropest_bgzf_last_error()
        assert L.dropest_bam_decoder_window_inflate(d.dec, b.ctypes.data, len(b), C.byref(s2)) == 0, L.dropest_bgzf_last_error()
        assert L.dropest_bam_decoder_window_chain(d.dec, s1.value, u0, 0, None, None) == 0, L.dropest_bgzf_last_error()
        assert L.dropest_bam_decoder_window_finish(d.dec, s1.value, C.byref(v1)) == 0, L.dropest_bgzf_last_error()
        p1 = d.filtered(verdict[:n1], cell[:n1], umi[:n1])
        assert L.dropest_bam_decoder_window_chain(d.dec, s2.value, 0, 1, None, None) == 0, L.dropest_bgzf_last_error()
        assert L.dropest_bam_decoder_window_finish(d.dec, s2.value, C.byref(v2)) == 0, L.dropest_bgzf_last_error()
        p2 = d.filtered(verdict[n1:], cell[n1:], umi[n1:])
        assert (p1, p2) == ((g1, m1), (g2, m2))
        # 3. corrected tags under other names, and one without a name (never written, drops nothing)
        other = fm.FilterOutCfg(read_type="RE", exonic=b"E", intronic=b"N", intergenic=b"I", cell_barcode="XC", umi="")
        configure()
        assert d.set_filtering(codes, cb="XC", umi="") == 0
        d.window(comp, u0, 1)
        want_o, n_o, _ = fm.filtered_stream(recs, cfg, other, dec)
        assert want_o != want and d.filtered(verdict, cell, umi) == (want_o, n_o)
    finally:
        d.close()


def small_records(n, unaccepted_head):
    """n short -f records; the first `unaccepted_head` are unmapped, every 7th of the rest has no UMI"""
    recs = []
    for i in range(n):
        tags = [("CB", "Z", "ACGTACGTAC%02d" % (i % 100)), ("NH", "i", i)]
        if i % 7 != 3:
            tags.append(("UB", "Z", "TTGA" + "ACGT"[i % 4] * 4))
        if i % 3:
            tags.append(("GX", "Z", "G%d" % (i % 5)))
        recs.append(bw.record(i % 4, i, "q%d" % i, flag=4 if i < unaccepted_head else 0, seq="ACGT" * 5, tags=tags))
    return recs


@pytest.mark.parametrize("n_rec", [1, 4, 5, 4096, 4097])
def test_the_edges_of_the_workgroup_and_the_scan_tile(tmp_path, n_rec):
    cfg = model_cfg(True)
    codes = tables(3, n_cells=20)
    d = FilterDecoder(parse_cfg(cfg))
    L = d.L
    try:
        t = tag_cfg(OUT)
        for head in (0, 1 if n_rec == 1 else max(1, n_rec // 3)):            # ... and a window whose first records are all unaccepted
            recs = small_records(n_rec, head)
            comp, u0 = bam_blob(tmp_path, recs, 60_000)
            assert L.dropest_bam_decoder_reset(d.dec, C.byref(d.cfg)) == 0
            assert L.dropest_bam_decoder_set_tagging(d.dec, C.byref(t)) == 0
            assert d.set_filtering(codes) == 0, L.dropest_bgzf_last_error()
            w = d.window(comp, u0, 1)
            n_ok = w.n_accepted
            assert w.n_records == n_rec and n_ok == sum(1 for i in range(head, n_rec) if i % 7 != 3)
            verdict, cell, umi = decisions(n_rec + head, n_ok, len(codes))
            variants = [verdict, np.full(n_ok, 2, np.uint8)]                     # the mix; nothing written
            if n_ok:
                only_first, only_last = np.full(n_ok, 4, np.uint8), np.full(n_ok, 3, np.uint8)
                only_first[0] = 0; only_last[-1] = 0
                variants += [only_first, only_last]
            for v in variants:
                c = cell.copy()
                c[(v != 1) & (v != 2) & (c == 0xFFFFFFFF)] = 7
                want, want_n, used = fm.filtered_stream(recs, cfg, OUT, as_strings(v, c, umi, codes))
                assert used == n_ok
                got, n_written = d.filtered(v, c, umi)
                assert n_written == want_n == int((v == 0).sum())
                assert len(got) == len(want) and got == want
                assert (len(got) == 0) == (want_n == 0)
    finally:
        d.close()


def test_what_the_calls_refuse(tmp_path):
    cfg = model_cfg(True)
    recs = small_records(50, 2)
    comp, u0 = bam_blob(tmp_path, recs, 60_000)
    codes = tables(3, n_cells=20)
    d = FilterDecoder(parse_cfg(cfg))
    L = d.L
    err = L.dropest_bgzf_last_error
    try:
        t = tag_cfg(OUT)
        w = d.window(comp, u0, 1)
        n_ok = w.n_accepted
        verdict, cell, umi = np.zeros(n_ok, np.uint8), np.full(n_ok, 3, np.uint32), np.full(n_ok, fm.pack_code(b"ACGTACGT"), np.uint64)
        # filtering needs tagging first; neither configured: the window is not filtered
        assert d.set_filtering(codes) != 0 and b"set_tagging" in err()
        assert d.filter_call(verdict, cell, umi)[0] == 1 and b"tagging is not configured" in err()
        assert L.dropest_bam_decoder_set_tagging(d.dec, C.byref(t)) == 0
        assert d.filter_call(verdict, cell, umi)[0] == 1 and b"filtering is not configured" in err()
        # two output tags with one name: the two new ones, or a new one and one of -b's
        for cb, um in (("CB", "CB"), ("CR", "UB"), ("CB", "UR"), ("RE", "UB"), ("CB", "GX")):
            assert d.set_filtering(codes, cb=cb, umi=um) != 0 and b"share a name" in err()
            assert d.filter_call(verdict, cell, umi)[0] == 1 and b"filtering is not configured" in err()
        assert d.set_filtering(codes) == 0, err()
        good = d.filtered(verdict, cell, umi)
        assert good[1] == n_ok and good[0] == fm.filtered_stream(recs, cfg, OUT, as_strings(verdict, cell, umi, codes))[0]
        # the number of decisions is the window's accepted count
        for n in (n_ok - 1, n_ok + 1, 0):
            rc, ptr, ln, nw = d.filter_call(verdict, cell, umi, n=n)
            assert rc == 1 and b"decisions for a window" in err() and (ptr, ln, nw) == (None, 0, 0)
        # a cell id out of range, an escaped UMI or barcode whose side string does not exist: an error when the read is written ...
        bad_cell, bad_umi = cell.copy(), umi.copy()
        bad_cell[n_ok // 2] = len(codes)
        bad_umi[n_ok - 1] = ESC | len(SIDE)
        bad_codes = codes.copy(); bad_codes[3] = ESC | 1000
        for c, u, k in ((bad_cell, umi, codes), (cell, bad_umi, codes), (cell, umi, bad_codes)):
            assert d.set_filtering(k) == 0
            rc, ptr, ln, nw = d.filter_call(verdict, c, u)
            assert rc == 1 and b"does not exist" in err() and (ptr, ln, nw) == (None, 0, 0)
        # ... and not looked at when it is not
        assert d.set_filtering(codes) == 0
        v = verdict.copy(); v[n_ok // 2] = 2; v[n_ok - 1] = 4
        bad_cell[n_ok // 2] = 0xFFFFFFFF
        got = d.filtered(v, bad_cell, bad_umi)
        dec = as_strings(v, np.where(bad_cell == 0xFFFFFFFF, 0, bad_cell), np.where(bad_umi == (ESC | len(SIDE)), 1, bad_umi), codes)
        assert got == fm.filtered_stream(recs, cfg, OUT, dec)[:2]
        # _tag_window after _filter_window: the -b bytes; a later _set_tagging turns filtering off, as NULL and a reset do
        assert d.tagged() == (b"".join(m for m in (tm.tagged_record(r, cfg, OUT) for r in recs) if m is not None), n_ok)
        assert L.dropest_bam_decoder_set_tagging(d.dec, C.byref(t)) == 0
        assert d.filter_call(verdict, cell, umi)[0] == 1 and b"filtering is not configured" in err()
        assert d.set_filtering(codes) == 0 and d.filtered(verdict, cell, umi) == good
        assert L.dropest_bam_decoder_set_filtering(d.dec, None) == 0
        assert d.filter_call(verdict, cell, umi)[0] == 1 and b"filtering is not configured" in err()
        assert d.set_filtering(codes) == 0
        assert L.dropest_bam_decoder_reset(d.dec, C.byref(d.cfg)) == 0
        d.window(comp, u0, 1)
        assert d.filter_call(verdict, cell, umi)[0] == 1 and b"not configured" in err()
    finally:
        d.close()
