"""dropest_bam_decoder_tag_window / _filter_window / _filter_window_segments on a decoder with sources (include/dropest_bgzf.h; SRCS in
csrc/k_bamtag.h) through the C-ABI alone: under -r (dropest_bam_decoder_set_read_params) the raw barcode, raw UMI and UMI quality of a written
record are the served row's fields, under -P (dropest_bam_decoder_set_gene_of_reference + _set_reference_names) the gene is the reference's name.
The bytes are tests/bam_tag_sources_model.py's -- over one window, two windows (both window orders), windows of 3 .. 257 records, a replay
(dropest_read_params_replay_begin / _end), and synthetic -F decisions as one array and in segments."""
import ctypes as C

import numpy as np
import pytest

import bam_filter_model as fm
import bam_model as bm
import bam_tag_sources_model as sm
import bam_writer as bw
import read_params_model as rp
from test_gpu_bam_decoder_cabi import Window
from test_gpu_bam_filter_segments import Segment
from test_gpu_bam_filter_window import FilterDecoder, as_strings, decisions, tables
from test_gpu_bam_tag_window import block_starts, first_record, parse_cfg, tag_cfg
from test_gpu_read_params_table import Table, lib as table_lib

pytestmark = pytest.mark.gpu
P = C.POINTER

# reference names of 1, 64, 65 and 0 characters, and a fifth one that a short table of names leaves out
REF_NAMES = [b"7", b"c" * 64, b"d" * 65, b"", b"extra"]
REFS = [(n.decode(), 1 << 20) for n in REF_NAMES]
CFG = bm.Cfg(tags=("CB", "UB", "CQ", "UQ", "GX", "RE"), filled_bam=False, min_phred=53, read_type=True, intronic=b"N", intergenic=b"I", n_refs=len(REFS))
OUT = fm.FilterOutCfg(read_type="RE", exonic=b"E", intronic=b"N", intergenic=b"I")
LENGTHS = (1, 63, 64, 65, 200)
DUPS = {11: 10, 64: 63, 301: 300, 650: 20, 655: 26, 660: 256}      # record -> the earlier record whose name it carries (inside a window, across two)
N = 700


def make_stream(seed=7):
    """N records and the two parameter texts (one per _add_text call).  Names are "q<i>!CB#UMI" so that -P alone can read them; under -r the
    name's barcode and UMI must not reach the output."""
    rng = np.random.default_rng(seed)
    recs, lines = [], [[], []]
    names = {}
    for i in range(N):
        base = b"q%d!ACGTAC#TTGA" % i if i % 29 != 4 else b"q%d-no-separators" % i
        if i in DUPS:
            base = names[DUPS[i]]
        names[i] = base
        at_kind = i % 4                                               # '@' on neither, on the row, on the record, on both
        tags = []
        if i % 5 == 0:
            tags.append(("CR", "Z", "OLDOLD"))
        if i % 3:
            tags.append(("GX", "Z", "GENE%d" % (i % 40)))
            if i % 4:
                tags.append(("RE", "A" if i % 8 < 4 else "Z", "NIE"[i % 3]))
        if i % 6 == 1:
            tags.append(("UR", "i", 77))
        tags.append(("NH", "i", i))
        if i % 8 == 2:
            tags.append(("UQ", "Z", "####"))
        if i % 9 == 3:
            tags.append(("CQ", "Z", "FFFF"))                          # never edited under -r
        if i % 23 == 9:
            tags.append(b"QQ?" + b"CRZbehind the stop\x00")           # the walk stops early: this CR stays
        flag, ref = 0, (i % 4 if i % 41 else 4)
        if i % 53 == 5:
            flag = 4
        elif i % 53 == 6:
            ref = -1
        recs.append(bw.record(ref, i, (b"@" if at_kind >= 2 else b"") + base, flag=flag, seq="ACGT" * 6, tags=tags))
        if i in DUPS or i % 17 == 6:
            continue                                                  # no row of its own
        cb = bytes(rng.choice(list(b"ACGT"), LENGTHS[i % 5]).tolist())
        umi = bytes(rng.choice(list(b"ACGT"), LENGTHS[(i // 5) % 5]).tolist())
        q = bytes(rng.integers(53, 74, LENGTHS[(i // 25) % 5], dtype=np.uint8).tolist())
        if i % 7 == 2:
            cb = b"N" + cb[1:]
        if i % 7 == 4:
            umi = umi.lower()
        if i % 11 == 3:
            q = b""
        cq = b"I" * min(len(cb), 12)
        if i % 19 == 7:
            cq = b"+" + cq[1:]                                        # low quality: the row is taken, the record not written
        line = (b"@" if at_kind in (1, 3) else b"") + base + b" " + cb + b" " + umi + b" " + cq + b" " + q + (b"\r\n" if i % 13 == 5 else b"\n")
        lines[i % 2].append(line)
    texts = [b"".join(ls[k] for k in rng.permutation(len(ls))) for ls in lines]
    return recs, texts


RECS, TEXTS = make_stream()


def model(recs, mode, decisions_=None, ref_names=REF_NAMES):
    server = rp.Server(rp.Rows(TEXTS, CFG.min_phred)) if "params" in mode else None
    return sm.stream(recs, CFG, OUT, server=server, ref_names=ref_names if "ref" in mode else None, decisions=decisions_)


def test_the_stream_holds_what_it_is_meant_to():
    """(on the expected side, so that no comparison below passes on an empty case)"""
    rows = rp.Rows(TEXTS, CFG.min_phred)
    first_call = len(rp.split_lines(TEXTS[0])[0])
    _, written, kinds = model(RECS, ("params", "ref"))
    hist = {k: kinds.count(k) for k in set(kinds)}
    assert written > 300 and hist[sm.NO_ROW] >= 20 and hist[sm.ROW_TAKEN] >= 6 and hist[sm.LOW_QUALITY] >= 20 and hist[sm.SKIPPED] >= 10
    served = [rows.lookup(sm.layout(r)[2]) for r, k in zip(RECS, kinds) if k == sm.WRITTEN]
    assert sum(1 for r in served if r < first_call) > 100 and sum(1 for r in served if r >= first_call) > 100      # rows of both _add_text calls
    for i, j in DUPS.items():
        assert kinds[i] == sm.ROW_TAKEN and kinds[j] in (sm.WRITTEN, sm.LOW_QUALITY), (i, j)
    assert any(kinds[j] == sm.LOW_QUALITY for j in DUPS.values())
    _, _, kinds_p = model(RECS, ("ref",))
    assert kinds_p.count(sm.NOT_PARSED) >= 20 and kinds_p.count(sm.WRITTEN) > 300


class DeviceArrays:
    """host arrays copied to device memory of the HIP runtime the library runs on (already loaded: not a copy another package brought along)"""

    def __init__(self):
        maps = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln]
        self.hip = C.CDLL(([m for m in maps if "-packages" not in m] or ["libamdhip64.so"])[0])
        self.hip.hipMalloc.argtypes = [P(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        self.held = []

    def put(self, values):
        values = np.ascontiguousarray(values)
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), max(values.nbytes, 16)) == 0
        self.held.append(p)
        if values.nbytes:
            assert self.hip.hipMemcpy(p, values.ctypes.data, values.nbytes, 1) == 0      # hipMemcpyHostToDevice
        return p.value

    def free(self):
        assert self.hip.hipDeviceSynchronize() == 0
        for p in self.held:
            self.hip.hipFree(p)
        self.held = []


class SourceDecoder(FilterDecoder):
    def __init__(self):
        super().__init__(parse_cfg(CFG))
        L = self.L
        L.dropest_bam_decoder_filter_window_segments.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, P(C.c_void_p), P(C.c_uint64), P(C.c_uint64)]
        table_lib()
        L.dropest_bam_decoder_set_read_params.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.dropest_bam_decoder_set_gene_of_reference.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.dropest_bam_decoder_set_reference_names.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        L.dropest_read_params_replay_begin.argtypes = [C.c_void_p]
        L.dropest_read_params_replay_end.argtypes = [C.c_void_p]
        self.t = tag_cfg(OUT)

    def err(self):
        return self.L.dropest_bgzf_last_error()

    def reference_names(self, names):
        off = np.cumsum([0] + [len(n) for n in names]).astype(np.uint32)
        pool = np.frombuffer(b"".join(names) + b"\0", np.uint8).copy()
        return self.L.dropest_bam_decoder_set_reference_names(self.dec, off.ctypes.data, pool.ctypes.data, len(names))

    def configure(self, mode, table, ordinal=0, names=REF_NAMES, tagging_first=True, codes=None):
        L = self.L
        assert L.dropest_bam_decoder_reset(self.dec, C.byref(self.cfg)) == 0, self.err()
        if tagging_first:                                             # a tagging decoder takes the sources, and a decoder with sources takes tagging
            assert L.dropest_bam_decoder_set_tagging(self.dec, C.byref(self.t)) == 0, self.err()
        if "params" in mode:
            assert L.dropest_bam_decoder_set_read_params(self.dec, table.h, ordinal) == 0, self.err()
        if "ref" in mode:
            g = np.array([-2 if not n else 10 + k for k, n in enumerate(REF_NAMES)], np.int32)
            assert L.dropest_bam_decoder_set_gene_of_reference(self.dec, g.ctypes.data, len(g)) == 0, self.err()
            if names is not None:
                assert self.reference_names(names) == 0, self.err()
        if not tagging_first:
            assert L.dropest_bam_decoder_set_tagging(self.dec, C.byref(self.t)) == 0, self.err()
        if codes is not None:
            assert self.set_filtering(codes) == 0, self.err()

    def filtered_segments(self, cuts, verdict, cell, umi):
        """filters the last window under decisions that stand in segments: segment s = entries [cuts[s], cuts[s + 1]) in device arrays of its own"""
        dev = DeviceArrays()
        segs = [Segment(hi - lo, dev.put(verdict[lo:hi]), dev.put(cell[lo:hi]), dev.put(umi[lo:hi]), 0) if hi > lo else Segment(0, None, None, None, 0)
                for lo, hi in zip(cuts[:-1], cuts[1:])]
        arr = (Segment * len(segs))(*segs)
        ptr, ln, nw = C.c_void_p(), C.c_uint64(), C.c_uint64()
        try:
            assert self.L.dropest_bam_decoder_filter_window_segments(self.dec, C.byref(arr), len(segs), C.byref(ptr), C.byref(ln), C.byref(nw)) == 0, self.err()
            buf = np.zeros(ln.value + 1, np.uint8)
            assert self.L.dropest_bam_decoder_tagged_to_host(self.dec, buf.ctypes.data, ln.value) == 0, self.err()
        finally:
            dev.free()
        return buf[:ln.value].tobytes(), nw.value

    def pipelined(self, a, b, u0, each):
        """the other window order: the inflate of window 2 is queued before window 1 is finished; each(k, window) after every finish"""
        L = self.L
        s1, s2, v1, v2 = C.c_int(-1), C.c_int(-1), Window(), Window()
        assert L.dropest_bam_decoder_window_inflate(self.dec, a.ctypes.data, len(a), C.byref(s1)) == 0, self.err()
        assert L.dropest_bam_decoder_window_inflate(self.dec, b.ctypes.data, len(b), C.byref(s2)) == 0, self.err()
        assert L.dropest_bam_decoder_window_chain(self.dec, s1.value, u0, 0, None, None) == 0, self.err()
        assert L.dropest_bam_decoder_window_finish(self.dec, s1.value, C.byref(v1)) == 0, self.err()
        r1 = each(0, v1)
        assert L.dropest_bam_decoder_window_chain(self.dec, s2.value, 0, 1, None, None) == 0, self.err()
        assert L.dropest_bam_decoder_window_finish(self.dec, s2.value, C.byref(v2)) == 0, self.err()
        return r1, each(1, v2)


def bam_blob(tmp_path, recs, block=4000):
    path = str(tmp_path / "s.bam")
    bw.write_bam(path, REFS, recs, block=block)
    blob = open(path, "rb").read()
    c0, u0 = first_record(blob)
    return np.frombuffer(blob[c0:], np.uint8), u0


def claims(L, t):
    n = len(rp.Rows(TEXTS, 0).rows)
    out = np.zeros(n, np.uint64)
    assert L.dropest_read_params_claims_to_host(t.h, 0, n, out.ctypes.data) == 0, L.dropest_bgzf_last_error()
    return out


@pytest.mark.parametrize("mode", [("params",), ("ref",), ("params", "ref")], ids=["r", "P", "r+P"])
def test_tagged_windows_equal_the_model(tmp_path, mode):
    want, want_n, kinds = model(RECS, mode)
    assert want_n > 300
    comp, u0 = bam_blob(tmp_path, RECS)
    starts = block_starts(comp.tobytes())
    cut = starts[len(starts) * 8 // 10]
    a, b = comp[:cut].copy(), comp[cut:].copy()
    d = SourceDecoder()
    L = d.L
    t = Table(L, TEXTS, CFG.min_phred)
    try:
        # 1. one window; the tagging configuration given first
        d.configure(mode, t, 1000)
        w = d.window(comp, u0, 1)
        assert w.n_records == N and w.n_accepted == want_n
        got, n = d.tagged()
        assert n == want_n and len(got) == len(want) and got == want
        assert d.tagged() == (got, n)
        # 2. two windows, the sources given first: names of the first are aligned again in the second
        assert L.dropest_read_params_reset_claims(t.h) == 0
        d.configure(mode, t, 1000, tagging_first=False)
        w1 = d.window(a, u0, 0)
        g1, n1 = d.tagged()
        w2 = d.window(b, 0, 1)
        g2, n2 = d.tagged()
        assert 301 < w1.n_records < 650 < w1.n_records + w2.n_records == N and n1 > 0 and n2 > 0
        assert n1 + n2 == want_n and g1 + g2 == want
        # 3. the other window order
        assert L.dropest_read_params_reset_claims(t.h) == 0
        d.configure(mode, t, 1000)
        assert d.pipelined(a, b, u0, lambda k, v: d.tagged()) == ((g1, n1), (g2, n2))
        if "params" not in mode:
            return
        # 4. a replay: the same windows from ordinal 0 on a claim array of its own -- the same bytes, and the claims come back as they were
        before = claims(L, t)
        assert (before != 0xFFFFFFFFFFFFFFFF).sum() > 300 and before[before != 0xFFFFFFFFFFFFFFFF].min() >= 1000
        assert L.dropest_read_params_replay_end(t.h) != 0 and b"not in a replay" in d.err()
        assert L.dropest_read_params_replay_begin(t.h) == 0, d.err()
        assert L.dropest_read_params_replay_begin(t.h) != 0 and b"in a replay already" in d.err()
        assert (claims(L, t) == 0xFFFFFFFFFFFFFFFF).all()
        d.configure(mode, t, 0)
        d.window(a, u0, 0)
        r1 = d.tagged()
        d.window(b, 0, 1)
        r2 = d.tagged()
        during = claims(L, t)
        assert ((during == 0xFFFFFFFFFFFFFFFF) == (before == 0xFFFFFFFFFFFFFFFF)).all() and (during[during != 0xFFFFFFFFFFFFFFFF] + 1000 == before[before != 0xFFFFFFFFFFFFFFFF]).all()
        assert L.dropest_read_params_replay_end(t.h) == 0, d.err()
        assert (r1, r2) == ((g1, n1), (g2, n2))
        assert (claims(L, t) == before).all()
        # ... and the ingest's claims still hold: the same windows above them serve nobody
        d.configure(mode, t, 5000)
        d.window(comp, u0, 1)
        assert d.tagged() == (b"", 0)
    finally:
        d.close()
        t.close()


@pytest.mark.parametrize("n_rec", [3, 4, 5, 255, 256, 257])
def test_the_edges_of_the_workgroup_and_the_scan(tmp_path, n_rec):
    """four records per workgroup, 256 lanes of 16 records in the scans: windows that end just before, at and just behind them; -b and -F"""
    recs = RECS[8:8 + n_rec]                                          # (from a record with a row on: a window of 3 writes something)
    mode = ("params", "ref")
    want, want_n, kinds = model(recs, mode)
    assert want_n >= 2
    n_ok = sm.accepted(kinds)
    codes = tables(3, n_cells=20)
    verdict, cell, umi = decisions(n_rec, n_ok, len(codes))
    verdict[0] = 0
    cell[(verdict != 1) & (verdict != 2) & (cell == 0xFFFFFFFF)] = 7
    want_f, want_fn, kinds_f = model(recs, mode, as_strings(verdict, cell, umi, codes))
    assert want_fn == int((verdict == 0).sum()) and sm.accepted(kinds_f) == n_ok
    comp, u0 = bam_blob(tmp_path, recs, block=60_000)
    d = SourceDecoder()
    t = Table(d.L, TEXTS, CFG.min_phred)
    try:
        d.configure(mode, t, 0, codes=codes)
        w = d.window(comp, u0, 1)
        assert w.n_records == n_rec and w.n_accepted == n_ok
        assert d.tagged() == (want, want_n)
        assert d.filtered(verdict, cell, umi) == (want_f, want_fn)
        assert d.filtered_segments([0, n_ok // 2, n_ok], verdict, cell, umi) == (want_f, want_fn)
    finally:
        d.close()
        t.close()


@pytest.mark.parametrize("mode", [("params",), ("params", "ref")], ids=["r", "r+P"])
def test_filtered_windows_equal_the_model(tmp_path, mode):
    """-F over synthetic decisions, as one array and in segments (one of them empty), over two windows in both orders"""
    _, _, kinds = model(RECS, mode)
    n_ok = sm.accepted(kinds)
    codes = tables(11)
    verdict, cell, umi = decisions(21, n_ok, len(codes))
    assert (verdict == 0).sum() * 3 >= n_ok and all((verdict == v).any() for v in range(5))
    cell[(verdict != 1) & (verdict != 2) & (cell == 0xFFFFFFFF)] = 7
    want, want_n, _ = model(RECS, mode, as_strings(verdict, cell, umi, codes))
    assert want_n == int((verdict == 0).sum()) > 100
    comp, u0 = bam_blob(tmp_path, RECS)
    starts = block_starts(comp.tobytes())
    cut = starts[len(starts) * 8 // 10]
    a, b = comp[:cut].copy(), comp[cut:].copy()
    d = SourceDecoder()
    L = d.L
    t = Table(L, TEXTS, CFG.min_phred)
    try:
        d.configure(mode, t, 0, codes=codes)
        w = d.window(comp, u0, 1)
        assert w.n_accepted == n_ok
        got = d.filtered(verdict, cell, umi)
        assert got[1] == want_n and len(got[0]) == len(want) and got[0] == want
        assert d.filtered_segments([0, n_ok // 3, n_ok // 3, n_ok - 1, n_ok], verdict, cell, umi) == got
        assert d.tagged() == model(RECS, mode)[:2]                    # the -b bytes of the same window afterwards
        # two windows: the second window's decisions begin at the first's accepted count
        assert L.dropest_read_params_reset_claims(t.h) == 0
        d.configure(mode, t, 0, codes=codes)
        w1 = d.window(a, u0, 0)
        n1 = int(w1.n_accepted)
        g1 = d.filtered(verdict[:n1], cell[:n1], umi[:n1])
        w2 = d.window(b, 0, 1)
        assert n1 + w2.n_accepted == n_ok and 0 < n1 < n_ok
        g2 = d.filtered_segments([0, 1, n_ok - n1], verdict[n1:], cell[n1:], umi[n1:])
        assert g1[0] + g2[0] == want and g1[1] + g2[1] == want_n

        def each(k, v):
            return d.filtered_segments([0, n1 // 2, n1], verdict[:n1], cell[:n1], umi[:n1]) if k == 0 else d.filtered(verdict[n1:], cell[n1:], umi[n1:])
        assert L.dropest_read_params_reset_claims(t.h) == 0
        d.configure(mode, t, 0, codes=codes)
        assert d.pipelined(a, b, u0, each) == (g1, g2)
    finally:
        d.close()
        t.close()


def test_reference_names_are_needed_and_checked(tmp_path):
    """-P: without the names the call says which call is missing; a record on a reference the names do not reach is flagged, not loaded"""
    recs = RECS[:60]
    assert any(sm.layout(r)[0] == 4 and sm.read(r, CFG)[0] == sm.WRITTEN for r in recs)
    comp, u0 = bam_blob(tmp_path, recs, block=60_000)
    d = SourceDecoder()
    L = d.L
    ptr, ln, n = C.c_void_p(), C.c_uint64(), C.c_uint64()
    try:
        d.configure(("ref",), None, names=None)
        d.window(comp, u0, 1)
        assert L.dropest_bam_decoder_tag_window(d.dec, C.byref(ptr), C.byref(ln), C.byref(n)) == 1 and b"dropest_bam_decoder_set_reference_names" in d.err()
        assert d.reference_names(REF_NAMES[:4]) == 0, d.err()          # reference 4 = the table's size
        assert L.dropest_bam_decoder_tag_window(d.dec, C.byref(ptr), C.byref(ln), C.byref(n)) == 1 and b"a reference that does not exist" in d.err()
        assert ptr.value is None and ln.value == 0 and n.value == 0
        assert d.reference_names(REF_NAMES) == 0, d.err()
        assert d.tagged() == model(recs, ("ref",))[:2]
        short = [x for x in REF_NAMES]
        short[0] = b"another"
        assert d.reference_names(short) == 0
        assert d.tagged() == model(recs, ("ref",), ref_names=short)[:2]
    finally:
        d.close()
