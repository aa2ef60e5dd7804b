"""dropest_bam_decoder_filter_window_segments (include/dropest_bgzf.h; BamTagSegments in csrc/k_bamtag.h) through the C-ABI alone: the decisions of
a window's accepted records given in SEGMENTS, as the shards of a sharded run hold them -- device arrays (torch tensors), one triple per segment,
each with poisoned entries in front of and behind the segment's own (verdict 0, cell = n_cells: a look-up that is off by one raises the range
flag or changes bytes).  The bytes are tests/bam_filter_model.py's over the concatenated decisions and those of dropest_bam_decoder_filter_window
over the same decisions in one array: for one segment, cuts at the first and last accepted record and between unaccepted ones, empty segments
anywhere, a segment per record, 63 / 64 / 65 segments (one step of the table search and two), the record counts where the workgroup and the scan
tile end, two windows cut inside a record with a segment boundary at and off the window boundary, every segment through the staging; and what
the call refuses.

All cases run in ONE process of their own, as tests/test_gpu_annotation.py runs its tensors: torch brings the HIP runtime up first and the library
binds to the same one, so that a tensor's memory is memory the library's kernels may read.  The process prints one line per case; every case is
a test here."""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import traceback

import numpy as np
import pytest

torch = None                                     # (the child process imports it, first thing)

import bam_filter_model as fm
import bam_model as bm
from test_gpu_bam_filter_window import OUT, FilterDecoder, as_strings, bam_blob, decisions, model_cfg, small_records, tables
from test_gpu_bam_tag_window import block_starts, make_records, parse_cfg, tag_cfg

pytestmark = pytest.mark.gpu
P = C.POINTER
PAD = 3
GOOD_UMI = fm.pack_code(b"ACGTACGT")


class Segment(C.Structure):
    _fields_ = [("count", C.c_uint64), ("verdict", C.c_void_p), ("cell", C.c_void_p), ("umi", C.c_void_p), ("device", C.c_int32)]


def poisoned(values, lo, hi, poison):
    """values[lo:hi] on the device with PAD poisoned entries on either side -> (the tensor, the address of entry lo)"""
    host = np.concatenate([np.full(PAD, poison, values.dtype), values[lo:hi], np.full(PAD, poison, values.dtype)])
    signed = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}[host.dtype]
    t = torch.from_numpy(host.view(signed)).cuda()
    return t, t.data_ptr() + PAD * host.dtype.itemsize


class SegmentDecoder(FilterDecoder):
    def __init__(self, cfg):
        super().__init__(cfg)
        self.L.dropest_bam_decoder_filter_window_segments.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, P(C.c_void_p), P(C.c_uint64), P(C.c_uint64)]

    def segment_call(self, segs):
        ptr, ln, nw = C.c_void_p(), C.c_uint64(), C.c_uint64()
        arr = (Segment * max(1, len(segs)))(*segs)
        rc = self.L.dropest_bam_decoder_filter_window_segments(self.dec, C.byref(arr) if segs else None, len(segs), C.byref(ptr), C.byref(ln), C.byref(nw))
        return rc, ptr.value, ln.value, nw.value

    def segments_of(self, cuts, verdict, cell, umi, n_cells, null_empty=True):
        """cuts = ascending bounds [0, ..., n]: segment s holds decisions [cuts[s], cuts[s + 1]) in tensors of its own"""
        segs, keep = [], []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            if lo == hi and null_empty:
                segs.append(Segment(0, None, None, None, 0))
                continue
            (tv, pv), (tc, pc), (tu, pu) = poisoned(verdict, lo, hi, 0), poisoned(cell, lo, hi, n_cells), poisoned(umi, lo, hi, GOOD_UMI)
            keep += [tv, tc, tu]
            segs.append(Segment(hi - lo, pv, pc, pu, 0))
        torch.cuda.synchronize()
        return segs, keep

    def filtered_segments(self, cuts, verdict, cell, umi, n_cells, null_empty=True):
        segs, keep = self.segments_of([int(c) for c in cuts], verdict, cell, umi, n_cells, null_empty)
        rc, ptr, ln, nw = self.segment_call(segs)
        assert rc == 0, self.L.dropest_bgzf_last_error()
        assert (ptr is None) == (ln == 0)
        buf = np.zeros(ln + 1, np.uint8)
        assert self.L.dropest_bam_decoder_tagged_to_host(self.dec, buf.ctypes.data, ln) == 0, self.L.dropest_bgzf_last_error()
        del keep
        return buf[:ln].tobytes(), nw


def configure(d, codes, reset=True):
    L = d.L
    if reset:
        assert L.dropest_bam_decoder_reset(d.dec, C.byref(d.cfg)) == 0
    t = tag_cfg(OUT)
    assert L.dropest_bam_decoder_set_tagging(d.dec, C.byref(t)) == 0, L.dropest_bgzf_last_error()
    assert d.set_filtering(codes) == 0, L.dropest_bgzf_last_error()


class Big:
    """3 000 varied records in one decoded window, their decisions, the model's bytes (computed once) and the one-array call's"""


def make_big(tmp):
    b = Big()
    b.cfg = model_cfg(True)
    b.recs = make_records(True, False, seed=6)
    b.ok = [bm.parse_record(r, b.cfg, bm.Dicts(chr_of_ref=[0] * 4)).status == bm.OK for r in b.recs]
    b.n_ok = sum(b.ok)
    b.codes = tables(11)
    b.verdict, b.cell, b.umi = decisions(13, b.n_ok, len(b.codes))
    b.want, b.want_n, used = fm.filtered_stream(b.recs, b.cfg, OUT, as_strings(b.verdict, b.cell, b.umi, b.codes))
    assert used == b.n_ok and b.want_n == int((b.verdict == 0).sum()) > b.n_ok // 4
    b.comp, b.u0 = bam_blob(tmp, b.recs, 997)
    b.d = SegmentDecoder(parse_cfg(b.cfg))
    configure(b.d, b.codes, reset=False)
    w = b.d.window(b.comp, b.u0, 1)
    assert w.n_accepted == b.n_ok
    b.one_array = b.d.filtered(b.verdict, b.cell, b.umi)
    assert b.one_array == (b.want, b.want_n)
    return b


def between_unaccepted(ok):
    """an accepted rank k whose record follows a run of unaccepted records that follows accepted record k - 1, with unaccepted records behind it too"""
    rank = np.cumsum([0] + [int(x) for x in ok])
    for i in range(2, len(ok) - 2):
        if ok[i] and not ok[i - 1] and not ok[i - 2] and not ok[i + 1] and rank[i] > 0:
            return int(rank[i])
    for i in range(2, len(ok) - 1):
        if ok[i] and not ok[i - 1] and not ok[i - 2] and rank[i] > 0:
            return int(rank[i])
    raise AssertionError("no accepted record behind two unaccepted ones")


def big_cuts(b):
    n, k = b.n_ok, between_unaccepted(b.ok)
    m = n // 3
    return {
        "one segment": [0, n],
        "behind the first accepted record": [0, 1, n],
        "in front of the last": [0, n - 1, n],
        "between unaccepted records": [0, k, n],
        "behind the record in front of them": [0, k - 1, k, k + 1, n],
        "empty first": [0, 0, m, n],
        "empty last": [0, m, n, n],
        "empty in the middle": [0, m, m, n],
        "two empty in a row": [0, m, m, m, n],
        "empty everywhere": [0, 0, 0, m, m, m, 2 * m, n, n],
        "63 segments": np.linspace(0, n, 64).astype(int).tolist(),
        "64 segments": np.linspace(0, n, 65).astype(int).tolist(),
        "65 segments": np.linspace(0, n, 66).astype(int).tolist(),
        "64 empty segments, then one": [0] * 65 + [n],
        "one, then 130 empty segments": [0] + [n] * 131,
    }


CUT_NAMES = ["one segment", "behind the first accepted record", "in front of the last", "between unaccepted records", "behind the record in front of them", "empty first",
             "empty last", "empty in the middle", "two empty in a row", "empty everywhere", "63 segments", "64 segments", "65 segments", "64 empty segments, then one",
             "one, then 130 empty segments"]


def case_segments_give_the_bytes_of_one_array(big, tmp, name):
    cuts = big_cuts(big)
    assert sorted(cuts) == sorted(CUT_NAMES)
    c = cuts[name]
    assert c[0] == 0 and c[-1] == big.n_ok and all(a <= b for a, b in zip(c[:-1], c[1:])) and len(c) - 1 == {"63 segments": 63, "64 segments": 64, "65 segments": 65}.get(name, len(c) - 1)
    got = big.d.filtered_segments(c, big.verdict, big.cell, big.umi, len(big.codes))
    assert got[1] == big.want_n and len(got[0]) == len(big.want)
    assert got == (big.want, big.want_n) == big.one_array
    if "empty" in name:                              # an empty segment may bring pointers as well: they are not looked at
        assert big.d.filtered_segments(c, big.verdict, big.cell, big.umi, len(big.codes), null_empty=False) == got


def case_the_poison_is_seen_by_a_lookup_that_is_off_by_one(big, tmp):
    """what the padding is for: decisions shifted by one entry inside a segment either name the cell that does not exist or change the bytes"""
    n, m = big.n_ok, big.n_ok // 2
    segs, keep = big.d.segments_of([0, m, n], big.verdict, big.cell, big.umi, len(big.codes))
    for shift in (-1, 1):
        s = Segment(segs[1].count, segs[1].verdict + shift, segs[1].cell + 4 * shift, segs[1].umi + 8 * shift, 0)
        rc, ptr, ln, nw = big.d.segment_call([segs[0], s])
        if rc == 0:
            buf = np.zeros(ln + 1, np.uint8)
            assert big.d.L.dropest_bam_decoder_tagged_to_host(big.d.dec, buf.ctypes.data, ln) == 0
            assert buf[:ln].tobytes() != big.want
        else:
            assert rc == 1 and b"does not exist" in big.d.L.dropest_bgzf_last_error() and (ptr, ln, nw) == (None, 0, 0)
    assert big.d.segment_call(segs)[0] == 0
    del keep


def case_a_segment_per_accepted_record(big, tmp_path):
    cfg = model_cfg(True)
    recs = small_records(300, 40)
    comp, u0 = bam_blob(tmp_path, recs, 60_000)
    codes = tables(3, n_cells=20)
    d = SegmentDecoder(parse_cfg(cfg))
    try:
        configure(d, codes, reset=False)
        n_ok = d.window(comp, u0, 1).n_accepted
        assert 200 < n_ok < 300                                                   # four steps of the table search and part of a fifth
        verdict, cell, umi = decisions(31, n_ok, len(codes))
        want = fm.filtered_stream(recs, cfg, OUT, as_strings(verdict, cell, umi, codes))[:2]
        assert d.filtered_segments(range(n_ok + 1), verdict, cell, umi, len(codes)) == want == d.filtered(verdict, cell, umi)
    finally:
        d.close()


def case_the_edges_of_the_workgroup_and_the_scan_tile(big, tmp_path, n_rec):
    cfg = model_cfg(True)
    codes = tables(3, n_cells=20)
    d = SegmentDecoder(parse_cfg(cfg))
    try:
        for head in (0, 1 if n_rec == 1 else max(1, n_rec // 3)):
            recs = small_records(n_rec, head)
            comp, u0 = bam_blob(tmp_path, recs, 60_000)
            configure(d, codes)
            n_ok = d.window(comp, u0, 1).n_accepted
            ok = [i >= head and i % 7 != 3 for i in range(n_rec)]
            assert n_ok == sum(ok)
            verdict, cell, umi = decisions(n_rec + head, n_ok, len(codes))
            cell[(verdict != 1) & (verdict != 2) & (cell == 0xFFFFFFFF)] = 7
            want = fm.filtered_stream(recs, cfg, OUT, as_strings(verdict, cell, umi, codes))[:2]
            # the ranks of the last record of the first scan tile and of the first record of the second; the middle; no cut at all
            rank = np.cumsum([0] + [int(x) for x in ok])
            inner = sorted({int(rank[min(n_rec, k)]) for k in (4095, 4096)} | {n_ok // 2})
            for cuts in ([0] + inner + [n_ok], [0, n_ok], [0, n_ok // 2, n_ok]):
                assert d.filtered_segments(cuts, verdict, cell, umi, len(codes)) == want
            assert d.filtered(verdict, cell, umi) == want
    finally:
        d.close()


def shard_pieces(bounds, at, n):
    """the host's rule (bam_device.cpp, filter_window): the window [at, at + n) cut at the shards' range boundaries -> the cuts relative to the window"""
    cuts = [0]
    for first, end in zip(bounds[:-1], bounds[1:]):
        lo, hi = max(at, first), min(at + n, end)
        if lo <= hi:
            cuts.append(hi - at)
    return cuts


def case_two_windows_cut_inside_a_record(big, tmp_path, at_the_window_boundary):
    b = big
    d = SegmentDecoder(parse_cfg(b.cfg))
    try:
        configure(d, b.codes, reset=False)
        starts = block_starts(b.comp.tobytes())
        cut = starts[len(starts) // 2]
        first, second = b.comp[:cut].copy(), b.comp[cut:].copy()
        w1 = d.window(first, b.u0, 0)
        assert w1.tail_bytes > 0                                                  # the record the cut went through waits inside the decoder
        n1 = w1.n_accepted
        assert 0 < n1 < b.n_ok
        # three "shards": their middle boundary at the window boundary, or 5 decisions in front of it (the second window then begins inside a shard)
        bounds = [0, n1 // 2, n1 if at_the_window_boundary else n1 - 5, b.n_ok - 7, b.n_ok]
        c1 = shard_pieces(bounds, 0, n1)
        assert c1[-1] == n1 and len(c1) == 4 and (c1[2] == n1) == at_the_window_boundary      # (at the boundary: the shard that begins there touches the window, empty)
        g1 = d.filtered_segments(c1, b.verdict[:n1], b.cell[:n1], b.umi[:n1], len(b.codes))
        w2 = d.window(second, 0, 1)
        n2 = w2.n_accepted
        assert n1 + n2 == b.n_ok
        c2 = shard_pieces(bounds, n1, n2)
        assert c2[-1] == n2 and (c2[1] == 0) == at_the_window_boundary            # (at the boundary: the shard that ends there touches the window, empty)
        g2 = d.filtered_segments(c2, b.verdict[n1:], b.cell[n1:], b.umi[n1:], len(b.codes))
        assert g1[1] + g2[1] == b.want_n and g1[0] + g2[0] == b.want
        assert g2 == d.filtered(b.verdict[n1:], b.cell[n1:], b.umi[n1:])
    finally:
        d.close()


def case_every_segment_through_the_staging(big, tmp):
    n = big.n_ok
    cuts = [0, n // 3, n // 3 + 1, n]
    os.environ["DROPEST_BAM_TEST_STAGE_SEGMENTS"] = "1"          # (read by the library at every call)
    try:
        staged = big.d.filtered_segments(cuts, big.verdict, big.cell, big.umi, len(big.codes))
    finally:
        del os.environ["DROPEST_BAM_TEST_STAGE_SEGMENTS"]
    assert staged == (big.want, big.want_n) == big.d.filtered_segments(cuts, big.verdict, big.cell, big.umi, len(big.codes))


def case_what_the_call_refuses(big, tmp_path):
    cfg = model_cfg(True)
    recs = small_records(50, 2)
    comp, u0 = bam_blob(tmp_path, recs, 60_000)
    codes = tables(3, n_cells=20)
    d = SegmentDecoder(parse_cfg(cfg))
    L = d.L
    err = L.dropest_bgzf_last_error
    try:
        n_ok = d.window(comp, u0, 1).n_accepted
        verdict, cell, umi = np.zeros(n_ok, np.uint8), np.full(n_ok, 3, np.uint32), np.full(n_ok, GOOD_UMI, np.uint64)
        segs, keep = d.segments_of([0, 10, n_ok], verdict, cell, umi, len(codes))
        # neither configured, then tagging alone: the window is not filtered
        assert d.segment_call(segs)[0] == 1 and b"tagging is not configured" in err()
        t = tag_cfg(OUT)
        assert L.dropest_bam_decoder_set_tagging(d.dec, C.byref(t)) == 0
        assert d.segment_call(segs) == (1, None, 0, 0) and b"filtering is not configured" in err()
        assert d.set_filtering(codes) == 0, err()
        want = fm.filtered_stream(recs, cfg, OUT, as_strings(verdict, cell, umi, codes))[:2]
        assert d.filtered_segments([0, 10, n_ok], verdict, cell, umi, len(codes)) == want
        # the counts sum to the window's accepted count: in the words of the one-array call's check
        for counts in ((10, n_ok - 11), (10, n_ok - 9), (n_ok + 1, 0), (2 ** 64 - 1, 2)):
            bad = [Segment(counts[0], segs[0].verdict, segs[0].cell, segs[0].umi, 0), Segment(counts[1], segs[1].verdict, segs[1].cell, segs[1].umi, 0)]
            assert d.segment_call(bad) == (1, None, 0, 0) and b"decisions for a window of %d accepted records" % n_ok in err()
        assert d.filter_call(verdict, cell, umi, n=n_ok - 1)[0] == 1 and b"decisions for a window of %d accepted records" % n_ok in err()
        # no segment at all for a window with accepted records
        assert d.segment_call([]) == (1, None, 0, 0) and b"0 decisions for a window" in err()
        # a segment that is not empty without one of its arrays; segments without a table
        for k in range(3):
            p = [segs[1].verdict, segs[1].cell, segs[1].umi]
            p[k] = None
            assert d.segment_call([segs[0], Segment(segs[1].count, p[0], p[1], p[2], 0)]) == (1, None, 0, 0) and b"null argument" in err()
        ptr, ln, nw = C.c_void_p(), C.c_uint64(), C.c_uint64()
        assert L.dropest_bam_decoder_filter_window_segments(d.dec, None, 2, C.byref(ptr), C.byref(ln), C.byref(nw)) == 1 and b"null argument" in err()
        # a decision that names a cell that does not exist, in the second segment
        bad_cell = cell.copy(); bad_cell[n_ok - 2] = len(codes)
        bsegs, bkeep = d.segments_of([0, 10, n_ok], verdict, bad_cell, umi, len(codes))
        assert d.segment_call(bsegs) == (1, None, 0, 0) and b"does not exist" in err()
        # ... and the call still works afterwards; filtering turned off again is refused
        assert d.filtered_segments([0, 10, n_ok], verdict, cell, umi, len(codes)) == want
        assert L.dropest_bam_decoder_set_filtering(d.dec, None) == 0
        assert d.segment_call(segs)[0] == 1 and b"filtering is not configured" in err()
        del keep, bkeep
    finally:
        d.close()


# ---- the cases by name; the child process that runs them; the tests that read its lines ------------------------------------------------------------
def _cases():
    out = {"segments[%s]" % n: (lambda big, tmp, n=n: case_segments_give_the_bytes_of_one_array(big, tmp, n)) for n in CUT_NAMES}
    out["the poison is seen by a look-up that is off by one"] = case_the_poison_is_seen_by_a_lookup_that_is_off_by_one
    out["a segment per accepted record"] = case_a_segment_per_accepted_record
    for n_rec in (1, 4, 5, 4096, 4097):
        out["edges of the workgroup and the scan tile[%d]" % n_rec] = lambda big, tmp, n=n_rec: case_the_edges_of_the_workgroup_and_the_scan_tile(big, tmp, n)
    out["two windows, a segment boundary at the window boundary"] = lambda big, tmp: case_two_windows_cut_inside_a_record(big, tmp, True)
    out["two windows, a segment boundary inside the first window"] = lambda big, tmp: case_two_windows_cut_inside_a_record(big, tmp, False)
    out["every segment through the staging"] = case_every_segment_through_the_staging
    out["what the call refuses"] = case_what_the_call_refuses
    return out


CASES = _cases()


def _child(tmp_root):
    """every case, one line each on stdout: CASE <tab> name <tab> OK | FAILED; a failure's traceback on stderr"""
    global torch
    import pathlib
    import torch as _torch
    torch = _torch
    torch.cuda.init()
    big = make_big(pathlib.Path(tempfile.mkdtemp(dir=tmp_root)))
    for name, case in CASES.items():
        try:
            case(big, pathlib.Path(tempfile.mkdtemp(dir=tmp_root)))
            print("CASE\t%s\tOK" % name, flush=True)
        except Exception:                                              # (an assertion, or an error of torch's or ctypes')
            print("CASE\t%s\tFAILED" % name, flush=True)
            sys.stderr.write("---- %s\n%s\n" % (name, traceback.format_exc()))
    big.d.close()


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, os.path.abspath(__file__), str(tmp_path_factory.mktemp("segments"))], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", "")))
    lines = [line.split("\t") for line in res.stdout.splitlines() if line.startswith("CASE\t")]
    return {name: verdict for _, name, verdict in lines}, res


@pytest.mark.parametrize("name", list(CASES))
def test_segments(child, name):
    results, res = child
    assert results.get(name) == "OK", "%s: %s\n%s%s" % (name, results.get(name, "did not run (exit status %d)" % res.returncode), res.stdout[-2000:], res.stderr[-6000:])


if __name__ == "__main__":
    _child(sys.argv[1])
