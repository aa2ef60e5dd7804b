"""The device BAM decoder (include/dropest_bgzf.h: dropest_bam_decoder_*) record by record against the reference model (tests/bam_model.py), on fuzzed
files that mix every record shape the walk and the tag parse must handle: every tag type and B subtype, repeated and numeric-first tags, unknown
types and values cut short, empty strings, quality bytes >= 0x80 or equal to the minimum, read names with several '!' / '#', barcodes of 31 / 32
bases, lowercase or high bytes, flags 0x800 / 0x4 / 0x100, ref_id == n_refs, records beyond a 16 KB segment and a 20 KB wave stage, payloads
that look like chains of records.  The files are cut into windows of several sizes and run through the window call, its _begin / _finish halves
and the pipelined _inflate / _chain / _finish order.  Also: records beyond 2^26 bytes, UMI quality strings beyond 65 535 bytes, and the same
files through the whole reader (host bulk, record by record, device) against the oracle."""
import ctypes as C
import gzip
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

import bam_model as bm      # noqa: E402
import bam_writer as bw     # noqa: E402

pytestmark = pytest.mark.gpu
P = C.POINTER
TAGS = ("CB", "UB", "CQ", "UQ", "GX", "RE")       # the reader's defaults (BamTags.cpp:7-24) and tests/cpp/bam_to_counts' read type
N_REFS = 6
REFS = [("chr%d" % i, 1 << 24) for i in range(N_REFS)]
GENES = [b"G%d" % i for i in range(60)] + [b"ENSG00000%06d" % i for i in range(40)]


class Cfg(C.Structure):
    _fields_ = [("tag", C.c_uint16 * 6), ("filled_bam", C.c_int32), ("min_phred", C.c_int32), ("has_read_type", C.c_int32), ("n_refs", C.c_int32),
                ("intronic_len", C.c_uint32), ("intergenic_len", C.c_uint32), ("intronic", C.c_uint8 * 24), ("intergenic", C.c_uint8 * 24)]


class Window(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("counts", C.c_uint64 * 5), ("n_accepted", C.c_uint64), ("d_cb", C.c_void_p), ("d_umi", C.c_void_p), ("d_gene", C.c_void_p),
                ("d_aux", C.c_void_p), ("n_need", C.c_uint32), ("need_rec", P(C.c_uint32)), ("need_pos", P(C.c_uint32)), ("need_size", P(C.c_uint32)),
                ("quality_seen", C.c_uint32), ("any_gene", C.c_uint32), ("window_bytes", C.c_uint64), ("tail_bytes", C.c_uint64), ("n_blocks", C.c_uint32),
                ("refused_blocks", C.c_uint32), ("guesses_repaired", C.c_uint32), ("pad", C.c_uint32), ("ms", C.c_double * 4), ("quality_len_min", C.c_uint32), ("quality_len_max", C.c_uint32)]


# ---- the fuzzed records ------------------------------------------------------------------------------------------------------------------
def _bases(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), n)) if n else ""


def _fake_chain(rng, n):
    """n small, well-formed records one after the other: bytes that look like the record chain to a guess made inside them"""
    return b"".join(bw.record(int(rng.integers(0, N_REFS)), 5, "fake%d" % k, seq="ACGT", tags=[("CB", "Z", "AAAA"), ("UB", "Z", "CC")]) for k in range(n))


def fuzz_records(seed, n, big=True, printable=False):
    """n records from `seed`.  big: a few records beyond 16 / 20 KB and payloads of fake chains.  printable: barcodes, UMIs and gene names of
    printable ASCII only, of one length each (the files that also go to the oracle, whose merge wants barcodes and UMIs of equal lengths)."""
    rng = np.random.default_rng(seed)
    out = []
    # (printable: N as the only escape -- the container's UMI re-keying takes no lowercase UMI, which the decoder legs do cover)
    high = "ACGTN" if printable else "ACGTNacgt\x80\xfe"
    pool = [_bases(rng, 16) for _ in range(40)]       # (printable: a few dozen cells with many reads each, so that the oracle keeps cells)
    for i in range(n):
        k = int(rng.integers(0, 100))
        # barcode / UMI: mostly packable, with every edge of pack_code
        cbn = int(rng.choice([12, 16, 31, 32, 1, 40])) if k < 30 and not printable else 16
        cb = (pool[int(rng.integers(0, len(pool)))] if printable else _bases(rng, cbn)) if k % 7 else _bases(rng, cbn, high)
        umi = _bases(rng, 10 if printable else int(rng.choice([8, 10, 31, 32]))) if k % 11 else _bases(rng, 10 if printable else 8, high)
        gene = GENES[int(rng.integers(0, len(GENES)))]
        qual = lambda m: bytes(int(x) for x in rng.choice([33, 34, 40, 74, 126, 127, 0x80, 0xFF, 35, 126], m, p=[.05, .05, .2, .3, .2, .05, .02, .03, .05, .05]))
        name = "r%d" % i
        flag = int(rng.choice([0, 0, 0, 0x10, 0x800, 0x4, 0x100, 0x200], p=[.5, .1, .1, .1, .08, .04, .04, .04]))
        ref = int(rng.integers(0, N_REFS)) if k % 29 else int(rng.choice([-1, N_REFS, N_REFS + 3]))
        tags = []
        for _ in range(int(rng.integers(0, 3))):      # noise in front: every type and subtype, skipped by its width
            tags.append(_noise(rng))
        if k % 13:
            tags.append(("CB", "Z", cb.encode("latin-1")))
        if k % 17 == 3:
            tags.insert(0, ("UB", "i", 7))            # numeric first: closes the name
        if k % 17:
            tags.append(("UB", "Z" if k % 5 or printable else "A", umi.encode("latin-1") if k % 5 or printable else umi[:1].encode("latin-1")))
        if k % 19 == 0:
            tags.append(("CB", "Z", b"TTTT"))         # second occurrence: not used
        if k % 3:
            tags.append(("CQ", "Z", qual(len(cb) if k % 4 else 0)))
        if k % 5 != 1 and not printable:       # (the reader legs: no UMI quality strings, whose lengths the container checks per molecule)
            tags.append(("UQ", "Z", qual(int(rng.choice([8, 8, 8, 10, 0])))))
        if k % 9:
            tags.append(("GX", "Z", gene if k % 23 else b""))
            if k % 37 == 2:
                tags.insert(0, ("GX", "S", 3))
        if k % 4:
            tags.append(("RE", "A" if k % 8 else "Z", [b"N", b"I", b"E", b"", b"X"][k % 5][: 1 if k % 8 else 8] or (b"" if k % 8 == 0 else b"E")))
        tags.append(_noise(rng))
        if k == 97:
            tags.append(b"xx" + b"Q" + bytes(5))      # an unknown type: the walk stops there
            tags.append(("GX", "Z", b"LATE"))
        if k == 98:
            tags.insert(len(tags) // 2, b"zzZ" + b"AB")    # a string that never ends: nothing behind it is seen
        if k == 96:
            tags.append(b"zzB" + b"i" + struct.pack("<I", 10_000_000))   # an array that claims more than the record holds
        if not printable and k == 95:
            name = "id!x!%s#%s#%s" % (cb, "AC", umi)
        elif k < 50:
            name = "id%d!%s#%s" % (i, cb, umi) if k % 10 else ("a!#%s" % umi if k % 20 else "b!%s#" % cb)
        seq = _bases(rng, int(rng.choice([0, 1, 7, 98])))
        cigar = [(int(rng.integers(1, 20)), op) for op in rng.choice(list("MIDNSHP=X"), int(rng.integers(0, 4)))] if k % 6 == 0 else None
        if big and k == 99 and i % 3 == 0:
            # beyond a segment / the wave's stage: a long array (sometimes a chain of fake records) behind the wanted tags
            body = _fake_chain(rng, 150) if i % 2 else bytes(int(rng.choice([17_000, 22_000, 70_000])))
            tags.append(("zb", "B", ("C", list(body))))
        out.append(bw.record(ref, i, name, flag=flag, seq=seq, cigar=cigar, tags=tags, qual=qual(len(seq)) if seq else b"",
                             next_ref=int(rng.integers(-1, N_REFS + 2))))
    return out


def _noise(rng):
    typ = str(rng.choice(list("cCsSiIfBZHA")))
    if typ == "B":
        sub = str(rng.choice(list("cCsSiIf")))
        vals = list(rng.integers(0, 100, int(rng.integers(0, 6))))
        return ("n%s" % sub, "B", (sub, [float(v) for v in vals] if sub == "f" else [int(v) for v in vals]))
    val = {"c": -5, "C": 250, "s": -3000, "S": 65000, "i": -70000, "I": 3_000_000_000, "f": 0.25, "Z": "CB", "H": "1F", "A": "q"}[typ]
    return ("x" + typ.lower(), typ, val)


# ---- configurations and dictionaries --------------------------------------------------------------------------------------------------
def configs():
    """(id, model Cfg): filled / name mode; min_phred off, 34, 126; read type off, intronic only, both; quality tags asked or not"""
    out = []
    for filled in (True, False):
        for mp in (0, 34, 126):
            for rt in ("off", "intronic", "both"):
                for q in (True, False):
                    if not filled and (mp == 34 or rt == "intronic"):
                        continue
                    tags = TAGS if q else (TAGS[0], TAGS[1], "", "", TAGS[4], TAGS[5])
                    out.append(("%s-q%d-%s-%s" % ("f" if filled else "n", mp, rt, "Q" if q else "noQ"),
                                bm.Cfg(tags=tags if rt != "off" else tags[:5] + ("",), filled_bam=filled, min_phred=mp, read_type=rt != "off",
                                       intronic=b"N" if rt != "off" else b"", intergenic=b"I" if rt == "both" else b"", n_refs=N_REFS)))
    return out


def c_cfg(cfg):
    c = Cfg()
    for k, t in enumerate(cfg.tags):
        c.tag[k] = bm.tag16(t)
    c.filled_bam, c.min_phred, c.has_read_type, c.n_refs = int(cfg.filled_bam), cfg.min_phred, int(cfg.read_type), cfg.n_refs
    c.intronic_len, c.intergenic_len = len(cfg.intronic), len(cfg.intergenic)
    for k, b in enumerate(cfg.intronic):
        c.intronic[k] = b
    for k, b in enumerate(cfg.intergenic):
        c.intergenic[k] = b
    return c


def dictionaries(kind, bits=64):
    """empty; half (every other gene, some chromosomes unknown); full with names; (hash bits < 64: names that collide)"""
    mask = (1 << bits) - 1
    if kind == "empty":
        return bm.Dicts({}, [-1] * N_REFS, None, mask), [], []
    ids = list(range(0, len(GENES), 2)) if kind == "half" else list(range(len(GENES)))
    genes, pairs = {}, []
    for g in ids:
        h = bm.fnv1a(GENES[g]) & mask
        genes.setdefault(h, 10 + g)
        pairs.append((h, 10 + g))
    names = None
    if kind == "named":
        names = [b""] * (10 + len(GENES))
        for g in ids:
            names[10 + g] = GENES[g]
    chr_of_ref = [3, -1, 0, 5, -1, 1] if kind == "half" else [4, 2, 0, 5, 3, 1]
    return bm.Dicts(genes, chr_of_ref, names, mask), pairs, names


# ---- the decoder through ctypes --------------------------------------------------------------------------------------------------------
def lib():
    from dropest_amd import capi
    L = capi.lib()
    L.dropest_bgzf_last_error.restype = C.c_char_p
    L.dropest_bam_decoder_window.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, P(Window)]
    L.dropest_bam_decoder_window_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, P(C.c_int)]
    L.dropest_bam_decoder_window_finish.argtypes = [C.c_void_p, C.c_int, P(Window)]
    L.dropest_bam_decoder_window_inflate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, P(C.c_int)]
    L.dropest_bam_decoder_window_chain.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
    L.dropest_bam_decoder_columns_to_host.argtypes = [C.c_void_p] * 5
    L.dropest_bam_decoder_fetch_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    L.dropest_bam_decoder_quality_rows.argtypes = [C.c_void_p, C.c_uint32, P(C.c_void_p)]
    L.dropest_bam_decoder_set_dictionaries.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    L.dropest_bam_decoder_set_gene_names.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.dropest_bam_decoder_reset.argtypes = [C.c_void_p, C.c_void_p]
    L.dropest_bam_decoder_destroy.argtypes = [C.c_void_p]
    L.dropest_bam_decoder_use_stream.argtypes = [C.c_void_p, C.c_void_p]
    return L


def make_decoder(L, cfg, dicts, pairs, names):
    dec = C.c_void_p()
    cc = c_cfg(cfg)
    assert L.dropest_bam_decoder_create(0, C.byref(cc), C.byref(dec)) == 0, L.dropest_bgzf_last_error()
    set_dicts(L, dec, dicts, pairs, names)
    return dec


def set_dicts(L, dec, dicts, pairs, names):
    if pairs or any(c >= 0 for c in dicts.chr_of_ref):
        h = np.array([p[0] for p in pairs] or [0], np.uint64); ids = np.array([p[1] for p in pairs] or [0], np.uint32)
        ch = np.array(dicts.chr_of_ref, np.int32)
        assert L.dropest_bam_decoder_set_dictionaries(dec, h.ctypes.data, ids.ctypes.data, len(pairs), ch.ctypes.data, len(ch)) == 0, L.dropest_bgzf_last_error()
    if names is not None:
        off = np.cumsum([0] + [len(n) for n in names]).astype(np.uint32)
        pool = np.frombuffer(b"".join(names) + b"\0", np.uint8)
        assert L.dropest_bam_decoder_set_gene_names(dec, off.ctypes.data, pool.ctypes.data, len(names)) == 0, L.dropest_bgzf_last_error()


class BamFile:
    """A written file: its compressed blocks from the one that holds the first record on, the inflated stream, the records and where they end."""
    def __init__(self, path, recs, block, compress=None):
        bw.write_bam(path, REFS, recs, block=block, compress=compress)
        self.blob = open(path, "rb").read()
        raw = gzip.decompress(self.blob)
        first, got = bm.records_of(raw)
        assert got == recs
        self.recs = recs
        self.blocks = []             # (compressed start, compressed end, inflated start, inflated end)
        at = cum = 0
        while at < len(self.blob):
            bsize = struct.unpack_from("<H", self.blob, at + 16)[0] + 1
            isize = struct.unpack_from("<I", self.blob, at + bsize - 4)[0]
            self.blocks.append((at, at + bsize, cum, cum + isize))
            at += bsize; cum += isize
        self.b0 = next(k for k, b in enumerate(self.blocks) if b[2] <= first < b[3])
        self.u0 = first - self.blocks[self.b0][2]
        self.ends = np.cumsum([len(r) for r in recs]) + first

    def windows(self, per):
        """whole blocks from the first record's block to the end, cut into windows of at least per[0], per[1], ... compressed bytes in turn
        (1: a single block); -> [(compressed bytes, inflated end)]"""
        out, k, j = [], self.b0, 0
        while k < len(self.blocks):
            want = per[j % len(per)]; j += 1
            last = k + 1
            while last < len(self.blocks) and self.blocks[last - 1][1] - self.blocks[k][0] < want:
                last += 1
            out.append((self.blob[self.blocks[k][0]:self.blocks[last - 1][1]], self.blocks[last - 1][3]))
            k = last
        return out


def run_file(L, dec, f, per, mode="window"):
    """Every window of file f through the decoder -> a list of per-window results.  mode: window | begin_finish | pipelined
    (inflate(k + 1) before chain(k), the order of BamController's device path)."""
    wins = f.windows(per)
    res = []
    comps = [np.frombuffer(w[0], np.uint8).copy() for w in wins]
    pending = None
    for k, comp in enumerate(comps):
        final = int(k == len(comps) - 1)
        skip = f.u0 if k == 0 else 0
        w = Window()
        if mode == "window":
            assert L.dropest_bam_decoder_window(dec, comp.ctypes.data, len(comp), skip, final, None, None, C.byref(w)) == 0, L.dropest_bgzf_last_error()
        elif mode == "begin_finish":
            slot = C.c_int(-1)
            assert L.dropest_bam_decoder_window_begin(dec, comp.ctypes.data, len(comp), skip, final, None, None, C.byref(slot)) == 0, L.dropest_bgzf_last_error()
            assert L.dropest_bam_decoder_window_finish(dec, slot.value, C.byref(w)) == 0, L.dropest_bgzf_last_error()
        else:
            slot = C.c_int(-1)
            if pending is None:
                assert L.dropest_bam_decoder_window_inflate(dec, comp.ctypes.data, len(comp), C.byref(slot)) == 0, L.dropest_bgzf_last_error()
                pending = slot.value
            cur = pending
            pending = None
            if k + 1 < len(comps):
                nxt = C.c_int(-1)
                assert L.dropest_bam_decoder_window_inflate(dec, comps[k + 1].ctypes.data, len(comps[k + 1]), C.byref(nxt)) == 0, L.dropest_bgzf_last_error()
                pending = nxt.value
            assert L.dropest_bam_decoder_window_chain(dec, cur, skip, final, None, None) == 0, L.dropest_bgzf_last_error()
            assert L.dropest_bam_decoder_window_finish(dec, cur, C.byref(w)) == 0, L.dropest_bgzf_last_error()
        res.append(collect(L, dec, w) + (wins[k][1],))
    return res


def collect(L, dec, w):
    n = int(w.n_accepted)
    cb, umi = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    gene, aux = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    if n:
        assert L.dropest_bam_decoder_columns_to_host(dec, cb.ctypes.data, umi.ctypes.data, gene.ctypes.data, aux.ctypes.data) == 0, L.dropest_bgzf_last_error()
    nn = int(w.n_need)
    need = [np.ctypeslib.as_array(a, (nn,)).tolist() if nn else [] for a in (w.need_rec, w.need_pos, w.need_size)]
    fetched = b""
    if nn:
        idx = np.array(need[0], np.uint32)
        buf = np.zeros(sum(need[2]) + 16, np.uint8); off = np.zeros(nn, np.uint64)
        assert L.dropest_bam_decoder_fetch_records(dec, idx.ctypes.data, nn, buf.ctypes.data, len(buf), off.ctypes.data) == 0, L.dropest_bgzf_last_error()
        fetched = buf[:sum(need[2])].tobytes()
    rows = None
    ql = int(w.quality_len_max)
    if n and w.any_gene and w.quality_len_min == ql and 0 < ql <= 255:
        p = C.c_void_p()
        assert L.dropest_bam_decoder_quality_rows(dec, ql, C.byref(p)) == 0, L.dropest_bgzf_last_error()
        rows = np.ctypeslib.as_array(C.cast(p, P(C.c_uint8)), (n, ql)).copy()
    info = dict(n_records=int(w.n_records), counts=list(w.counts), need=need, quality_seen=int(w.quality_seen), any_gene=int(w.any_gene),
                ql=(int(w.quality_len_min), int(w.quality_len_max)), refused=int(w.refused_blocks), repaired=int(w.guesses_repaired), tail=int(w.tail_bytes),
                blocks=int(w.n_blocks), bytes=int(w.window_bytes))
    return (info, (cb, umi, gene, aux), fetched, rows)


def check_against_model(f, res, cfg, dicts):
    """the decoder's windows == the model's, record by record"""
    rows = [bm.parse_record(r, cfg, dicts) for r in f.recs]
    at = 0
    all_cols, want_cols = [[], [], [], []], [[], [], [], []]
    for info, cols, fetched, qrows, inflated_end in res:
        k = int(np.searchsorted(f.ends, inflated_end, side="right"))       # the records that END in this window start in it (or were carried over)
        mine, recs = rows[at:k], f.recs[at:k]
        m = bm.window(mine)
        assert info["refused"] == 0
        assert info["n_records"] == len(mine)
        assert info["counts"] == m.counts, (info["counts"], m.counts)
        assert info["need"] == [m.need_rec, m.need_pos, m.need_size]
        assert fetched == b"".join(recs[i] for i in m.need_rec)
        assert (info["quality_seen"], info["any_gene"]) == (m.quality_seen, m.any_gene)
        assert info["ql"] == (m.quality_len_min, m.quality_len_max)
        ok = [r for r in mine if r.status == bm.OK]
        if qrows is not None:
            ql = m.quality_len_max
            assert [qrows[j].tobytes() for j in range(len(ok))] == [(r.umi_quality or b"\0" * ql) if r.need & 2 else b"\0" * ql for r in ok]
        for c in range(4):
            all_cols[c].extend(int(x) for x in cols[c])
        for r in ok:
            want_cols[0].append(r.cb); want_cols[1].append(r.umi); want_cols[2].append(r.gene); want_cols[3].append(r.aux)
        at = k
    assert at == len(rows)
    for c, what in enumerate(("cb", "umi", "gene", "aux")):
        if all_cols[c] != want_cols[c]:
            bad = next(j for j in range(len(want_cols[c])) if j >= len(all_cols[c]) or all_cols[c][j] != want_cols[c][j])
            raise AssertionError("column %s differs first at accepted row %d: device %r, model %r" % (what, bad, all_cols[c][bad:bad + 3], want_cols[c][bad:bad + 3]))
    return rows


SEEDS = [(101, 0xFF00), (202, 12_345), (303, 4093), (404, 40_000), (505, 0xFF00), (606, 777)]
CASES = configs()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("fuzz")
    return {seed: BamFile(str(d / ("f%d.bam" % seed)), fuzz_records(seed, 12_000), block) for seed, block in SEEDS}


@pytest.mark.parametrize("seed_i", range(len(SEEDS)))
def test_fuzzed_windows_against_the_model(files, seed_i, monkeypatch):
    """each seed: a share of the configurations and dictionaries; windows of 1, 3, 17, 5 blocks and the whole file"""
    seed, _ = SEEDS[seed_i]
    f = files[seed]
    L = lib()
    kinds = ["empty", "half", "named", "collide"]
    for j, (cid, cfg) in enumerate(CASES):
        if j % len(SEEDS) != seed_i:
            continue
        kind = kinds[(j // len(SEEDS) + seed_i) % len(kinds)]
        bits = 6 if kind == "collide" else 64
        if kind == "collide":
            monkeypatch.setenv("DROPEST_BAM_TEST_GENE_HASH_BITS", "6")      # (read when a decoder is created)
        else:
            monkeypatch.delenv("DROPEST_BAM_TEST_GENE_HASH_BITS", raising=False)
        dicts, pairs, names = dictionaries("named" if kind == "collide" else kind, bits)
        dec = make_decoder(L, cfg, dicts, pairs, names)
        try:
            per = [[1, 60_000, 250_000], [90_000], [1 << 40]][j % 3]
            res = run_file(L, dec, f, per, "window")
            rows = check_against_model(f, res, cfg, dicts)
            assert sum(r.status == bm.OK for r in rows) > 1000 or not cfg.filled_bam or cfg.min_phred > 33, cid
            # the two split orders give the same windows
            for mode in ("begin_finish", "pipelined"):
                assert L.dropest_bam_decoder_reset(dec, C.byref(c_cfg(cfg))) == 0
                set_dicts(L, dec, dicts, pairs, names)
                res2 = run_file(L, dec, f, per, mode)
                assert [r[0] for r in res2] == [r[0] for r in res], (cid, mode)
                assert all((a[1][c] == b[1][c]).all() for a, b in zip(res, res2) for c in range(4)), (cid, mode)
        finally:
            L.dropest_bam_decoder_destroy(dec)


def test_layouts_long_records_and_fake_chains(tmp_path):
    """records > 16 KB and > 20 KB among small ones in one wave; payloads of fake record chains (the guesses go wrong on their own: repaired
    without DROPEST_BAM_TEST_SPOIL_GUESSES); a record > 1 MB cut by window boundaries in the pipelined order (its tail outgrows the room kept
    for it: the data move behind it)"""
    assert "DROPEST_BAM_TEST_SPOIL_GUESSES" not in os.environ
    rng = np.random.default_rng(9)
    recs = fuzz_records(77, 3000, big=False)
    long_ = []
    for j, at in enumerate(range(100, 3000, 150)):
        body = bytes(1_500_000) if j == 5 else [bytes(17_000), bytes(21_000), _fake_chain(rng, 600), bytes(30_000)][j % 4]
        long_.append(at)
        recs[at] = bw.record(1, at, "long%d" % at, tags=[("CB", "Z", "ACGTACGTACGT"), ("UB", "Z", "ACGTAC"), ("GX", "Z", "G1"), ("zb", "B", ("C", list(body)))])
    f = BamFile(str(tmp_path / "l.bam"), recs, 0xFF00)
    sizes = [len(r) for r in recs]
    assert max(sizes) > (1 << 20) and sum(s > 20_480 for s in sizes) >= 10
    assert any(sum(sizes[w:w + 64]) > 20_480 and min(sizes[w:w + 64]) < 1000 for w in range(0, len(sizes), 64))     # a wave that falls back to memory
    L = lib()
    cfg = dict(CASES)["f-q0-both-Q"]
    dicts, pairs, names = dictionaries("named")
    for mode, per in (("window", [1, 50_000]), ("pipelined", [1]), ("begin_finish", [1 << 40])):
        dec = make_decoder(L, cfg, dicts, pairs, names)
        try:
            res = run_file(L, dec, f, per, mode)
            check_against_model(f, res, cfg, dicts)
            assert sum(r[0]["repaired"] for r in res) > 0, mode          # the fake chains fooled a guess and the host's check put it right
            if mode == "pipelined":
                tails = [r[0]["tail"] for r in res]
                # window k + 1 was inflated before window k said how long its tail is: a tail beyond 1 MB and beyond the one before it moved the data
                assert any(tails[k] > (1 << 20) and tails[k] > (tails[k - 1] if k else 0) for k in range(len(tails) - 1)), tails
        finally:
            L.dropest_bam_decoder_destroy(dec)


class BamFileByBlocks(BamFile):
    def windows(self, per):
        """windows of per[0], per[1], ... BLOCKS in turn (the last entry again and again)"""
        out, k = [], self.b0
        for j in range(len(self.blocks)):
            if k >= len(self.blocks):
                break
            last = min(k + per[min(j, len(per) - 1)], len(self.blocks))
            out.append((self.blob[self.blocks[k][0]:self.blocks[last - 1][1]], self.blocks[last - 1][3]))
            k = last
        return out


def _window_shapes(f, per, rows):
    """per window of f.windows(per), from the file and the model alone: (blocks, bytes with the record carried over, 16 KB segments of those
    bytes, records, records the host must see)"""
    out, k, at, start = [], f.b0, 0, f.blocks[f.b0][2]
    for comp, end in f.windows(per):
        n_blocks = 0
        while k < len(f.blocks) and f.blocks[k][3] <= end:
            n_blocks += 1; k += 1
        carried = start - (int(f.ends[at - 1]) if at else start)          # the record the window before cut off
        upto = int(np.searchsorted(f.ends, end, side="right"))
        data = carried + end - start
        out.append((n_blocks, data, -(-data // 16384), upto - at, len(bm.window(rows[at:upto]).need_rec)))
        at, start = upto, end
    return out


def test_windows_at_the_copy_launches_edges(tmp_path):
    """The block table goes to the device, the chain's three arrays and the need lists come back, by kernels of 256 lanes a workgroup over n
    blocks / segments / listed records: windows with n = 1, 256 and 257 of each, with no listed record, and one with no record at all (nothing
    but the middle of a long record, which the window before and this one carry on).  File A: blocks of 512 bytes, windows of 1, 256 and 257
    blocks, in which 1, 256 and 257 records name a gene the dictionary does not have ("half": G1 is not in it, G0 is); a record of 3 000 bytes
    behind them.  File B: blocks of 16 KB, windows of 256 blocks: 256 segments in the first, 257 with the record carried into the second."""
    L = lib()
    cfg = dict(CASES)["f-q0-both-Q"]
    dicts, pairs, names = dictionaries("half")
    rec = lambda i, gene, seq="ACGT" * 10, extra=(): bw.record(0, i, "r%06d" % i, seq=seq, tags=[("CB", "Z", "ACGTACGTACGT"), ("UB", "Z", "ACGTAC"), ("GX", "Z", gene)] + list(extra))
    # A: the layout first (every gene known), then the same bytes with the genes of the chosen records changed -- names of one length
    n_a, long_at = 2600, 2300
    genes = [b"G0"] * n_a
    make_a = lambda path: BamFileByBlocks(path, [rec(i, genes[i], extra=[("zb", "B", ("C", [0] * 3000))] if i == long_at else ()) for i in range(n_a)], 512)
    f = make_a(str(tmp_path / "layout.bam"))
    s_long, e_long = int(f.ends[long_at - 1]), int(f.ends[long_at])
    inside = next(k for k, b in enumerate(f.blocks) if b[2] > s_long and b[3] < e_long)      # a block that holds nothing but bytes of the long record
    per_a = [1, 256, 257, inside - (f.b0 + 514), 1, 1 << 30]
    assert per_a[3] > 0
    plain = [bm.parse_record(r, cfg, dicts) for r in f.recs]
    shapes = _window_shapes(f, per_a, plain)
    assert [s[0] for s in shapes[:3]] == [1, 256, 257] and shapes[4][3] == 0 and all(s[4] == 0 for s in shapes)
    at = 0
    for (n_blocks, data, segs, n_recs, _), want in zip(shapes, (1, 256, 257)):
        assert n_recs >= want
        for i in range(at, at + want):
            genes[i] = b"G1"
        at += n_recs
    f = make_a(str(tmp_path / "a.bam"))
    # B: records of ~3 KB in blocks of 16 KB
    fb = BamFileByBlocks(str(tmp_path / "b.bam"), [rec(i, b"G0" if i % 300 else b"G1", seq="ACGT" * 500) for i in range(2800)], 16384)
    per_b = [256, 256, 1 << 30]
    seen = {"blocks": set(), "segments": set(), "need": set(), "records": set()}
    for g, per in ((f, per_a), (fb, per_b)):
        dec = make_decoder(L, cfg, dicts, pairs, names)
        try:
            first = None
            for mode in ("window", "begin_finish", "pipelined"):
                if first is not None:
                    assert L.dropest_bam_decoder_reset(dec, C.byref(c_cfg(cfg))) == 0
                    set_dicts(L, dec, dicts, pairs, names)
                res = run_file(L, dec, g, per, mode)
                rows = check_against_model(g, res, cfg, dicts)
                shapes = _window_shapes(g, per, rows)
                # the windows the device saw are the ones counted here, and what it listed is what the model lists
                assert [(r[0]["blocks"], r[0]["bytes"], r[0]["n_records"], len(r[0]["need"][0])) for r in res] == [(s[0], s[1], s[3], s[4]) for s in shapes], mode
                if first is None:
                    first = res
                    for s in shapes:
                        seen["blocks"].add(s[0]); seen["segments"].add(s[2]); seen["records"].add(s[3]); seen["need"].add(s[4])
                else:
                    assert [r[0] for r in res] == [r[0] for r in first], mode
                    assert all((a[1][c] == b[1][c]).all() for a, b in zip(first, res) for c in range(4)), mode
        finally:
            L.dropest_bam_decoder_destroy(dec)
    for what in ("blocks", "segments", "need"):
        assert {1, 256, 257} <= seen[what], (what, sorted(seen[what]))
    assert 0 in seen["need"] and 0 in seen["records"]


CHILD = r"""
import sys, os, ctypes as C
sys.path.insert(0, %(here)r); sys.path.insert(0, %(root)r)
import test_gpu_bam_decoder_model as t, bam_model as bm
f = t.BamFile(%(path)r, t.fuzz_records(%(seed)d, 6000), 4093)
L = t.lib()
for cid, cfg in t.CASES[::5]:
    dicts, pairs, names = t.dictionaries("half")
    dec = t.make_decoder(L, cfg, dicts, pairs, names)
    for mode, per in (("window", [20_000, 1]), ("pipelined", [1, 5_000])):
        assert L.dropest_bam_decoder_reset(dec, C.byref(t.c_cfg(cfg))) == 0
        t.set_dicts(L, dec, dicts, pairs, names)
        t.check_against_model(f, t.run_file(L, dec, f, per, mode), cfg, dicts)
    L.dropest_bam_decoder_destroy(dec)
print("child ok")
"""


@pytest.mark.parametrize("env", [{"DROPEST_INFLATE_PAR": "0"}, {"DROPEST_BAM_TEST_TAIL_RESERVE": "0"}])
def test_switches_read_once_in_a_child(tmp_path, env):
    """the serial inflate kernel, and no room kept in front of a window (every carried-over record moves the data): in a fresh process each"""
    code = CHILD % dict(here=HERE, root=os.path.dirname(HERE), path=str(tmp_path / "c.bam"), seed=31)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240, env=dict(os.environ, **env))
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---- part 3: the whole reader ---------------------------------------------------------------------------------------------------------
def _reader_run(tmp_path, bams, env, threads=3):
    import test_gpu_bam as tb
    return tb._run(tmp_path, "filled", bams, 3, 5, threads=threads, env=env)


@pytest.mark.parametrize("seed", [11, 12])
def test_fuzzed_files_through_the_reader(tmp_path, seed):
    """host bulk, host record by record and the device path (windows of 1 MB) give the same cells, counts and stats, and match the oracle fed
    with the model's accepted reads"""
    import test_gpu_bam as tb
    recs = fuzz_records(seed, 12_000, big=True, printable=True)
    path = str(tmp_path / "p.bam")
    bw.write_bam(path, REFS, recs, block=[0xFF00, 9_999][seed % 2])
    cfg = bm.Cfg(tags=TAGS, filled_bam=True, min_phred=0, read_type=True, intronic=b"N", intergenic=b"I", n_refs=N_REFS)
    rows = [bm.parse_record(r, cfg, bm.Dicts({}, [-1] * N_REFS)) for r in recs]
    kept = [(r.strings[0].decode(), r.strings[1].decode(), r.strings[2].decode() or None, REFS[r.strings[3]][0], r.strings[4]) for r in rows if r.status == bm.OK]
    want, cols = tb._oracle(kept, 3, 5)
    got, cells, stats, _ = _reader_run(tmp_path / "bulk", [path], {})
    assert cells == cols and got == want and len(want) > 50
    assert stats["saved"] == len(kept)
    assert stats["cant_parse"] == sum(r.status in (bm.CANT_PARSE, bm.CANT_PARSE_NO_COUNT) for r in rows)
    assert stats["total_reads"] == sum(r.status in (bm.OK, bm.CANT_PARSE, bm.LOW_QUALITY) for r in rows)
    for env in ({"DROPEST_BAM_RECORD_BY_RECORD": "1"}, {"DROPEST_BAM_DEVICE": "1", "DROPEST_BAM_DEVICE_WINDOW_MB": "1"}):
        got2, cells2, stats2, _ = _reader_run(tmp_path / ("e%d" % len(env)), [path], env)
        assert cells2 == cells and got2 == got, env
        assert {k: stats2[k] for k in ("total_reads", "cant_parse", "low_quality", "saved")} == {k: stats[k] for k in ("total_reads", "cant_parse", "low_quality", "saved")}, env


# ---- the three known divergences -------------------------------------------------------------------------------------------------------
def test_record_beyond_2_26_bytes(tmp_path):
    """a record with a B array of ~17 M int32 (68 MB, ~100 KB compressed): the host reader takes it; so must the device path, and the
    decoder must report it as a record"""
    import test_gpu_bam as tb
    recs = fuzz_records(5, 400, big=False, printable=True)
    n = 17 << 20
    big = bw.record(2, 77, "huge", tags=[("CB", "Z", "ACGTACGTACGTACGT"), ("UB", "Z", "ACGTACGT"), ("GX", "Z", "G3"), b"zzBi" + struct.pack("<I", n) + bytes(4 * n)])
    assert len(big) > (1 << 26)
    recs.insert(200, big)
    path = str(tmp_path / "huge.bam")
    bw.write_bam(path, REFS, recs, block=0xFF00)
    got, cells, stats, _ = _reader_run(tmp_path / "host", [path], {})
    got2, cells2, stats2, _ = _reader_run(tmp_path / "dev", [path], {"DROPEST_BAM_DEVICE": "1", "DROPEST_BAM_DEVICE_WINDOW_MB": "1"})
    assert cells2 == cells and got2 == got
    assert {k: stats2[k] for k in ("total_reads", "cant_parse", "low_quality", "saved")} == {k: stats[k] for k in ("total_reads", "cant_parse", "low_quality", "saved")}
    # the decoder itself: the record is one of the window's, accepted, its bytes fetched whole
    f = BamFile(str(tmp_path / "huge2.bam"), recs, 0xFF00)
    L = lib()
    cfg = bm.Cfg(tags=TAGS, filled_bam=True, read_type=True, intronic=b"N", intergenic=b"I", n_refs=N_REFS)
    dec = make_decoder(L, cfg, *dictionaries("empty"))
    try:
        res = run_file(L, dec, f, [1 << 40], "window")
        rows = check_against_model(f, res, cfg, dictionaries("empty")[0])
        assert rows[200].status == bm.OK and len(res) == 1 and res[0][0]["n_records"] == len(recs)
    finally:
        L.dropest_bam_decoder_destroy(dec)


def test_umi_quality_longer_than_65535(tmp_path):
    """quality_len_min / _max are the true lengths of the UMI quality strings (include/dropest_bgzf.h), not clamped to 16 bits"""
    recs = [bw.record(0, i, "q%d" % i, tags=[("CB", "Z", "ACGTACGT"), ("UB", "Z", "ACGT"), ("UQ", "Z", "I" * n), ("GX", "Z", "G1")])
            for i, n in enumerate([70_000, 66_000, 100_000, 65_535])]
    f = BamFile(str(tmp_path / "q.bam"), recs, 0xFF00)
    L = lib()
    cfg = bm.Cfg(tags=TAGS, filled_bam=True, min_phred=34, n_refs=N_REFS)
    dicts = dictionaries("named")
    dec = make_decoder(L, cfg, *dicts)
    try:
        res = run_file(L, dec, f, [1 << 40], "window")
        assert res[0][0]["ql"] == (65_535, 100_000)
        check_against_model(f, res, cfg, dicts[0])
    finally:
        L.dropest_bam_decoder_destroy(dec)
