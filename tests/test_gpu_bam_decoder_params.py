"""The device BAM decoder with its two sources beside a record's own tags and name, through the C-ABI (include/dropest_bgzf.h):
dropest_bam_decoder_set_read_params (-r: barcode, UMI and UMI quality from the read-parameter table, every row serving the first record of the
stream that asks) and dropest_bam_decoder_set_gene_of_reference (-P: the gene is the reference's name).  Counters, served rows, dense columns,
need list and quality rows of every record against the plain model (read_params_model.py)."""
import ctypes as C

import numpy as np
import pytest

import bam_writer as bw
import read_params_model as m
import test_gpu_bam_decoder_model as dm
from test_gpu_read_params_table import Table, lib as table_lib

pytestmark = pytest.mark.gpu
REFS = dm.REFS
GENES = ["G%d" % i for i in range(30)]
GENE_ID = {g: 7 + k for k, g in enumerate(GENES)}
CHR_OF_REF = [4, 2, 0, 5, 3, 1]
NO_GENE = 0xFFFFFFFF


def lib():
    L = dm.lib()
    table_lib()
    L.dropest_bam_decoder_set_read_params.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.dropest_bam_decoder_set_gene_of_reference.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.dropest_bam_decoder_param_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.dropest_bam_decoder_set_annotation.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    return L


def decoder(L, min_phred=0):
    """name mode (no -f), gene tag GX, read type RE (N intronic, I intergenic); the dictionaries hold every gene and chromosome"""
    cfg = dm.bm.Cfg(tags=dm.TAGS, filled_bam=False, min_phred=min_phred, read_type=True, intronic=b"N", intergenic=b"I", n_refs=len(REFS))
    cc = dm.c_cfg(cfg)
    dec = C.c_void_p()
    assert L.dropest_bam_decoder_create(0, C.byref(cc), C.byref(dec)) == 0, L.dropest_bgzf_last_error()
    give_dictionaries(L, dec)
    return dec, cc


def give_dictionaries(L, dec):
    h = np.array([dm.bm.fnv1a(g.encode()) for g in GENES], np.uint64)
    ids = np.array([GENE_ID[g] for g in GENES], np.uint32)
    ch = np.array(CHR_OF_REF, np.int32)
    assert L.dropest_bam_decoder_set_dictionaries(dec, h.ctypes.data, ids.ctypes.data, len(GENES), ch.ctypes.data, len(ch)) == 0, L.dropest_bgzf_last_error()


def param_rows(L, dec, n):
    out = np.zeros(max(n, 1), np.uint32)
    assert L.dropest_bam_decoder_param_rows(dec, None, n, out.ctypes.data) == 0, L.dropest_bgzf_last_error()
    return out[:n].tolist()


def make_records(n, seed, dups=(), special=True):
    """n records "q<i>" on random references, two thirds with a gene; dups: (i, j) -> record j carries record i's name.
    -> [(bytes, name, status before the parameters, gene or None, mark, ref)]"""
    rng = np.random.default_rng(seed)
    names = ["q%d" % i for i in range(n)]
    for i, j in dups:
        names[j] = names[i]
    out = []
    for i in range(n):
        g = None if i % 3 == 0 else GENES[int(rng.integers(0, len(GENES)))]
        rt = [None, "N", "I", "E"][i % 4] if g else None
        tags = ([("GX", "Z", g)] if g else []) + ([("RE", "A", rt)] if rt else []) + [("NH", "i", 1)]
        mark = 1 if g is None else (4 if rt == "N" else 1 if rt == "I" else 2)
        flag, ref, status = 0, int(rng.integers(0, len(REFS))), m.OK
        if special and i % 53 == 5:
            flag, status = 4, m.SKIP
        elif special and i % 53 == 6:
            flag, status = 0x100, m.SKIP
        elif special and i % 53 == 7:
            ref, status = -1, m.CANT_PARSE_NO_COUNT
        name = ("@" if i % 5 == 0 else "") + names[i]
        out.append((bw.record(ref, i, name, flag=flag, tags=tags), name.encode(), status, g, mark, ref))
    return out


def make_rows(recs, seed):
    """The parameter text for the records' names: some names without a row, some rows of low quality (under min_phred 53), barcodes / UMIs with N
    or 32 bases, repeated rows; in a shuffled order, '@' in front of some."""
    rng = np.random.default_rng(seed)
    lines, seen = [], set()
    for k, r in enumerate(recs):
        name = r[1].lstrip(b"@")
        if name in seen:
            continue
        seen.add(name)
        if k % 17 == 3:
            continue                                                  # no row
        cb = bytes(rng.choice(list(b"ACGT"), 12).tolist()); umi = bytes(rng.choice(list(b"ACGT"), 8).tolist())
        if k % 29 == 1:
            cb = cb[:4] + b"N" + cb[5:]
        if k % 31 == 2:
            umi = b"N" + umi[1:]
        if k % 101 == 9:
            cb = cb + cb + cb[:8]                                     # 32 bases
        q = bytes(rng.integers(53, 74, 8, dtype=np.uint8).tolist())
        cq = b"I" * len(cb)
        if k % 13 == 4:
            cq = b"+" + cq[1:]                                        # low quality
        lines.append((b"@" if k % 2 else b"") + name + b" " + cb + b" " + umi + b" " + cq + b" " + q + b"\n")
        if k % 37 == 8:
            lines.append(name + b" AAAA CCCC IIII IIII\n")            # a repeated name: never served
    order = rng.permutation(len(lines))
    return b"".join(lines[k] for k in order)


def expected(recs, rows, server, chr_missing=()):
    """per record: (status, served row); chr_missing: the references a -g annotation has no chromosome for"""
    out = []
    for raw, name, status0, g, mark, ref in recs:
        if status0 == m.OK and ref in chr_missing:
            status0 = m.CANT_PARSE
        out.append(server.serve(status0, name))
    return out


def check_window(L, dec, w, recs, exp, rows, gene_of=None, annotated=False):
    """one finished window over `recs` against exp = [(status, row)]; gene_of(rec) -> (gene id or None, mark) replaces the gene tag's answer"""
    info, (cb, umi, gene, aux), _, qrows = dm.collect(L, dec, w)
    assert info["n_records"] == len(recs)
    assert info["counts"] == [sum(1 for s, _ in exp if s == k) for k in range(5)]
    assert param_rows(L, dec, len(recs)) == [r for _, r in exp]
    ok = [k for k, (s, _) in enumerate(exp) if s == m.OK]
    assert len(cb) == len(ok)
    need_pos, q_lens = [], []
    for at, k in enumerate(ok):
        row = rows.rows[exp[k][1]]
        _, _, _, g, mark, ref = recs[k]
        gid = GENE_ID[g] if g else None
        if gene_of:
            gid, mark = gene_of(recs[k])
        if annotated:                                                  # (the annotation's genes are not compared here: barcode and UMI alone)
            assert cb[at] == m.pack(row["cb"]), k
            continue
        has_gene = gid is not None
        want_umi = m.pack(row["umi"]) if has_gene else 1
        touches = not has_gene or (mark & 6)
        unknown = gid == -1
        assert (cb[at], umi[at]) == (m.pack(row["cb"]), want_umi), k
        if not unknown:
            assert gene[at] == (gid if has_gene else NO_GENE), k
        assert aux[at] == (mark << 16) | (CHR_OF_REF[ref] if touches else 0), k
        if not m.pack(row["cb"]) or not want_umi or unknown:
            need_pos.append(at)
        if has_gene:
            q_lens.append(len(row["quality"]))
        if qrows is not None:
            assert qrows[at].tobytes() == (row["quality"] if has_gene else b"\0" * qrows.shape[1]), k
    if not annotated:
        assert info["need"][1] == need_pos and info["need"][0] == [ok[p] for p in need_pos]
        assert info["ql"] == ((min(q_lens), max(q_lens)) if q_lens else (0, 0))
        assert qrows is not None or not q_lens or min(q_lens) != max(q_lens)


def run_windows(L, dec, f, per, recs, exp, rows, **kw):
    """the file's windows in turn, each against its stretch of the records"""
    at, in_windows = 0, []
    wins = f.windows(per)
    for k, (comp, _) in enumerate(wins):
        buf = np.frombuffer(comp, np.uint8).copy()
        w = dm.Window()
        assert L.dropest_bam_decoder_window(dec, buf.ctypes.data, len(buf), f.u0 if k == 0 else 0, int(k == len(wins) - 1), None, None, C.byref(w)) == 0, L.dropest_bgzf_last_error()
        n = int(w.n_records)
        check_window(L, dec, w, recs[at:at + n], exp[at:at + n], rows, **kw)
        at += n; in_windows.append(n)
    assert at == len(recs)
    return in_windows


DUPS = [(10, 11), (63, 64), (127, 128), (4095, 4096), (21, 4200), (200, 5000), (4101, 5100)]      # (lanes, waves, parse workgroups, fin tiles, windows)


@pytest.fixture(scope="module")
def stream(tmp_path_factory):
    """5 300 records and their parameter text"""
    recs = make_records(5300, 1, DUPS)
    text = make_rows(recs, 2)
    f = dm.BamFile(str(tmp_path_factory.mktemp("params") / "p.bam"), [r[0] for r in recs], block=20_000)
    return recs, text, f


@pytest.mark.parametrize("cut", [None, 0.85], ids=["one-window", "two-windows"])
def test_records_are_served_in_file_order(stream, cut):
    recs, text, f = stream
    per = (1 << 30,) if cut is None else (int(len(f.blob) * cut), 1 << 30)
    L = lib()
    rows = m.Rows([text], 53)
    exp = expected(recs, rows, m.Server(rows))
    # the construction holds what it is meant to: both records of a pair ask for one row, and the first gets it
    served_pairs = 0
    for i, j in DUPS:
        if exp[i][0] in (m.OK, m.LOW_QUALITY) and recs[j][2] == m.OK:
            assert exp[j] == (m.CANT_PARSE, m.NONE)
            served_pairs += 1
    assert served_pairs == len(DUPS)
    hist = [sum(1 for s, _ in exp if s == k) for k in range(5)]
    assert hist[m.CANT_PARSE] > 250 and hist[m.LOW_QUALITY] > 250 and hist[m.SKIP] > 150 and hist[m.CANT_PARSE_NO_COUNT] > 80
    t = Table(L, [text], 53)
    dec, cc = decoder(L, 53)
    assert L.dropest_bam_decoder_set_read_params(dec, t.h, 1000) == 0, L.dropest_bgzf_last_error()
    in_windows = run_windows(L, dec, f, per, recs, exp, rows)
    assert len(in_windows) == len(per) and (cut is None or 4200 < in_windows[0] <= 5000)      # (three pairs lie across the cut)
    # the claims: a served row carries the ordinal of the record that took it (first_ordinal 1000 + its place in the stream)
    claims = np.zeros(len(rows.rows), np.uint64)
    assert L.dropest_read_params_claims_to_host(t.h, 0, len(claims), claims.ctypes.data) == 0
    want = np.full(len(claims), 0xFFFFFFFFFFFFFFFF, np.uint64)
    for k, (_, r) in enumerate(exp):
        if r != m.NONE:
            want[r] = 1000 + k
    assert (claims == want).all()
    # the same file again: every row is taken -- nothing is served; after _reset_claims everything is, as the first time (ordinals carried on)
    assert L.dropest_bam_decoder_reset(dec, C.byref(cc)) == 0
    give_dictionaries(L, dec)
    assert L.dropest_bam_decoder_set_read_params(dec, t.h, 1000 + len(recs)) == 0
    taken = {r for _, r in exp if r != m.NONE}
    server2 = m.Server(rows)
    server2.left = {name: r for name, r in server2.left.items() if r not in taken}
    exp2 = expected(recs, rows, server2)
    assert sum(1 for s, _ in exp2 if s == m.OK) < 20
    run_windows(L, dec, f, per, recs, exp2, rows)
    assert L.dropest_read_params_reset_claims(t.h) == 0
    assert L.dropest_bam_decoder_reset(dec, C.byref(cc)) == 0
    give_dictionaries(L, dec)
    assert L.dropest_bam_decoder_set_read_params(dec, t.h, 7) == 0
    run_windows(L, dec, f, per, recs, exp, rows)
    L.dropest_bam_decoder_destroy(dec)
    t.close()


def test_dups_second_record_served_when_the_first_is_skipped(tmp_path):
    """an unmapped, a secondary and a ref -1 record with a listed name consume nothing; a low-quality row is consumed"""
    L = lib()
    recs = [(bw.record(0, 1, "a", flag=4), b"a", m.SKIP, None, 1, 0), (bw.record(0, 2, "b", flag=0x100), b"b", m.SKIP, None, 1, 0),
            (bw.record(-1, 3, "c"), b"c", m.CANT_PARSE_NO_COUNT, None, 1, -1), (bw.record(1, 4, "@a"), b"@a", m.OK, None, 1, 1),
            (bw.record(2, 5, "b"), b"b", m.OK, None, 1, 2), (bw.record(3, 6, "c"), b"c", m.OK, None, 1, 3), (bw.record(3, 7, "c"), b"c", m.OK, None, 1, 3),
            (bw.record(4, 8, "low"), b"low", m.OK, None, 1, 4), (bw.record(4, 9, "low"), b"low", m.OK, None, 1, 4), (bw.record(5, 10, "none"), b"none", m.OK, None, 1, 5)]
    text = b"a ACGT TT II II\n@b CCGT TT II II\nc GGGT TT II II\nlow ACGT TT +I II\n"
    rows = m.Rows([text], 53)
    exp = expected(recs, rows, m.Server(rows))
    assert exp == [(m.SKIP, m.NONE), (m.SKIP, m.NONE), (m.CANT_PARSE_NO_COUNT, m.NONE), (m.OK, 0), (m.OK, 1), (m.OK, 2), (m.CANT_PARSE, m.NONE),
                   (m.LOW_QUALITY, 3), (m.CANT_PARSE, m.NONE), (m.CANT_PARSE, m.NONE)]
    f = dm.BamFile(str(tmp_path / "s.bam"), [r[0] for r in recs], block=20_000)
    t = Table(L, [text], 53)
    dec, _ = decoder(L, 53)
    assert L.dropest_bam_decoder_set_read_params(dec, t.h, 0) == 0
    run_windows(L, dec, f, (1 << 30,), recs, exp, rows)
    # an empty table: nothing can be parsed
    t0 = Table(L, [b""], 53)
    assert L.dropest_bam_decoder_set_read_params(dec, t0.h, 0) == 0
    rows0 = m.Rows([b""], 53)
    run_windows(L, dec, f, (1 << 30,), recs, expected(recs, rows0, m.Server(rows0)), rows0)
    # no table any more: the names are read as "id!CB#UMI" again, which these are not
    assert L.dropest_bam_decoder_set_read_params(dec, None, 0) == 0
    buf = np.frombuffer(f.windows((1 << 30,))[0][0], np.uint8).copy()
    w = dm.Window()
    assert L.dropest_bam_decoder_window(dec, buf.ctypes.data, len(buf), f.u0, 1, None, None, C.byref(w)) == 0
    assert list(w.counts) == [0, 2, 1, 7, 0]
    out = np.zeros(4, np.uint32)
    assert L.dropest_bam_decoder_param_rows(dec, None, 1, out.ctypes.data) != 0 and b"no read-parameter table" in L.dropest_bgzf_last_error()
    L.dropest_bam_decoder_destroy(dec)
    t.close(); t0.close()


def test_annotated_record_on_a_missing_chromosome_takes_its_row(tmp_path):
    """-g: a record on a chromosome the annotation lacks cannot be parsed and still consumes its row; low quality wins over that verdict"""
    from test_gene_annotation import Product
    from test_gpu_annotation import DeviceAnnotation
    L = lib()
    gtf = tmp_path / "a.gtf"
    gtf.write_text('chr0\ts\texon\t1\t5000\t.\t+\t.\tgene_id "A"; transcript_id "T";\nchr1\ts\texon\t1\t5000\t.\t+\t.\tgene_id "B"; transcript_id "U";\n')
    ann = DeviceAnnotation(Product(str(gtf)))
    recs = make_records(600, 3, [(5, 300), (8, 301), (13, 302)], special=False)
    text = make_rows(recs, 4)
    rows = m.Rows([text], 53)
    missing = {r for r in range(len(REFS)) if REFS[r][0] not in ann.chr_index}
    assert missing == {2, 3, 4, 5}
    exp = expected(recs, rows, m.Server(rows), chr_missing=missing)
    took = [k for k, (s, r) in enumerate(exp) if s == m.CANT_PARSE and r != m.NONE]
    low = [k for k, (s, r) in enumerate(exp) if s == m.LOW_QUALITY and recs[k][5] in missing]
    assert len(took) > 100 and len(low) > 10
    f = dm.BamFile(str(tmp_path / "g.bam"), [r[0] for r in recs], block=20_000)
    t = Table(L, [text], 53)
    dec, _ = decoder(L, 53)
    ann_chr = np.array([ann.chr_index.get(name, -1) for name, _ in REFS], np.int32)
    assert L.dropest_bam_decoder_set_annotation(dec, ann.h, ann_chr.ctypes.data, len(REFS)) == 0, L.dropest_bgzf_last_error()
    assert L.dropest_bam_decoder_set_read_params(dec, t.h, 0) == 0
    run_windows(L, dec, f, (1 << 30,), recs, exp, rows, annotated=True)
    L.dropest_bam_decoder_destroy(dec)
    t.close(); ann.close()


def test_gene_of_reference(tmp_path):
    """-P: the gene is the reference's; -1 makes need records until the table is sent again, -2 is no gene and mark 0; the gene tag, the read type
    and an annotation are not looked at; with and without -r"""
    from test_gene_annotation import Product
    from test_gpu_annotation import DeviceAnnotation
    L = lib()
    recs = make_records(700, 5)
    text = make_rows(recs, 6)
    f = dm.BamFile(str(tmp_path / "p.bam"), [r[0] for r in recs], block=20_000)
    gtf = tmp_path / "a.gtf"
    gtf.write_text('chr0\ts\texon\t1\t5000\t.\t+\t.\tgene_id "A"; transcript_id "T";\n')
    ann = DeviceAnnotation(Product(str(gtf)))
    ann_chr = np.array([ann.chr_index.get(name, -1) for name, _ in REFS], np.int32)
    for with_params in (True, False):
        for with_annotation in (False, True):
            t = Table(L, [text], 53)
            rows = m.Rows([text], 53)
            exp = expected(recs, rows, m.Server(rows)) if with_params else None
            dec, cc = decoder(L, 53)
            if with_annotation:
                assert L.dropest_bam_decoder_set_annotation(dec, ann.h, ann_chr.ctypes.data, len(REFS)) == 0, L.dropest_bgzf_last_error()
            for table in ([40, -1, -2, 41, -1, 42], [40, 43, -2, 41, 44, 42]):
                g = np.array(table, np.int32)
                assert L.dropest_bam_decoder_set_gene_of_reference(dec, g.ctypes.data, len(g)) == 0, L.dropest_bgzf_last_error()
                if with_params:
                    assert L.dropest_read_params_reset_claims(t.h) == 0
                    assert L.dropest_bam_decoder_set_read_params(dec, t.h, 0) == 0

                    def gene_of(rec, table=table):
                        v = table[rec[5]]
                        return (None, 0) if v == -2 else (v, 2)
                    run_windows(L, dec, f, (1 << 30,), recs, exp, rows, gene_of=gene_of)
                else:             # (these names are no "id!CB#UMI": without the table nothing parses)
                    buf = np.frombuffer(f.windows((1 << 30,))[0][0], np.uint8).copy()
                    w = dm.Window()
                    assert L.dropest_bam_decoder_window(dec, buf.ctypes.data, len(buf), f.u0, 1, None, None, C.byref(w)) == 0
                    assert w.n_accepted == 0 and w.counts[m.CANT_PARSE] == sum(1 for r in recs if r[2] == m.OK)
            bad = np.array([0] * 5, np.int32)
            assert L.dropest_bam_decoder_set_gene_of_reference(dec, bad.ctypes.data, 5) != 0
            L.dropest_bam_decoder_destroy(dec)
            t.close()
    ann.close()


def test_gene_of_reference_with_names_in_the_read_name(tmp_path):
    """-P without -r: barcode and UMI from "id!CB#UMI", the gene from the reference, whatever the gene tag says"""
    L = lib()
    rng = np.random.default_rng(9)
    recs, want = [], []
    table = [40, -1, -2, 41, 42, 43]
    for i in range(500):
        cb = "".join(rng.choice(list("ACGT"), 10)); umi = "".join(rng.choice(list("ACGT"), 6))
        ref = int(rng.integers(0, 6))
        tags = [("GX", "Z", GENES[i % 30]), ("RE", "A", "N")] if i % 2 else []
        recs.append(bw.record(ref, i, "r%d!%s#%s" % (i, cb, umi), tags=tags))
        want.append((cb.encode(), umi.encode(), ref))
    f = dm.BamFile(str(tmp_path / "n.bam"), recs, block=20_000)
    dec, _ = decoder(L, 0)
    g = np.array(table, np.int32)
    assert L.dropest_bam_decoder_set_gene_of_reference(dec, g.ctypes.data, 6) == 0
    buf = np.frombuffer(f.windows((1 << 30,))[0][0], np.uint8).copy()
    w = dm.Window()
    assert L.dropest_bam_decoder_window(dec, buf.ctypes.data, len(buf), f.u0, 1, None, None, C.byref(w)) == 0
    info, (cb, umi, gene, aux), _, _ = dm.collect(L, dec, w)
    assert info["counts"] == [500, 0, 0, 0, 0]
    need = []
    for k, (c, u, ref) in enumerate(want):
        v = table[ref]
        assert cb[k] == m.pack(c) and umi[k] == (1 if v == -2 else m.pack(u)), k
        assert aux[k] == ((0 if v == -2 else 2) << 16) | CHR_OF_REF[ref], k
        if v >= 0 or v == -2:
            assert gene[k] == (NO_GENE if v == -2 else v), k
        else:
            need.append(k)
    assert info["need"][0] == need and len(need) > 50
    L.dropest_bam_decoder_destroy(dec)
