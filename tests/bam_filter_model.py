"""What one accepted BAM record becomes in the filtered BAM output (-F), restated in plain Python: TEST INFRASTRUCTURE for
dropest_bam_decoder_filter_window (include/dropest_bgzf.h) and the `.filtered.bam` file of BamController::write_filtered_bam_files.
Written from the rule of DESIGN.md §7 (FilteringBamProcessor::write_alignment, FilteringBamProcessor.cpp:61-96, which writes through
BamProcessorAbstract::save_alignment, BamProcessorAbstract.cpp:65-114) and from bam_model.py / bam_tag_model.py -- not from the kernels.

  filtered_record(rec, cfg, out_cfg, verdict, cb, umi) -> the output record's bytes (block_size field first), or None for a record that is
  not written: any status but OK, or a verdict that is not 0 ("written").
  cb / umi: the corrected cell barcode (the target cell's) and the corrected UMI, as bytes; an empty one writes no tag and drops none.

  filtered_stream(recs, cfg, out_cfg, decisions) -> the output of a stream of records, where decisions[k] = (verdict, cb, umi) belongs to the
  k-th ACCEPTED record; (bytes, records written, decisions used)."""
import struct
from dataclasses import dataclass

import bam_model as bm
import bam_tag_model as tm


@dataclass
class FilterOutCfg(tm.OutCfg):
    """dropest_bam_tag_cfg and dropest_bam_filter_cfg in Python terms: -b's output tags and the two corrected ones ("" = never written)."""
    cell_barcode: str = "CB"
    umi: str = "UB"


def code_string(code, side):
    """A packed code of include/dropest_amd.h as bytes: (1 << 2 * len) | bases, first base most significant; or ESCAPE | k for side[k]."""
    if code >> 63:
        return bytes(side[code & ((1 << 63) - 1)])
    n = (code.bit_length() - 1) // 2 if code else 0
    return bytes(b"ACGT"[(code >> (2 * (n - 1 - j))) & 3] for j in range(n))


def pack_code(s):
    """bytes of A, C, G, T (at most 31) -> the plain code"""
    code = 1
    for c in s:
        code = (code << 2) | b"ACGT".index(c)
    return code


def filtered_record(rec, cfg, out_cfg, verdict, cb, umi, gene_name=None, mark=None):
    row = bm.parse_record(rec, cfg, bm.Dicts(chr_of_ref=[0] * max(cfg.n_refs, 1)))
    if row.status != bm.OK or verdict != 0:
        return None
    raw_cb, raw_umi, g, _ref, m = row.strings
    if gene_name is not None:
        g = gene_name
    if mark is not None:
        m = mark
    block_size, l_read_name, n_cigar, l_seq = struct.unpack_from("<I", rec, 0)[0], rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<I", rec, 20)[0]
    aux = 32 + l_read_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq
    tags = bytes(rec[4 + aux:4 + block_size])
    cq = uq = b""
    if cfg.filled_bam:
        tv = bm.string_tags(tags, [bm.tag16(t) for t in cfg.tags])
        cq, uq = tv.get(bm.T_CBQ, b""), tv.get(bm.T_UMIQ, b"")
    # save_alignment's edits in its order: a tag is edited when it has a name and a value
    edits = [(out_cfg.gene, g), (out_cfg.cb_raw, raw_cb), (out_cfg.umi_raw, raw_umi), (out_cfg.cb_quality, cq), (out_cfg.umi_quality, uq)]
    edits = [(n, v) for n, v in edits if v or n in (out_cfg.cb_raw, out_cfg.umi_raw)]
    if out_cfg.read_type and m in (tm.EXONIC, tm.INTRONIC, tm.INTERGENIC):
        edits.append((out_cfg.read_type, {tm.EXONIC: out_cfg.exonic, tm.INTRONIC: out_cfg.intronic, tm.INTERGENIC: out_cfg.intergenic}[m]))
    if cb:
        edits.append((getattr(out_cfg, "cell_barcode", "CB"), cb))
    if umi:
        edits.append((getattr(out_cfg, "umi", "UB"), umi))
    edits = [(n.encode(), bytes(v)) for n, v in edits if n]
    names = {n for n, _ in edits}
    entries, stop = tm.aux_entries(tags)
    kept = b"".join(tags[a:b] for a, b, n in entries if n not in names) + tags[stop:]
    body = bytes(rec[4:4 + aux]) + kept + b"".join(n + b"Z" + v + b"\0" for n, v in edits)
    return struct.pack("<I", len(body)) + body


def filtered_stream(recs, cfg, out_cfg, decisions):
    out, k, written = [], 0, 0
    dicts = bm.Dicts(chr_of_ref=[0] * max(cfg.n_refs, 1))
    for rec in recs:
        if bm.parse_record(rec, cfg, dicts).status != bm.OK:
            continue
        verdict, cb, umi = decisions[k]
        k += 1
        r = filtered_record(rec, cfg, out_cfg, verdict, cb, umi)
        if r is not None:
            out.append(r); written += 1
    return b"".join(out), written, k
