"""What one accepted BAM record becomes in the tagged BAM output (-b), restated in plain Python: TEST INFRASTRUCTURE for
dropest_bam_decoder_tag_window (include/dropest_bgzf.h) and the `.tagged.bam` files of BamController::parse_bam_files(files, true, container).
Written from the edit rule of DESIGN.md §7 (BamProcessorAbstract::save_alignment, BamProcessorAbstract.cpp:65-114) and from bam_model.py -- not
from the kernels.

  tagged_record(rec, cfg, out_cfg, gene_name=None, mark=None) -> the output record's bytes (block_size field first), or None for a record
  that is not written (any status but OK)."""
import struct
from dataclasses import dataclass

import bam_model as bm

EXONIC, INTRONIC, INTERGENIC = bm.HAS_EXONS, bm.HAS_INTRONS, bm.HAS_NOT_ANNOTATED


@dataclass
class OutCfg:
    """dropest_bam_tag_cfg in Python terms: the output tag names ("" = never written) and the read-type out-values by mark."""
    gene: str = "GX"
    cb_raw: str = "CR"
    umi_raw: str = "UR"
    cb_quality: str = "CQ"
    umi_quality: str = "UQ"
    read_type: str = ""
    exonic: bytes = b"EXONIC"              # BamTags.cpp:19-21, unless an in-value is configured
    intronic: bytes = b"INTRONIC"
    intergenic: bytes = b"INTERGENIC"


def aux_entries(tags):
    """The walk of BamRecord::get_string_tags over the aux bytes (bam_model.string_tags has the rules): [(start, end, name)] for every entry
    the walk reaches, and where it stopped (the bytes from there on are not looked at)."""
    out = []
    o, n = 0, len(tags)
    while o + 3 <= n:
        name, typ = bytes(tags[o:o + 2]), tags[o + 2]
        v = o + 3
        if typ in b"AcC":
            ln = 1
        elif typ in b"sS":
            ln = 2
        elif typ in b"iIf":
            ln = 4
        elif typ in b"ZH":
            e = tags.find(b"\0", v)
            if e < 0:
                break
            ln = e - v + 1
        elif typ == ord("B"):
            if v + 5 > n:
                break
            w = 1 if tags[v] in b"cC" else 2 if tags[v] in b"sS" else 4
            ln = 5 + struct.unpack_from("<I", tags, v + 1)[0] * w
        else:
            break
        if v + ln > n:
            break
        out.append((o, v + ln, name))
        o = v + ln
    return out, o


def tagged_record(rec, cfg, out_cfg, gene_name=None, mark=None):
    """rec: the input record's bytes; cfg: bam_model.Cfg (how the record is read); out_cfg: OutCfg.  gene_name / mark override what
    bam_model.parse_record finds (-g: the annotation's gene, b"" for none, and its mark)."""
    row = bm.parse_record(rec, cfg, bm.Dicts(chr_of_ref=[0] * max(cfg.n_refs, 1)))
    if row.status != bm.OK:
        return None
    cb, umi, g, _ref, m = row.strings
    if gene_name is not None:
        g = gene_name
    if mark is not None:
        m = mark
    block_size, l_read_name, n_cigar, l_seq = struct.unpack_from("<I", rec, 0)[0], rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<I", rec, 20)[0]
    aux = 32 + l_read_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq
    tags = bytes(rec[4 + aux:4 + block_size])
    cq = uq = b""
    if cfg.filled_bam:                                   # the quality strings exist under -f only (ReadParamsParser builds its parameters without them)
        tv = bm.string_tags(tags, [bm.tag16(t) for t in cfg.tags])
        cq, uq = tv.get(bm.T_CBQ, b""), tv.get(bm.T_UMIQ, b"")
    edits = []
    if g:
        edits.append((out_cfg.gene, g))
    edits += [(out_cfg.cb_raw, cb), (out_cfg.umi_raw, umi)]
    if cq:
        edits.append((out_cfg.cb_quality, cq))
    if uq:
        edits.append((out_cfg.umi_quality, uq))
    if out_cfg.read_type and m in (EXONIC, INTRONIC, INTERGENIC):      # a spanning mark (several bits) writes none
        edits.append((out_cfg.read_type, {EXONIC: out_cfg.exonic, INTRONIC: out_cfg.intronic, INTERGENIC: out_cfg.intergenic}[m]))
    edits = [(n.encode(), v) for n, v in edits if n]
    names = {n for n, _ in edits}
    entries, stop = aux_entries(tags)
    kept = b"".join(tags[a:b] for a, b, n in entries if n not in names) + tags[stop:]
    body = bytes(rec[4:4 + aux]) + kept + b"".join(n + b"Z" + bytes(v) + b"\0" for n, v in edits)
    return struct.pack("<I", len(body)) + body
