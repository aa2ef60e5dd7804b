"""Tagged and filtered BAM output (-b, -F) under read-parameter files (-r) and gene = chromosome name (-P), restated in plain Python: TEST
INFRASTRUCTURE for dropest_bam_decoder_tag_window / _filter_window* on a decoder with sources (include/dropest_bgzf.h) and for the `.tagged.bam` /
`.filtered.bam` files of a BamController with set_device_source_output.  Written from the rules -- BamController.cpp:26-68,132-172 (a NEW parser
for the -F pass; parameters before the gene), ReadMapParamsParser.cpp:22-48 (a served name is erased; low quality takes its row),
ReadParametersEfficient.cpp:15-22 (no barcode quality), ReadParamsParser.cpp:42-50 (-P: the gene is the reference's name, mark HAS_EXONS) and
BamProcessorAbstract.cpp:65-114 (save_alignment) -- and from bam_model.py / bam_tag_model.py / read_params_model.py, not from the kernels.

  stream(recs, cfg, out_cfg, server=None, ref_names=None, annotated=None, decisions=None) -> (bytes, records written, kinds)
    server     -r: a read_params_model.Server; it is CONSUMED (a second pass takes a fresh one: rule 5)
    ref_names  -P: the references' names (bytes), by reference id; comes before `annotated` and before the gene tag
    annotated  -g: per record (gene name or b"", mark), None for a record on a chromosome the annotation lacks
    decisions  -F: (verdict, corrected barcode, corrected UMI) per ACCEPTED record, in order
    kinds      per record: WRITTEN, or why it was not"""
import struct

import bam_model as bm
import bam_tag_model as tm
import read_params_model as rp

WRITTEN, SKIPPED, NO_REFERENCE, NO_ROW, ROW_TAKEN, LOW_QUALITY, NOT_PARSED, NOT_KEPT = "written", "skipped", "no reference", "no row", "row taken", "low quality", "not parsed", "not kept"


def layout(rec):
    """(ref_id, flag, read name without its NUL, where the aux bytes begin, where the record ends)"""
    block_size, ref_id, _pos, l_read_name, _mapq, _bin, n_cigar, flag, l_seq = struct.unpack_from("<IiiBBHHHI", rec, 0)
    aux = 32 + l_read_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq
    return ref_id, flag, bytes(rec[36:36 + max(l_read_name - 1, 0)]), 4 + aux, 4 + block_size


def gene_and_mark(tags, cfg):
    """get_gene + parse_read_type (ReadParamsParser.cpp:36-90) over the record's own tags, as bam_model.parse_record has them"""
    tv = bm.string_tags(tags, [bm.tag16(t) for t in cfg.tags])
    if bm.T_GENE not in tv:
        return b"", bm.HAS_NOT_ANNOTATED
    if not cfg.read_type or bm.T_TYPE not in tv:
        return tv[bm.T_GENE], bm.HAS_EXONS
    if tv[bm.T_TYPE] == cfg.intronic:
        return tv[bm.T_GENE], bm.HAS_INTRONS
    if cfg.intergenic and tv[bm.T_TYPE] == cfg.intergenic:
        return tv[bm.T_GENE], bm.HAS_NOT_ANNOTATED
    return tv[bm.T_GENE], bm.HAS_EXONS


def save_alignment(rec, out_cfg, gene, cb, umi, cq, uq, mark, corrected=None):
    """The edit rule of -b: every reached aux entry with an edited name goes, the new tags follow as Z in the fixed order; a
    tag is edited when it has a name and (the raw two apart) a value.  corrected: -F's (barcode, UMI), behind the read type."""
    _ref, _flag, _name, aux, end = layout(rec)
    tags = bytes(rec[aux:end])
    edits = [(out_cfg.gene, gene), (out_cfg.cb_raw, cb), (out_cfg.umi_raw, umi), (out_cfg.cb_quality, cq), (out_cfg.umi_quality, uq)]
    edits = [(n, v) for n, v in edits if v or n in (out_cfg.cb_raw, out_cfg.umi_raw)]
    if out_cfg.read_type and mark in (tm.EXONIC, tm.INTRONIC, tm.INTERGENIC):
        edits.append((out_cfg.read_type, {tm.EXONIC: out_cfg.exonic, tm.INTRONIC: out_cfg.intronic, tm.INTERGENIC: out_cfg.intergenic}[mark]))
    if corrected is not None:
        edits += [(n, v) for n, v in ((getattr(out_cfg, "cell_barcode", "CB"), corrected[0]), (getattr(out_cfg, "umi", "UB"), corrected[1])) if v]
    edits = [(n.encode(), bytes(v)) for n, v in edits if n]
    names = {n for n, _ in edits}
    entries, stop = tm.aux_entries(tags)
    kept = b"".join(tags[a:b] for a, b, n in entries if n not in names) + tags[stop:]
    body = bytes(rec[4:aux]) + kept + b"".join(n + b"Z" + v + b"\0" for n, v in edits)
    return struct.pack("<I", len(body)) + body


def read(rec, cfg, server=None, ref_names=None, annotated=False):
    """One record through the reader -> (kind, (gene, cb, umi, cq, uq, mark) for an accepted one).  `annotated`: this record's -g answer (gene
    name or b"", mark), None for a record on a chromosome the annotation lacks, False without an annotation."""
    ref_id, flag, name, aux, end = layout(rec)
    if flag & 0x4 or flag & 0x100:
        return SKIPPED, None
    if ref_id < 0 or ref_id >= cfg.n_refs:
        return NO_REFERENCE, None
    tags = bytes(rec[aux:end])
    if server is not None:                                   # rules 1 and 2: the row's fields as they stand; the record's own name and tags are not asked
        key = name[1:] if name[:1] == b"@" else name
        status, row = server.serve(rp.OK, name)
        if status == rp.CANT_PARSE:
            return (ROW_TAKEN if key in server.rows.first else NO_ROW), None
        if status == rp.LOW_QUALITY:
            return LOW_QUALITY, None                         # (the row is gone all the same)
        r = server.rows.rows[row]
        cb, umi, cq, uq = r["cb"], r["umi"], b"", r["quality"]      # ReadParametersEfficient::parameters: "" for the barcode quality
    else:
        row = bm.parse_record(rec, cfg, bm.Dicts(chr_of_ref=[0] * max(cfg.n_refs, 1)))
        if row.status != bm.OK:
            return (LOW_QUALITY if row.status == bm.LOW_QUALITY else NOT_PARSED), None
        cb, umi = row.strings[0], row.strings[1]
        cq = uq = b""
        if cfg.filled_bam:
            tv = bm.string_tags(tags, [bm.tag16(t) for t in cfg.tags])
            cq, uq = tv.get(bm.T_CBQ, b""), tv.get(bm.T_UMIQ, b"")
    if ref_names is not None:                                # rule 3: before -g and the gene tag; an empty name is no gene and mark 0
        gene = bytes(ref_names[ref_id])
        mark = bm.HAS_EXONS if gene else 0
    elif annotated is not False:                             # rule 4 (False: there is no annotation)
        if annotated is None:
            return NOT_PARSED, None                          # the chromosome is not in the annotation: after the row was taken
        gene, mark = annotated
    else:
        gene, mark = gene_and_mark(tags, cfg)
    return WRITTEN, (gene, cb, umi, cq, uq, mark)


def stream(recs, cfg, out_cfg, server=None, ref_names=None, annotated=None, decisions=None):
    out, kinds, k = [], [], 0
    for i, rec in enumerate(recs):
        kind, s = read(rec, cfg, server, ref_names, annotated[i] if annotated is not None else False)
        if kind == WRITTEN and decisions is not None:        # rule 5: entry k belongs to the k-th accepted record
            verdict, ccb, cumi = decisions[k]
            k += 1
            if verdict != 0:
                kind = NOT_KEPT
            else:
                out.append(save_alignment(rec, out_cfg, *s, corrected=(ccb, cumi)))
        elif kind == WRITTEN:
            out.append(save_alignment(rec, out_cfg, *s))
        kinds.append(kind)
    return b"".join(out), sum(1 for x in kinds if x == WRITTEN), kinds


def accepted(kinds):
    """records that reach write_alignment (the container's reads): written or not kept"""
    return sum(1 for x in kinds if x in (WRITTEN, NOT_KEPT))
