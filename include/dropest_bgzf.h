/* dropest_bgzf.h -- BGZF blocks inflated on the device (the BAM reader that feeds the path).
 *
 * What it replaces: BamTools' BgzfStream (zlib inflate, one block at a time) under BamReader::GetNextAlignment, the loop of
 * Estimation/BamProcessing/BamController.cpp:85.  A BGZF block (SAMv1 §4.1) is an independent DEFLATE stream of at most 64 KB:
 * dropest_bgzf_scan walks the block headers on the host (18 + 8 bytes per block), dropest_bgzf_inflate_device decodes every block
 * with one 64-lane wave whose lanes take different chunks of the block's symbol stream (csrc/k_inflate_par.h; csrc/k_inflate.h, one chain of
 * symbols per block, behind DROPEST_INFLATE_PAR=0 -- both written from RFC 1951).  Plain C, no torch types.
 *
 * Checked on the device: every Huffman code, distance and length, the input and output bounds, ISIZE, and the block's CRC-32 (the wave
 * that inflated a block reads it back: 64 partial CRCs joined in GF(2)).  A block the device refuses (status != 0: damaged, or a CRC that
 * does not match) is left for the caller to inflate elsewhere; nothing outside its own output range is written. */
#ifndef DROPEST_BGZF_H
#define DROPEST_BGZF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Walks the BGZF blocks of data[0 .. len): for block k the DEFLATE payload is data[in_off[k] .. + in_len[k]), its ISIZE bytes belong at
 * out_off[k] (running sum) and number out_len[k]; crc32[k] is the stored CRC-32 (may be NULL).  Stops at `cap` blocks, at a block that
 * is not complete inside the buffer, or at the end; *bytes_used = offset of the first byte not consumed.  0 = ok, 1 = not a BGZF header. */
int dropest_bgzf_scan(const uint8_t *data, uint64_t len, uint64_t cap, uint64_t *in_off, uint32_t *in_len, uint64_t *out_off,
                      uint32_t *out_len, uint32_t *crc32, uint64_t *n_blocks, uint64_t *bytes_used, uint64_t *out_total);

/* Every pointer is DEVICE memory of `device`; d_in 8-byte aligned, in_total = bytes of d_in that may be read.  Asynchronous on `stream`
 * (a hipStream_t, NULL = the default stream).  d_status[k] = 0 when block k came out whole. */
int dropest_bgzf_inflate_device(int device, void *stream, const uint8_t *d_in, uint64_t in_total, const uint64_t *d_in_off,
                                const uint32_t *d_in_len, const uint64_t *d_out_off, const uint32_t *d_out_len, uint32_t n_blocks,
                                uint8_t *d_out, uint32_t *d_status, const uint32_t *d_crc32 /* stored CRC-32 per block, or NULL: not checked */);

/* Host buffer in, host buffer out (tests, scripts/bench_bgzf_inflate.py): scan + upload + kernel (`repeats` times; *kernel_ms = mean
 * of the runs by HIP events; repeats < 0: |repeats| runs WITHOUT the CRC-32 check) + download.  status[0 .. min(n_blocks, status_cap)) per block.  Returns 0, or 1 with
 * dropest_bgzf_last_error() set (no GPU, out_cap too small, not BGZF). */
int dropest_bgzf_inflate_buffer(int device, const uint8_t *data, uint64_t len, uint8_t *out, uint64_t out_cap, uint64_t *out_len,
                                uint32_t *status, uint64_t status_cap, uint64_t *n_blocks, double *kernel_ms, int repeats);

/* ---- BAM records of a window of BGZF blocks, on the device (csrc/k_bamparse.h; csrc/bam_decoder*.h) -------------------------------------------------------
 * What BamController::process_alignment (BamController.cpp:132-172) decides without a dictionary: the reader's status of a record, the
 * 2-bit codes of its barcode and UMI, its UMI::Mark, and -- against a copy of the caller's dictionaries -- its gene and chromosome index:
 * the accepted records leave as the four dense columns of dropest_push_reads IN DEVICE MEMORY (dropest_push_reads_device takes them as
 * they are).  The dictionaries themselves (gene names, chromosomes, strings with N) stay with the caller, who asks for the bytes of the
 * few records that bring something new, resolves them in file order and patches their rows. */
typedef struct dropest_bam_decoder dropest_bam_decoder;

typedef struct dropest_bam_parse_cfg {
	uint16_t tag[6];          /* cell barcode, UMI, barcode quality, UMI quality, gene, read type (BamTags.cpp:7-24): letters lo | hi << 8, 0 = none */
	int32_t filled_bam;       /* -f: 1 = barcode / UMI from tags (FilledBamParamsParser), 0 = from the read name "id!CB#UMI" */
	int32_t min_phred;        /* min_barcode_phred as a character code (33 + score); the filter is on when > 33 */
	int32_t has_read_type;
	int32_t n_refs;
	uint32_t intronic_len, intergenic_len;
	uint8_t intronic[24], intergenic[24];
} dropest_bam_parse_cfg;

enum { DROPEST_BAM_OK = 0, DROPEST_BAM_SKIP = 1, DROPEST_BAM_CANT_PARSE_NO_COUNT = 2, DROPEST_BAM_CANT_PARSE = 3, DROPEST_BAM_LOW_QUALITY = 4 };

typedef struct dropest_bam_window {        /* host pointers: pinned memory of the decoder; d_*: DEVICE memory; all valid until its next window */
	uint64_t n_records;                    /* complete records that START in this window (the cut-off last one opens the next window) */
	uint64_t counts[5];                    /* records per DROPEST_BAM_* status */
	uint64_t n_accepted;                   /* = counts[DROPEST_BAM_OK]: rows of the dense columns below, in file order */
	const uint64_t *d_cb, *d_umi;          /* the columns of dropest_push_reads (dropest_amd.h), as BamController's bulk path fills them: */
	const uint32_t *d_gene, *d_aux;        /*   gene = index from the dictionary given to the decoder, aux = chromosome index | mark << 16 */
	uint32_t n_need;                       /* accepted records the caller must see as bytes (a gene or chromosome the dictionaries lack, an N): */
	const uint32_t *need_rec, *need_pos, *need_size;   /* record of the window, its row in the dense columns, its bytes (block_size field included) */
	uint32_t quality_seen, any_gene;       /* an accepted record carries a UMI quality tag / a gene name */
	uint64_t window_bytes, tail_bytes;     /* inflated bytes looked at; bytes of the cut-off last record carried over */
	uint32_t n_blocks, refused_blocks;     /* blocks the device left to `inflate_fallback` */
	uint32_t guesses_repaired, pad;        /* segments whose guessed first record was not on the chain (walked again from the true place) */
	double ms_inflate, ms_boundaries, ms_parse, ms_copy;
	uint32_t quality_len_min, quality_len_max;   /* shortest / longest UMI quality string over the accepted GENE-BEARING reads, true lengths (0 = none) */
} dropest_bam_window;

/* raw DEFLATE of one block on the host (zlib or the like) for the blocks the device refuses; 0 = ok */
typedef int (*dropest_bgzf_host_inflate)(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_len, void *user);

/* Loads this path's kernels onto the current device (their first launch otherwise does, ~10 ms); dropest_ctx_create calls it. */
void dropest_bgzf_warm_up(void *stream);
int dropest_bam_decoder_create(int device, const dropest_bam_parse_cfg *cfg, dropest_bam_decoder **out);
/* The decoder for another file: its device buffers, streams and pinned memory stay (creating and freeing them is ~60 ms per file), the
 * dictionaries are emptied, the annotation and the record carried over are dropped. */
int dropest_bam_decoder_reset(dropest_bam_decoder *d, const dropest_bam_parse_cfg *cfg);
/* Blocks the device inflates at the same time (one wave each): a window of that many blocks takes about as long as a window of fewer. */
uint32_t dropest_bam_decoder_wave_slots(const dropest_bam_decoder *d);
/* Two pinned host buffers of the decoder for the caller's compressed bytes (which = 0 / 1, at least `bytes` long): a window handed over from
 * one of them crosses PCIe at the link's rate; any other host memory works too (pageable memory is staged by the runtime at a third of it). */
int dropest_bam_decoder_staging(dropest_bam_decoder *d, int which, uint64_t bytes, uint8_t **out);
/* The first `len` bytes of staging buffer `which` start for the device now, on a stream of their own; the window call that is given exactly that
 * buffer and length then waits for this copy instead of making one.  For a reader thread that calls it when its read is done: the copy of
 * window k + 1 runs under the kernels of window k.  The one decoder call that may run beside a window call; allocates nothing; a length the
 * buffers were not sized for is left to the window call (0 is returned all the same). */
int dropest_bam_decoder_upload(dropest_bam_decoder *d, int which, uint64_t len);
/* The same road in pieces, so that the pinned memory (0.15-0.4 ms per MB to allocate: 35-65 ms for two windows of 128 MB) does not grow with the
 * window: .._reserve sizes the device side of up-buffer / front `which` for windows of `bytes` compressed bytes; .._pieces makes n pinned pieces
 * of `bytes` each (out[k] = piece k); a reader fills a piece (.._piece_wait(piece) first: the copy that read it last is through), sends its
 * first `len` bytes to byte `dst_off` of up-buffer `which` (.._upload_piece: asynchronous, callable from several threads on different pieces),
 * and when a window's pieces are all on their way says what the buffer holds: .._upload_done(which, host, len, blocks) -- `host` are the same bytes in
 * host memory of any kind (the mapped file), from which the block table is made and which the window call is then given
 * (dropest_bam_decoder_window(d, host, len, ...)); they stay readable until that call has returned. */
int dropest_bam_decoder_reserve(dropest_bam_decoder *d, int which, uint64_t bytes, uint64_t inflated_bytes /* what such a window inflates to, if the caller knows (0: 14 x bytes) */);
int dropest_bam_decoder_pieces(dropest_bam_decoder *d, uint32_t n, uint64_t bytes, uint8_t **out);
int dropest_bam_decoder_piece_wait(dropest_bam_decoder *d, uint32_t piece);
int dropest_bam_decoder_upload_begin(dropest_bam_decoder *d, int which);   /* before a window's first piece: picks the stream its pieces travel on */
int dropest_bam_decoder_upload_piece(dropest_bam_decoder *d, int which, uint32_t piece, uint64_t dst_off, uint64_t len);
/* blocks != NULL: the window's block table as the caller found it while reading the file (block k: payload at in_off[k], in_len[k] bytes long, ISIZE
 * out_len[k], CRC-32 crc32[k]); `host` is then read only if the device refuses a block. */
typedef struct { uint64_t n; const uint64_t *in_off; const uint32_t *in_len, *out_len, *crc32; } dropest_bgzf_blocks;
int dropest_bam_decoder_upload_done(dropest_bam_decoder *d, int which, const uint8_t *host, uint64_t len, const dropest_bgzf_blocks *blocks);
/* The decoder's kernels run on `stream` (a hipStream_t of its device that the caller lends: one that exists and has run kernels saves the ~16 ms
 * a new stream and its first dispatch cost) until NULL gives it back -- before that stream is destroyed.  Not while a window is in flight. */
int dropest_bam_decoder_use_stream(dropest_bam_decoder *d, void *stream);
void dropest_bam_decoder_destroy(dropest_bam_decoder *d);
/* comp[0 .. len): whole BGZF blocks, following the previous window's.  first_skip: bytes of the first block to pass over (the BAM header;
 * first window only).  final != 0: the file ends here (a cut-off record is then an error). */
int dropest_bam_decoder_window(dropest_bam_decoder *d, const uint8_t *comp, uint64_t len, uint32_t first_skip, int final,
                               dropest_bgzf_host_inflate inflate_fallback, void *user, dropest_bam_window *out);
/* The same in two halves, for a caller that overlaps windows: _begin (copy in, inflate, the chain of records; needs no dictionary) of window
 * k + 1 may run on ANOTHER THREAD while _finish (fields against the dictionaries, dense columns) of window k and the caller's own work go on.
 * Windows are begun in file order, one at a time; a window is finished before the one after the next is begun (two sets of buffers). */
int dropest_bam_decoder_window_begin(dropest_bam_decoder *d, const uint8_t *comp, uint64_t len, uint32_t first_skip, int final,
                                     dropest_bgzf_host_inflate inflate_fallback, void *user, int *slot);
int dropest_bam_decoder_window_finish(dropest_bam_decoder *d, int slot, dropest_bam_window *out);
/* _begin in two parts, for ONE thread that keeps the device busy (round 6; what BamController::parse_bam_files does on the device path,
 * BamProcessing/BamController.cpp:70-116): _inflate enqueues the copies and the inflate kernel of a window and returns at once -- it needs
 * nothing from the window before, so window k + 1 is given to the device BEFORE the caller waits for window k; _chain then waits for the
 * inflate of `slot`, puts the record the window before cut off in front of the data and finds the chain of records (windows take _chain in
 * file order).  The order per window k:  _inflate(k + 1); _chain(k); _finish(k).  comp must stay untouched until _chain has returned. */
int dropest_bam_decoder_window_inflate(dropest_bam_decoder *d, const uint8_t *comp, uint64_t len, int *slot);
int dropest_bam_decoder_window_chain(dropest_bam_decoder *d, int slot, uint32_t first_skip, int final, dropest_bgzf_host_inflate inflate_fallback, void *user);
/* The dictionaries the records are looked up in (copied): gene_hash[k] (FNV-1a of the name) -> gene_id[k]; chr_of_ref[r] = chromosome
 * index of reference r, -1 = none yet.  Call again whenever they have grown. */
int dropest_bam_decoder_set_dictionaries(dropest_bam_decoder *d, const uint64_t *gene_hash, const uint32_t *gene_id, uint32_t n_genes,
                                         const int32_t *chr_of_ref, uint32_t n_refs);
/* The names of the dictionary's genes by index (name k = pool[off[k] .. off[k + 1]), n_names + 1 offsets): a gene found by its hash is then
 * confirmed byte by byte on the device, and a name that only shares the FNV-1a value of another comes back to the host like an unseen one
 * (CellsDataContainer::intern_gene compares the bytes: Estimation/StringIndexer.cpp:10-18 keys by the string itself).  Optional: without it
 * the hash alone decides.  Call after _set_dictionaries, whenever the dictionary has grown. */
int dropest_bam_decoder_set_gene_names(dropest_bam_decoder *d, const uint32_t *off, const uint8_t *pool, uint32_t n_names);
/* -g: genes from a GTF / BED annotation instead of the gene tag (ReadParamsParser::get_gene_from_reference, ReadParamsParser.cpp:92-151): the
 * decoder asks `a` (dropest_annotation.h, same GPU; stays the caller's) about the two ends of every accepted alignment.  ann_chr_of_ref[r] =
 * the annotation's chromosome for reference r, -1 = it has none of that name (such a record cannot be parsed, BamController.cpp:153-161).
 * _annotation_genes: id_of_ann_gene[g] = index of the annotation's gene g in the caller's gene dictionary, -1 = not in it yet (a record
 * that names it comes back through need_*); call again whenever the dictionary has grown. */
struct dropest_annotation;
int dropest_bam_decoder_set_annotation(dropest_bam_decoder *d, struct dropest_annotation *a, const int32_t *ann_chr_of_ref, uint32_t n_refs);
int dropest_bam_decoder_set_annotation_genes(dropest_bam_decoder *d, const int32_t *id_of_ann_gene, uint32_t n);
/* the bytes of records idx[0 .. n) of the LAST window (block_size field first), one after the other: dst_off[k] = where record idx[k] starts in dst */
int dropest_bam_decoder_fetch_records(dropest_bam_decoder *d, const uint32_t *idx, uint32_t n, uint8_t *dst, uint64_t dst_cap, uint64_t *dst_off);
/* The dense columns of the LAST window copied to host arrays of n_accepted entries each (any of them may be NULL): for a caller that keeps its
 * reads on the host after all. */
int dropest_bam_decoder_columns_to_host(dropest_bam_decoder *d, uint64_t *cb, uint64_t *umi, uint32_t *gene, uint32_t *aux);
/* One row of ql bytes per accepted read of the LAST window, in the order of the dense columns, in pinned HOST memory: the read's UMI quality string
 * (zeros for a read without a gene).  For a window whose quality_len_min == quality_len_max == ql. */
int dropest_bam_decoder_quality_rows(dropest_bam_decoder *d, uint32_t ql, const uint8_t **rows);
/* rows pos[0 .. n) of the LAST window's dense columns take these values (what the caller resolved for the `need` records) */
int dropest_bam_decoder_patch(dropest_bam_decoder *d, const uint32_t *pos, const uint64_t *cb, const uint64_t *umi, const uint32_t *gene,
                              const uint32_t *aux, uint32_t n);

/* ---- -r: read-parameter files as a table on the device (csrc/k_readparams.h, csrc/bam_read_params.h; DESIGN.md section 7 has the rules) ---------------
 * What ReadMapParamsParser (ReadMapParamsParser.cpp:22-108) keeps in an unordered_map: read name -> barcode, UMI, UMI quality, quality verdict, each
 * name serving ONE record, the first of the file order that asks.  The caller inflates the gzip files and finds the line starts; the rows are
 * validated, packed, hashed and entered on the device.  An object of its own: decoders come and go per file, the table and its claims stay.  Every
 * call returns with its work done; none may run while a window of a decoder that was given the table is in flight. */
typedef struct dropest_read_params dropest_read_params;
typedef struct dropest_read_params_row {   /* one line of the files; offsets into the table's text = the bytes of every _add_text call, one after the other */
	uint64_t hash;                         /* FNV-1a 64 of the name (under the table's hash mask) */
	uint64_t cb_code, umi_code;            /* packed codes of dropest_amd.h; 0 = does not pack (an N, more than 31 bases): the caller spells it from the text */
	uint64_t name_off, cb_off, umi_off, quality_off;      /* the name without its '@'; the UMI quality is the fifth field, the rest of the line */
	uint32_t name_len, cb_len, umi_len, quality_len;
	uint32_t canonical;                    /* the first row that carries this name (the row itself when it is that one): the row look-ups answer with; 0xFFFFFFFF when !valid */
	uint8_t valid, pass, empty, pad;       /* valid: five fields, barcode and UMI not empty; pass: the quality verdict; empty: the line has no character */
} dropest_read_params_row;
/* hash_bits in 1 .. 63: only that many bits of a name's hash are used (tests: names that collide); anything else: all 64. */
int dropest_read_params_create(int device, int hash_bits, dropest_read_params **out);
/* text[0 .. len): lines of "name cb umi cb_quality umi_quality"; line k begins at line_off[k] and ends where line k + 1 begins (the last one at len),
 * its '\n' included if it has one.  min_phred as in dropest_bam_parse_cfg.  Callable several times before _build (one call per file, say): row
 * numbers go on counting, and a name met again keeps its FIRST row, across calls too.  The text is copied. */
int dropest_read_params_add_text(dropest_read_params *t, const uint8_t *text, uint64_t len, const uint64_t *line_off, uint64_t n_lines, int min_phred);
int dropest_read_params_build(dropest_read_params *t);      /* once; the table is of the power of two >= 2 x rows (at least 64) slots */
/* rows: lines; valid; malformed: neither valid nor empty; repeated: valid rows whose name an earlier row carries.  Any pointer may be NULL. */
int dropest_read_params_counts(dropest_read_params *t, uint64_t *rows, uint64_t *valid, uint64_t *malformed, uint64_t *repeated);
int dropest_read_params_rows_to_host(dropest_read_params *t, uint64_t first, uint64_t n, dropest_read_params_row *out);
/* name k = name_pool[name_off[k] .. name_off[k + 1]) (n + 1 offsets; one '@' in front is passed over, as for a record's name) -> out_row[k] = its
 * canonical row, 0xFFFFFFFF = not listed.  The device function the decoder's parse kernel calls, a lane per name.  Claims nothing. */
int dropest_read_params_lookup(dropest_read_params *t, const uint8_t *name_pool, const uint64_t *name_off, uint64_t n, uint32_t *out_row);
/* claim[row]: the lowest stream ordinal among the records that found the row (dropest_bam_decoder_set_read_params), all ones = none did: a row with
 * a claim is consumed, for the table's life or until _reset_claims. */
int dropest_read_params_claims_to_host(dropest_read_params *t, uint64_t first, uint64_t n, uint64_t *out);
int dropest_read_params_reset_claims(dropest_read_params *t);
/* A second pass over the same stream (-F: the reference makes a new parser for write_filtered_bam_files, ReadMapParamsParser and all, so every row
 * serves afresh).  _replay_begin puts a fresh claim array, all ones, in the table's place for claims; the array that was current stays untouched
 * beside it and _replay_end puts it back.  In between every decoder window, _claims_to_host and _reset_claims work on the fresh array, and the
 * first file's decoder is given first_ordinal 0 (dropest_bam_decoder_set_read_params: the caller counts, as ever).  One replay at a time. */
int dropest_read_params_replay_begin(dropest_read_params *t);
int dropest_read_params_replay_end(dropest_read_params *t);
void dropest_read_params_destroy(dropest_read_params *t);
/* The decoder takes barcode, UMI and UMI quality of every record from `table` (same GPU; stays the caller's) by the read's name, one '@' off.  A
 * record that is neither skipped nor on an unknown reference claims the row it finds with its stream ordinal: first_ordinal + the records of the
 * windows finished since this call + its index in the window.  A launch behind the parse serves the record whose ordinal stands in the claim: no
 * row, or a row claimed by an earlier record -> DROPEST_BAM_CANT_PARSE; a row that fails the quality filter -> DROPEST_BAM_LOW_QUALITY (the row is
 * taken all the same); else the row's codes and quality string are the record's (a code of 0 makes it a need record).  first_ordinal must lie above
 * every ordinal that claimed a row of the table before.  NULL turns it off, as a reset does.  Refused under -f.  With tagged output
 * (dropest_bam_decoder_set_tagging, in either order) the raw barcode, the raw UMI and the UMI quality tag of a written record are the served row's
 * fields as they stand in the line; no barcode quality tag is written (ReadParametersEfficient::parameters answers "" for it) and an entry of
 * that name stays in the record. */
int dropest_bam_decoder_set_read_params(dropest_bam_decoder *d, dropest_read_params *table, uint64_t first_ordinal);
/* -P (gene = chromosome name, ReadParamsParser.cpp:42-48): gene_of_ref[r] = index of reference r's name in the caller's gene dictionary, -1 = not in
 * it yet (a record on r is a need record; send the table again once the dictionary has grown), -2 = the name is empty (no gene, mark 0).  Other
 * records carry mark HAS_EXONS.  Comes before an annotation and the gene tag; the read type is not looked at.  NULL turns it off, as a reset does. */
int dropest_bam_decoder_set_gene_of_reference(dropest_bam_decoder *d, const int32_t *gene_of_ref, uint32_t n_refs);
/* -P with tagged output: the references' names, name r = pool[off[r] .. off[r + 1]) (n_names + 1 offsets; HOST memory, copied), which the tag
 * kernels write as the gene tag of a record on reference r (an empty name: no gene tag, no read type).  .._tag_window / .._filter_window* under -P
 * without them fail and name this call.  A written record whose reference id is not below n_names makes them fail too (nothing is loaded from
 * there).  n_names = 0 drops the names, as a reset does. */
int dropest_bam_decoder_set_reference_names(dropest_bam_decoder *d, const uint32_t *off, const uint8_t *pool, uint32_t n_names);
/* For records rec_idx[0 .. n) of the LAST window (NULL: its first n records): the row of the table each was served (a row that fails the quality
 * filter included), 0xFFFFFFFF for every other record. */
int dropest_bam_decoder_param_rows(dropest_bam_decoder *d, const uint32_t *rec_idx, uint32_t n, uint32_t *out_rows);

/* ---- -b: tagged BAM output (csrc/k_bamtag.h, csrc/bam_decoder_tag.h; DESIGN.md section 7 has the edit rule) ---------------------------------------------------
 * What BamProcessorAbstract::save_alignment (BamProcessorAbstract.cpp:65-114) writes for every accepted alignment: the record with its gene, raw
 * barcode, raw UMI, the two quality strings and the read type as Z tags.  Every aux entry the tag walk reaches whose name is one of the edited
 * names is left out (every occurrence, whatever its type); the edited tags are appended in the order gene, raw barcode, raw UMI, barcode quality,
 * UMI quality, read type; everything else in the record is a byte copy.  The gene tag is edited when the record has a gene, a quality tag when
 * the string is not empty (-f only), the read type when a tag is configured and the mark is exactly exonic (2), intronic (4) or intergenic (1). */
typedef struct dropest_bam_tag_cfg {
	uint16_t out_tag[5];                 /* gene, raw barcode, raw UMI, barcode quality, UMI quality: letters lo | hi << 8 (0 = never written; not the raw two) */
	uint16_t type_tag;                   /* read type, 0 = none */
	uint32_t type_len[3];                /* out-values for an exonic, intronic, intergenic read: at most 24 bytes each */
	uint8_t type_val[3][24];
	/* -g (a decoder with an annotation): the annotation's gene names by ITS gene index, name g = pool[off[g] .. off[g + 1]); HOST memory, copied */
	const uint32_t *gene_name_off;
	const uint8_t *gene_name_pool;
	uint32_t n_gene_names;
} dropest_bam_tag_cfg;
/* NULL turns tagging off; so does dropest_bam_decoder_reset (the names are the annotation's, which a reset drops). */
int dropest_bam_decoder_set_tagging(dropest_bam_decoder *d, const dropest_bam_tag_cfg *cfg);
/* Tags the LAST window (after .._window, or after .._window_finish in either window order; before the next window call): *d_out = the output
 * records of its accepted records one after the other in file order, in a DEVICE buffer of the decoder that stays valid until the next window is
 * tagged; *len its bytes, *n_written its records (= counts[DROPEST_BAM_OK]).  The kernels run on the decoder's stream; the call waits once, for
 * the total that sizes the output, and returns with the emit kernel queued: work queued on that stream afterwards (dropest_bam_decoder_stream)
 * sees the bytes, .._tagged_to_host waits for them.  Returns 0; 1 with the error set (tagging is off, ...); 2 when, under -g, the annotation
 * query left the gene of some accepted reads to the host (more transcripts at an end point than it holds: exactly the records of the window's
 * need list may be such): nothing was written, the caller gives the host's answer for them with .._patch_annotation and calls again. */
int dropest_bam_decoder_tag_window(dropest_bam_decoder *d, const uint8_t **d_out, uint64_t *len, uint64_t *n_written);
/* -g: for records rec[0 .. n) of the LAST window, the annotation's gene (its index in the annotation, 0xFFFFFFFF = none) and the UMI::Mark bits
 * as the host decided them; read by the tag kernels only (the dense columns take the host's answer through .._patch). */
int dropest_bam_decoder_patch_annotation(dropest_bam_decoder *d, const uint32_t *rec, const uint32_t *ann_gene, const uint32_t *mark, uint32_t n);
/* the bytes of the last tagged window to host memory (callers and tests that want them there) */
int dropest_bam_decoder_tagged_to_host(dropest_bam_decoder *d, uint8_t *dst, uint64_t cap);
/* Since the decoder was created or reset: the time of the tag kernels (plan, scan, emit) by device events, the inflated bytes of the windows
 * they looked at and the bytes they wrote (waits for the last emit).  Any pointer may be NULL. */
int dropest_bam_decoder_tag_stats(dropest_bam_decoder *d, double *kernel_ms, uint64_t *bytes_in, uint64_t *bytes_out);
/* ---- -F: filtered BAM output (the filtered mode of csrc/k_bamtag.h; DESIGN.md section 7 has the rule) ---------------------------------------------------
 * What FilteringBamProcessor::write_alignment (FilteringBamProcessor.cpp:61-96) writes: an accepted alignment only when the container's verdict for
 * it is 0 (dropest_read_corrections, dropest_amd.h), through the same save_alignment -- the edits of -b, then the corrected cell barcode (the target
 * cell's) and the corrected UMI as two more Z tags behind the read type, under the same rule; a value of no character writes no tag and drops none.
 * The values are packed codes of dropest_amd.h (plain, or DROPEST_ESCAPE | k for side string k); the kernels spell them. */
typedef struct dropest_bam_filter_cfg {
	uint16_t out_tag[2];                 /* corrected cell barcode ("CB"), corrected UMI ("UB"): letters lo | hi << 8, 0 = never written */
	uint32_t on_device;                  /* cell_barcode is DEVICE memory of the decoder's GPU that stays valid while filtering is on; 0: host memory, copied */
	const uint64_t *cell_barcode;        /* every cell's barcode as a code, by cell id */
	uint32_t n_cells;
	uint32_t n_side;                     /* the strings of escaped codes, string k = side_pool[side_off[k] .. side_off[k + 1]); HOST memory, copied */
	const uint32_t *side_off;
	const uint8_t *side_pool;
} dropest_bam_filter_cfg;
/* After dropest_bam_decoder_set_tagging, from which the other six tags come (a later _set_tagging turns filtering off again, as a reset does).  NULL
 * turns it off.  Refused: two output tags with one name. */
int dropest_bam_decoder_set_filtering(dropest_bam_decoder *d, const dropest_bam_filter_cfg *cfg);
/* The filtered twin of .._tag_window for the LAST window.  verdict / cell / umi: the decisions of the window's accepted records in file order --
 * entry k belongs to the k-th accepted record; n must be the window's n_accepted.  on_device != 0: device arrays (dropest_read_corrections'
 * pointers offset to the window's first accepted read); 0: host arrays, uploaded through the decoder's pinned staging.  Which record takes which
 * entry is found on the device.  *len = 0 and *n_written = 0 when no read of the window is written.  Returns as .._tag_window does (2: -g left
 * genes to the host; .._patch_annotation, then call again); 1 as well when the decision of a read that is written names a cell >= n_cells or a
 * side string >= n_side (nothing is loaded from there, nothing is written).  The bytes: *d_out, or .._tagged_to_host.  .._tag_window on the same
 * window afterwards still gives the -b bytes. */
int dropest_bam_decoder_filter_window(dropest_bam_decoder *d, const uint8_t *verdict, const uint32_t *cell, const uint64_t *umi, uint64_t n, int on_device,
                                      const uint8_t **d_out, uint64_t *len, uint64_t *n_written);
/* .._filter_window for decisions that stand in SEGMENTS, as the shards of a sharded run hold them (dropest_shard_read_corrections, dropest_amd.h:
 * read i's decision lives with the shard whose resident range holds ordinal i, and a window crosses up to one boundary per shard).  Segment s
 * holds the decisions of the next `count` accepted records of the window, entry 0 first; the counts must sum to the window's n_accepted, a count
 * of 0 is legal anywhere (its pointers are not looked at).  The arrays are DEVICE memory of GPU `device`, finished (nothing queued still writes
 * them).  Segments on the decoder's GPU are read where they are -- only the table of segments travels, through the decoder's pinned staging;
 * segments on another GPU are copied into the decoder's staging first, on its stream (that hop has never run: DESIGN.md section 7;
 * DROPEST_BAM_TEST_STAGE_SEGMENTS=1 sends every segment through the staging).  A decision's `cell` indexes the cell_barcode table of
 * .._set_filtering, whatever that table lists (a sharded run: the columns of dropest_shard_filtered_barcodes_device).  Returns as .._filter_window. */
typedef struct dropest_bam_decision_segment {
	uint64_t count;
	const uint8_t *verdict;
	const uint32_t *cell;
	const uint64_t *umi;
	int32_t device;
} dropest_bam_decision_segment;
int dropest_bam_decoder_filter_window_segments(dropest_bam_decoder *d, const dropest_bam_decision_segment *seg, uint32_t n_seg, const uint8_t **d_out, uint64_t *len,
                                               uint64_t *n_written);
/* The hipStream_t the decoder's kernels run on (lent or its own): work a caller queues there follows the tagged bytes in order. */
void *dropest_bam_decoder_stream(dropest_bam_decoder *d);

const char *dropest_bgzf_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
