// k_bamtag.h -- tagged BAM output (-b) on the device: the accepted records of a decoded window, written again with their raw barcode, raw UMI,
// gene and read type as tags.
//
// What it replaces: BamProcessor::write_alignment -> BamProcessorAbstract::save_alignment (Estimation/BamProcessing/BamProcessorAbstract.cpp:65-114):
// BamTools' EditTag per tag (remove the tag, append it as Z) and BamWriter::SaveAlignment per read.  Here a record's output is its input bytes with
// the spans of the edited tags left out and the new tags appended, so the work is ONE walk over the aux bytes and a copy (DESIGN.md §7 has the rule).
//
// How lanes map to records and bytes: ONE WAVE PER RECORD, four records per workgroup of 256.  The walk over the aux bytes is done by the whole wave
// in step: every lane holds the same offset (the loaded name, type and count are made wave-uniform with readfirstlane, so the walk's state lives in
// scalar registers), the NUL of a Z / H string is found 64 bytes at a time with a ballot, and so are the '#' and '!' of the read name.  Every copy
// (the bytes before the aux data, each run of kept aux entries, each appended value) is made by the 64 lanes over consecutive bytes: byte j of a
// span goes to lane j mod 64, so a wave's loads and stores are 64 consecutive bytes.
// Why not a lane per record staged through LDS (bam_parse_kernel's shape): that shape is right where a record is READ -- ~150 single-byte loads per
// lane, which LDS turns from 64 transactions into one -- but here every record is also WRITTEN, 270 bytes to 10 KB of it, to an offset of its own:
// a lane per record would store its record byte by byte to addresses 270 bytes apart from its neighbours' (64 transactions per store, the very thing
// the stage was built to avoid on the load side), would need a second stage for the output, and a record beyond the 20 KB stage (10 000 bases)
// would fall back to memory on both sides.  A wave per record (bam_gather_records_kernel's shape) has no size limit, coalesces both sides, and
// its serial part -- the walk, ~15 entries -- costs a wave a few hundred cycles that other waves of the CU hide.  Byte work, bound by memory; no MFMA.
// Measured: plan + scan + emit 59 ms for 16 M records of ~310 bytes, 159 GB/s read + written = 2 % of the HBM peak -- the walk's
// dependent loads, not the copies, are the supposed bound; under -b both kernels together are 2-5 % of the ingest, the compressor 60-70 %.
//
// bam_tag_plan and bam_tag_emit run the SAME function (bamtag_record) once without and once with a destination: the spans the plan finds live in
// registers and are found again by the emit from bytes that are still in L2, instead of ~100 bytes of spans per record going through memory (a record
// may drop any number of entries -- a repeated CR -- so a stored plan would need a bound that the rule does not have).
//
// The filtered mode (-F: FilteringBamProcessor::write_alignment, FilteringBamProcessor.cpp:61-96) is the same function with FILT = true: a record is
// written only when the container's verdict for it is 0, and two more tags follow the read type -- the corrected cell barcode and the corrected UMI.
// The decisions are indexed by the window's ACCEPTED records, so record r takes entry rank[r] = accepted records before r (bam_tag_rank_*: a tile
// count, a scan of the tiles by one workgroup, a scan inside the tile -- the shape of the size scan below, on the device: no status goes to the
// host).  The two values exist nowhere as bytes: a plain 2-bit code is spelled by the lanes (base j by lane j, at most 31 of them), an escaped
// one is a side string copied 64 bytes a step like every other span.  The shape stays for the same reason: the decision costs a wave five
// wave-uniform loads (rank, verdict, cell, the cell's code, the UMI code) in front of a walk of ~15 entries, and a record that is not written
// costs nothing else.  Everything a decision points at is checked before it is
// loaded: a cell id or a side-string index out of range sets BAMTAG_FLAG_RANGE and the record gets size 0.
// Where the decisions stand is a template parameter of the decision (SRC, as read_corrections_kernel takes its look-up): BamTagOneArray, entry
// rank[r] of one array -- one context's -- or BamTagSegments, a table of segments in device memory, one per shard of a sharded run whose resident
// range meets the window; the segment of a rank is found by a ballot over 64 table entries a step, wave-uniform like everything else here.
// Measured: rank + plan + scan + emit 64.5 ms for 16 M records of which 13.7 M are written (-b in the same job: 59.1 ms for all 16 M);
// 3-9 % of the -F pass, of which the compressor is 71-81 %.
//
// The sources beside the record (-r, -P: BAM_SRC_*, k_bamparse.h) are one more template parameter of bamtag_record and bamtag_inputs (SRCS) and
// kernels of their own on top of them (bam_tag_sources_plan / _emit): with -r the raw barcode, the raw UMI and the UMI quality are three extents of
// the read-parameter table's text -- the row the settle served the record (BamSources::rp_row), loaded wave-uniformly like everything else the walk
// decides by -- and no barcode quality is written (ReadParametersEfficient::parameters answers "" for it); with -P the gene is the name of the
// record's reference and the mark what the parse left in o_aux.  Which of the two is on is a wave-uniform test of BamTagSrc::bits, not a template
// parameter: one instantiation per decision source, not four.  The kernels without sources are untouched: SRCS = false compiles to what they were.
#pragma once

#include "k_bamparse.h"

namespace dropest {

struct BamTagCfg {
	uint16_t out_tag[5];          // gene, raw barcode, raw UMI, barcode quality, UMI quality: the order they are appended in
	uint16_t type_tag;            // read type, 0 = none is written
	uint32_t type_len[3];         // out-values by mark: exonic (2), intronic (4), intergenic (1)
	uint8_t type_val[3][24];
};
// -g: the annotation's gene names by its gene index (name g = pool[off[g] .. off[g + 1])), null without -g
struct BamTagNames { const uint32_t *off; const uint8_t *pool; uint32_t n; };
struct BamTagIn {
	const uint8_t *data; const uint64_t *rec_off; const uint8_t *status; const uint32_t *o_aux; uint32_t n_rec;
	const uint32_t *a_gene; const int32_t *a_mark;      // -g (null without): the annotation's gene and verdict per record
};

constexpr uint32_t BAMTAG_T = 256, BAMTAG_WAVES = BAMTAG_T / 64;
constexpr uint32_t BAMTAG_SCAN_PER = 16, BAMTAG_SCAN_TILE = 256 * BAMTAG_SCAN_PER;      // the scans below: records per lane, per workgroup
// -g left the record's gene to the host; plan and emit disagree (internal); -F: a decision names a cell or a side string that does not exist
enum : uint32_t { BAMTAG_FLAG_UNDECIDED = 1u, BAMTAG_FLAG_SIZE = 2u, BAMTAG_FLAG_RANGE = 4u };

// -F: the decisions of the window's accepted records (entry rank[r] belongs to record r) and what they point at
struct BamTagFilt {
	const uint32_t *rank;                                                 // per record of the window: accepted records before it
	const uint8_t *verdict; const uint32_t *cell; const uint64_t *umi; uint32_t n;      // per accepted record: 0 = written, target cell, corrected UMI (a code)
	const uint64_t *cell_barcode; uint32_t n_cells;             // every cell's barcode as a code
	const uint32_t *side_off; const uint8_t *side_pool; uint32_t n_side;  // the strings of escaped codes: string k = pool[off[k] .. off[k + 1])
	uint32_t out_tag[2];                                                  // corrected barcode, corrected UMI (0 = never written)
};
// -F, decisions in segments (a sharded run: read i's decision lives in the arrays of the shard whose resident range holds ordinal i, and a window
// crosses up to one boundary per shard): segment s holds the decisions of the accepted ranks [first, first + count) of the window, entry
// k - first of its arrays.  `first` ascends (it is the sum of the counts before), a count of 0 is legal anywhere.  The table lives in device
// memory (64 entries would be 2 KB of kernel arguments); the arrays belong to the decoder's GPU.
struct BamTagSeg { uint32_t first, count; const uint8_t *verdict; const uint32_t *cell; const uint64_t *umi; };
static_assert(sizeof(BamTagSeg) == 32, "one table entry is 32 bytes");
// where the decision of accepted rank k stands (all three wave-uniform)
struct BamTagEntry { const uint8_t *verdict; const uint32_t *cell; const uint64_t *umi; };
// a value of -F as the record function takes it: len characters, of a side string (str) or spelled from a plain code
struct BamTagValue { const uint8_t *str; unsigned long long code; uint32_t len; };
struct BamTagFix { uint32_t name[2]; BamTagValue v[2]; };

__device__ inline uint32_t bt_u(uint32_t v) { return uint32_t(__builtin_amdgcn_readfirstlane(int(v))); }
__device__ inline unsigned long long bt_u64(unsigned long long v) { return (unsigned long long)bt_u(uint32_t(v)) | ((unsigned long long)bt_u(uint32_t(v >> 32)) << 32); }

// -r / -P (SRCS): where a record's strings come from when not from the record.  bits: BAM_SRC_*.  -r: rp_row[r] = the row of `rows` that record r was
// served (bam_params_settle_kernel), whose extents lie in text[0 .. text_len); -P: reference k's name = refs.pool[refs.off[k] .. refs.off[k + 1])
struct BamTagSrc {
	int bits;
	const uint32_t *rp_row; const RpRow *rows; const uint8_t *text; uint32_t n_rows; unsigned long long text_len;
	BamTagNames refs;
};
// the served row's raw barcode, raw UMI and UMI quality (on: the record's own name and tags are not asked for them)
struct BamTagRowStrings { const uint8_t *s[3]; uint32_t len[3]; bool on; };

// One aux entry whose name starts at tags + o (o + 3 <= n): name, type and the length of its value (which starts at o + 3).  false: the walk stops
// here -- an unknown type, a string without its NUL, a value past the record's end (BamRecord::get_string_tags; tests/bam_model.py: string_tags).
__device__ inline bool bamtag_entry(const uint8_t *tags, uint32_t n, uint32_t o, uint32_t lane, uint32_t &name, uint32_t &type, uint32_t &len, bool &text) {
	name = bt_u(uint32_t(tags[o]) | (uint32_t(tags[o + 1]) << 8));
	type = bt_u(tags[o + 2]);
	const uint32_t v = o + 3;
	text = false;
	switch (type) {
		case 'A': case 'c': case 'C': len = 1; break;
		case 's': case 'S': len = 2; break;
		case 'i': case 'I': case 'f': len = 4; break;
		case 'Z': case 'H': {
			uint32_t e = v;
			for (;;) {                                     // the NUL, 64 bytes a step
				if (e >= n) return false;
				const uint32_t j = e + lane;
				const uint64_t m = __ballot(j < n && tags[j] == 0);
				if (m) { e += uint32_t(__ffsll((long long)m) - 1); break; }
				e += 64;
			}
			len = e - v + 1; text = true; break;
		}
		case 'B': {
			if (uint64_t(v) + 5u > n) return false;
			const uint32_t sub = bt_u(tags[v]);
			const uint32_t cnt = bt_u(uint32_t(tags[v + 1]) | (uint32_t(tags[v + 2]) << 8) | (uint32_t(tags[v + 3]) << 16) | (uint32_t(tags[v + 4]) << 24));
			const uint32_t w = (sub == 'c' || sub == 'C') ? 1u : ((sub == 's' || sub == 'S') ? 2u : 4u);
			const uint64_t l64 = 5ull + uint64_t(cnt) * w;
			if (l64 > n) return false;
			len = uint32_t(l64); break;
		}
		default: return false;
	}
	return uint64_t(v) + len <= n;
}

// where the record's output stands: `at` bytes of `cap` are written so far; EMIT = false only counts
template <bool EMIT> struct BamTagOut {
	uint8_t *dst; uint32_t at, cap; bool over;
	__device__ void copy(const uint8_t *src, uint32_t n, uint32_t lane) {
		if (EMIT) {
			if (uint64_t(at) + n > cap) { over = true; return; }      // (never, while plan and emit run the same code: nothing is written past the record's room)
			for (uint32_t j = lane; j < n; j += 64) dst[at + j] = src[j];
		}
		at += n;
	}
	// name, 'Z', the value, NUL
	__device__ void tag(uint32_t name, const uint8_t *src, uint32_t n, uint32_t lane) {
		if (EMIT) {
			if (uint64_t(at) + n + 4u > cap) { over = true; return; }
			for (uint32_t j = lane; j < n + 4u; j += 64) dst[at + j] = j == 0 ? uint8_t(name) : j == 1 ? uint8_t(name >> 8) : j == 2 ? uint8_t('Z') : j < n + 3u ? src[j - 3u] : uint8_t(0);
		}
		at += n + 4u;
	}
	// -F: name, 'Z', a value spelled from its 2-bit code (base j, the first most significant, by lane j) or copied from its side string, NUL
	__device__ void value(uint32_t name, const BamTagValue &v, uint32_t lane) {
		const uint32_t n = v.len;
		if (EMIT) {
			if (uint64_t(at) + n + 4u > cap) { over = true; return; }
			for (uint32_t j = lane; j < n + 4u; j += 64) {
				uint8_t c = 0;
				if (j == 0) c = uint8_t(name);
				else if (j == 1) c = uint8_t(name >> 8);
				else if (j == 2) c = uint8_t('Z');
				else if (j < n + 3u) c = v.str ? v.str[j - 3u] : uint8_t(0x54474341u >> (8u * (uint32_t(v.code >> (2u * (n + 2u - j))) & 3u)));      // "ACGT"
				dst[at + j] = c;
			}
		}
		at += n + 4u;
	}
};

// Record `rec` (its block_size field first, accepted by bam_parse) -> the bytes of its output (block_size field included), counted or written.
// FILT (-F): the two values of `fx` follow the read type, under the same rule (a value of no character is not written and drops nothing).
// SRCS with rs.on (-r): raw barcode, raw UMI and UMI quality are the row's; no barcode quality; the record's name and those four tags are not looked at.
template <bool EMIT, bool FILT = false, bool SRCS = false>
__device__ inline uint32_t bamtag_record(const uint8_t *rec, uint32_t lane, const BamParseCfg &pc, const BamTagCfg &tc, uint32_t mark, const uint8_t *gene_override, uint32_t gene_override_len,
                                         bool use_override, uint8_t *dst, uint32_t cap, bool &over, const BamTagFix &fx = BamTagFix{}, const BamTagRowStrings &rs = BamTagRowStrings{}) {
	const uint32_t block_size = bt_u(b_le32(rec));
	const uint8_t *p = rec + 4;
	const uint32_t l_read_name = bt_u(p[8]), n_cigar = bt_u(b_le16(p + 12)), l_seq = bt_u(b_le32(p + 16));
	const uint32_t aux = uint32_t(32ull + l_read_name + 4ull * n_cigar + (uint64_t(l_seq) + 1) / 2 + l_seq);   // (<= block_size: bam_parse accepted the record)
	const uint8_t *tags = p + aux;
	const uint32_t tags_size = block_size - aux;
	enum { T_CB, T_UMI, T_CBQ, T_UMIQ, T_GENE, T_TYPE };
	// 1. the values of the wanted tags, as bam_parse found them: the first text occurrence, unless a numeric one came before it
	const uint8_t *val[6]; uint32_t vlen[6]; bool found[6], closed[6];
#pragma unroll
	for (int k = 0; k < 6; ++k) { found[k] = false; closed[k] = false; val[k] = nullptr; vlen[k] = 0; }
	uint32_t o = 0;
	while (uint64_t(o) + 3u <= tags_size) {
		uint32_t name, type, len; bool text;
		if (!bamtag_entry(tags, tags_size, o, lane, name, type, len, text)) break;
#pragma unroll
		for (int k = 0; k < 6; ++k) {
			if (SRCS && rs.on && k < 4) continue;
			if (pc.tag[k] != name || !pc.tag[k] || found[k] || closed[k]) continue;
			if (text) { val[k] = tags + o + 3; vlen[k] = len - 1; found[k] = true; }
			else if (type == 'A') { val[k] = tags + o + 3; vlen[k] = 1; found[k] = true; }
			else closed[k] = true;
		}
		o += 3u + len;
	}
	const uint32_t walk_end = o;      // entries start in [0, walk_end); the bytes from there on were not reached
	// 2. the strings to write: gene, raw barcode, raw UMI, barcode quality, UMI quality (+ the read type)
	const uint8_t *src[5]; uint32_t sl[5];
#pragma unroll
	for (int k = 0; k < 5; ++k) { src[k] = nullptr; sl[k] = 0; }
	if (SRCS && rs.on) {
		src[1] = rs.s[0]; sl[1] = rs.len[0]; src[2] = rs.s[1]; sl[2] = rs.len[1]; src[4] = rs.s[2]; sl[4] = rs.len[2];
	} else if (pc.filled_bam) {
		src[1] = val[T_CB]; sl[1] = vlen[T_CB]; src[2] = val[T_UMI]; sl[2] = vlen[T_UMI];
		if (found[T_CBQ]) { src[3] = val[T_CBQ]; sl[3] = vlen[T_CBQ]; }
		if (found[T_UMIQ]) { src[4] = val[T_UMIQ]; sl[4] = vlen[T_UMIQ]; }
	} else {                                                  // "id!CB#UMI": rfind('#'), then rfind('!') at or before it, 64 bytes a step from the end
		const uint8_t *name = p + 32;
		const uint32_t nl = l_read_name ? l_read_name - 1 : 0;
		int32_t up = -1, cp = -1;
		for (int32_t base = int32_t((nl + 63u) / 64u) * 64 - 64; base >= 0 && up < 0; base -= 64) {
			const uint32_t j = uint32_t(base) + lane;
			const uint64_t m = __ballot(j < nl && name[j] == '#');
			if (m) up = base + 63 - __clzll((long long)m);
		}
		for (int32_t base = up >= 0 ? (up / 64) * 64 : -1; base >= 0 && cp < 0; base -= 64) {
			const uint32_t j = uint32_t(base) + lane;
			const uint64_t m = __ballot(int32_t(j) <= up && name[j] == '!');
			if (m) cp = base + 63 - __clzll((long long)m);
		}
		if (up >= 0 && cp >= 0) { src[1] = name + cp + 1; sl[1] = uint32_t(up - cp - 1); src[2] = name + up + 1; sl[2] = nl - uint32_t(up) - 1; }   // (always: bam_parse accepted the record)
	}
	if (use_override) { src[0] = gene_override; sl[0] = gene_override_len; }
	else if (found[T_GENE]) { src[0] = val[T_GENE]; sl[0] = vlen[T_GENE]; }
	const int type_k = mark == 2u ? 0 : mark == 4u ? 1 : mark == 1u ? 2 : -1;      // exactly exonic / intronic / intergenic; a spanning mark writes none
	constexpr int NT = FILT ? 8 : 6;
	bool on[NT];
	on[0] = sl[0] != 0; on[1] = true; on[2] = true; on[3] = sl[3] != 0; on[4] = sl[4] != 0; on[5] = type_k >= 0;
	uint32_t ename[NT];
#pragma unroll
	for (int k = 0; k < 5; ++k) ename[k] = tc.out_tag[k];
	ename[5] = tc.type_tag;
	if (FILT) { on[NT - 2] = fx.v[0].len != 0; on[NT - 1] = fx.v[1].len != 0; ename[NT - 2] = fx.name[0]; ename[NT - 1] = fx.name[1]; }
#pragma unroll
	for (int k = 0; k < NT; ++k) on[k] = on[k] && ename[k] != 0u;      // a tag without a name is never written (and drops nothing)
	// 3. the output: block_size, the bytes before the aux data, the runs of kept entries, the bytes the walk did not reach, the new tags
	BamTagOut<EMIT> out{dst, 4u, cap, false};
	out.copy(p, aux, lane);
	uint32_t run = 0;
	o = 0;
	while (o < walk_end) {
		uint32_t name, type, len; bool text;
		if (!bamtag_entry(tags, tags_size, o, lane, name, type, len, text)) break;      // (never before walk_end: the same walk)
		bool drop = false;
#pragma unroll
		for (int k = 0; k < NT; ++k) drop |= on[k] && ename[k] == name;
		if (drop) { out.copy(tags + run, o - run, lane); run = o + 3u + len; }
		o += 3u + len;
	}
	out.copy(tags + run, tags_size - run, lane);
#pragma unroll
	for (int k = 0; k < 5; ++k) if (on[k]) out.tag(ename[k], src[k], sl[k], lane);
	if (on[5]) out.tag(ename[5], tc.type_val[type_k], tc.type_len[type_k], lane);
	if (FILT) {
		if (on[NT - 2]) out.value(ename[NT - 2], fx.v[0], lane);
		if (on[NT - 1]) out.value(ename[NT - 1], fx.v[1], lane);
	}
	if (EMIT) {
		const uint32_t new_block = out.at - 4u;
		if (lane < 4u && cap >= 4u) dst[lane] = uint8_t(new_block >> (8u * lane));
		over = out.over || out.at != cap;
	}
	return out.at;
}

// the record's gene under -g and its mark; false: not an accepted record
// SRCS: -P, the gene is the name of the record's reference (the mark is o_aux's already); -r, the served row's three strings into `rs`.  Everything is
// checked before it is loaded (as bamtag_decision does): a reference or a row outside its table, an extent past the text -> BAMTAG_FLAG_RANGE, false
template <bool SRCS = false>
__device__ inline bool bamtag_inputs(const BamTagIn &in, const BamTagNames &names, uint32_t r, uint32_t &mark, const uint8_t *&g, uint32_t &g_len, bool &use_override, uint32_t *flags, uint32_t lane,
                                     const BamTagSrc *ts = nullptr, BamTagRowStrings *rs = nullptr) {
	if (bt_u(in.status[r]) != BAM_OK) return false;
	mark = bt_u(in.o_aux[r] >> 16);
	g = nullptr; g_len = 0; use_override = names.off != nullptr;
	if (use_override) {
		if (bt_u(uint32_t(in.a_mark[r])) == uint32_t(-2)) { if (lane == 0) atomicOr(flags, BAMTAG_FLAG_UNDECIDED); }      // more genes at an end point than annotate_reads holds: the host decided, the device cannot name the gene
		const uint32_t ag = bt_u(in.a_gene[r]);
		if (ag < names.n) { const uint32_t a = bt_u(names.off[ag]); g = names.pool + a; g_len = bt_u(names.off[ag + 1]) - a; }
	}
	if (SRCS) {
		bool ok = true;
		rs->on = false;
		if (ts->bits & BAM_SRC_REF_GENE) {
			const uint32_t ref = bt_u(b_le32(in.data + in.rec_off[r] + 4));
			use_override = true; g = nullptr; g_len = 0;
			if (ref < ts->refs.n) { const uint32_t a = bt_u(ts->refs.off[ref]), b = bt_u(ts->refs.off[ref + 1]); g = ts->refs.pool + a; g_len = b > a ? b - a : 0u; }
			else ok = false;
		}
		if (ts->bits & BAM_SRC_PARAMS) {
			const uint32_t row = bt_u(ts->rp_row[r]);
			if (row < ts->n_rows) {
				const RpRow &w = ts->rows[row];
				const unsigned long long off[3] = {bt_u64(w.cb_off), bt_u64(w.umi_off), bt_u64(w.quality_off)};
				rs->len[0] = bt_u(w.cb_len); rs->len[1] = bt_u(w.umi_len); rs->len[2] = bt_u(w.quality_len);
#pragma unroll
				for (int k = 0; k < 3; ++k) { ok = ok && off[k] <= ts->text_len && rs->len[k] <= ts->text_len - off[k]; rs->s[k] = ts->text + off[k]; }
				rs->on = true;
			} else ok = false;
		}
		if (!ok) { if (lane == 0) atomicOr(flags, BAMTAG_FLAG_RANGE); return false; }
	}
	return true;
}

// -g: what the host decided for records the annotation query left to it (a_mark == -2: more transcripts at an end point than the kernel holds) --
// the annotation's gene (~0: none) and the mark of records rec[0 .. n), written where the tag kernels read them
__global__ __launch_bounds__(256) void bam_tag_patch_annotation_kernel(const uint32_t *rec, const uint32_t *gene, const uint32_t *mark, uint32_t n, uint32_t *__restrict__ a_gene,
                                                                       int32_t *__restrict__ a_mark, uint32_t *__restrict__ o_aux) {
	const uint32_t k = blockIdx.x * 256 + threadIdx.x;
	if (k >= n) return;
	const uint32_t r = rec[k];
	a_gene[r] = gene[k]; a_mark[r] = int32_t(mark[k] & 7u); o_aux[r] = (o_aux[r] & 0xFFFFu) | ((mark[k] & 7u) << 16);
}

// size[r] = bytes of record r's output (0: not written)
__global__ __launch_bounds__(BAMTAG_T) void bam_tag_plan_kernel(BamTagIn in, BamParseCfg pc, BamTagCfg tc, BamTagNames names, uint32_t *__restrict__ size, uint32_t *__restrict__ flags) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t r = bt_u(blockIdx.x * BAMTAG_WAVES + (threadIdx.x >> 6));
	if (r >= in.n_rec) return;
	uint32_t mark, g_len; const uint8_t *g; bool use_override, over = false;
	uint32_t bytes = 0;
	if (bamtag_inputs(in, names, r, mark, g, g_len, use_override, flags, lane))
		bytes = bamtag_record<false>(in.data + in.rec_off[r], lane, pc, tc, mark, g, g_len, use_override, nullptr, 0u, over);
	if (lane == 0) size[r] = bytes;
}

// the output of record r to out + out_off[r], size[r] bytes of it
__global__ __launch_bounds__(BAMTAG_T) void bam_tag_emit_kernel(BamTagIn in, BamParseCfg pc, BamTagCfg tc, BamTagNames names, const uint32_t *__restrict__ size, const uint64_t *__restrict__ out_off,
                                                                 uint8_t *__restrict__ out, uint64_t out_total, uint32_t *__restrict__ flags) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t r = bt_u(blockIdx.x * BAMTAG_WAVES + (threadIdx.x >> 6));
	if (r >= in.n_rec) return;
	const uint32_t cap = bt_u(size[r]);
	if (!cap) return;
	const uint64_t at = out_off[r];
	if (at + cap > out_total) { if (lane == 0) atomicOr(flags, BAMTAG_FLAG_SIZE); return; }
	uint32_t mark, g_len; const uint8_t *g; bool use_override, over = false;
	if (!bamtag_inputs(in, names, r, mark, g, g_len, use_override, flags, lane)) return;
	bamtag_record<true>(in.data + in.rec_off[r], lane, pc, tc, mark, g, g_len, use_override, out + at, cap, over);
	if (over && lane == 0) atomicOr(flags, BAMTAG_FLAG_SIZE);
}

// ---- -F: a record's decision ------------------------------------------------------------------------------------------------------------
// a code -> the value to write; false: an escaped code whose side string does not exist (nothing of it is loaded)
__device__ inline bool bamtag_value(unsigned long long code, const BamTagFilt &f, BamTagValue &v) {
	v.str = nullptr; v.code = code; v.len = 0;
	if (code >> 63) {
		const unsigned long long k = code & 0x7FFFFFFFFFFFFFFFull;
		if (k >= f.n_side) return false;
		const uint32_t a = bt_u(f.side_off[k]), b = bt_u(f.side_off[k + 1]);
		v.str = f.side_pool + a; v.len = b > a ? b - a : 0u;
	} else if (code)
		v.len = uint32_t(63 - __clzll((long long)code)) / 2u;      // the sentinel bit says how many bases follow it
	return true;
}

// The two sources of a decision (bamtag_decision's SRC, as read_corrections_kernel takes its look-up): entry(f, k, lane, e) = where rank k's
// decision stands; false: no decision covers k (nothing is loaded from there).
// BamTagOneArray: entry k of BamTagFilt's own arrays -- no load, no branch.
struct BamTagOneArray {
	__device__ bool entry(const BamTagFilt &f, uint32_t k, uint32_t, BamTagEntry &e) const {
		e.verdict = f.verdict + k; e.cell = f.cell + k; e.umi = f.umi + k;
		return k < f.n;                                                // (always: the caller checked the window's accepted count)
	}
};
// BamTagSegments: the segment that covers k, by wave-uniform work alone -- 64 entries of the table a step, one per lane, and a ballot over
// first <= k < first + count (at most one lane answers: the segments do not overlap; an empty one never does); the table ascends, so the
// search ends at the first step that holds an entry beginning behind k.  Then the entry's three pointers, loaded by the whole wave from one address.
// A window of a sharded run has one segment per shard: one step, one 8-byte load per lane and three uniform ones more than the one array.
struct BamTagSegments {
	const BamTagSeg *seg; uint32_t n_seg;
	__device__ bool entry(const BamTagFilt &, uint32_t k, uint32_t lane, BamTagEntry &e) const {
		for (uint32_t base = 0; base < n_seg; base += 64u) {
			const uint32_t s = base + lane;
			uint32_t first = 0xFFFFFFFFu, count = 0;
			if (s < n_seg) { first = seg[s].first; count = seg[s].count; }
			const uint64_t hit = __ballot(first <= k && k - first < count);
			if (hit) {
				const BamTagSeg &g = seg[base + uint32_t(__ffsll((long long)hit) - 1)];
				const uint32_t j = k - bt_u(g.first);
				e.verdict = reinterpret_cast<const uint8_t *>(bt_u64(reinterpret_cast<unsigned long long>(g.verdict))) + j;
				e.cell = reinterpret_cast<const uint32_t *>(bt_u64(reinterpret_cast<unsigned long long>(g.cell))) + j;
				e.umi = reinterpret_cast<const uint64_t *>(bt_u64(reinterpret_cast<unsigned long long>(g.umi))) + j;
				return true;
			}
			if (__ballot(s < n_seg && first > k)) break;
		}
		return false;
	}
};

// Record r of the window: false = not written (not accepted, or a verdict that is not 0, or a decision that points outside its tables, or no
// decision at all: flagged)
template <class SRC>
__device__ inline bool bamtag_decision(const BamTagIn &in, const BamTagFilt &f, const SRC &src, uint32_t r, BamTagFix &fx, uint32_t *flags, uint32_t lane) {
	if (bt_u(in.status[r]) != BAM_OK) return false;
	const uint32_t k = bt_u(f.rank[r]);
	BamTagEntry e;
	bool ok = src.entry(f, k, lane, e);
	if (ok && bt_u(*e.verdict) != 0u) return false;
	uint32_t cell = 0;
	if (ok) { cell = bt_u(*e.cell); ok = cell < f.n_cells; }
	if (ok) ok = bamtag_value(bt_u64(f.cell_barcode[cell]), f, fx.v[0]);
	if (ok) ok = bamtag_value(bt_u64(*e.umi), f, fx.v[1]);
	if (!ok) { if (lane == 0) atomicOr(flags, BAMTAG_FLAG_RANGE); return false; }
	fx.name[0] = f.out_tag[0]; fx.name[1] = f.out_tag[1];
	return true;
}

// bam_tag_plan_kernel / bam_tag_emit_kernel for -F; SRC: BamTagOneArray (one context) or BamTagSegments (the shards of a sharded run), the last
// argument so that no other one moves
template <class SRC>
__global__ __launch_bounds__(BAMTAG_T) void bam_tag_filter_plan_kernel(BamTagIn in, BamParseCfg pc, BamTagCfg tc, BamTagNames names, BamTagFilt filt, uint32_t *__restrict__ size,
                                                                        uint32_t *__restrict__ flags, SRC src) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t r = bt_u(blockIdx.x * BAMTAG_WAVES + (threadIdx.x >> 6));
	if (r >= in.n_rec) return;
	uint32_t mark, g_len; const uint8_t *g; bool use_override, over = false;
	uint32_t bytes = 0;
	BamTagFix fx;
	if (bamtag_decision(in, filt, src, r, fx, flags, lane) && bamtag_inputs(in, names, r, mark, g, g_len, use_override, flags, lane))
		bytes = bamtag_record<false, true>(in.data + in.rec_off[r], lane, pc, tc, mark, g, g_len, use_override, nullptr, 0u, over, fx);
	if (lane == 0) size[r] = bytes;
}

template <class SRC>
__global__ __launch_bounds__(BAMTAG_T) void bam_tag_filter_emit_kernel(BamTagIn in, BamParseCfg pc, BamTagCfg tc, BamTagNames names, BamTagFilt filt, const uint32_t *__restrict__ size,
                                                                        const uint64_t *__restrict__ out_off, uint8_t *__restrict__ out, uint64_t out_total, uint32_t *__restrict__ flags, SRC src) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t r = bt_u(blockIdx.x * BAMTAG_WAVES + (threadIdx.x >> 6));
	if (r >= in.n_rec) return;
	const uint32_t cap = bt_u(size[r]);
	if (!cap) return;
	const uint64_t at = out_off[r];
	if (at + cap > out_total) { if (lane == 0) atomicOr(flags, BAMTAG_FLAG_SIZE); return; }
	uint32_t mark, g_len; const uint8_t *g; bool use_override, over = false;
	BamTagFix fx;
	if (!bamtag_decision(in, filt, src, r, fx, flags, lane) || !bamtag_inputs(in, names, r, mark, g, g_len, use_override, flags, lane)) return;
	bamtag_record<true, true>(in.data + in.rec_off[r], lane, pc, tc, mark, g, g_len, use_override, out + at, cap, over, fx);
	if (over && lane == 0) atomicOr(flags, BAMTAG_FLAG_SIZE);
}

// ---- -r / -P: the four kernels above with the sources (SRCS) -----------------------------------------------------------------------------------
// FILT = false: bam_tag_plan / _emit (filt and src are not looked at: BamTagFilt{}, BamTagOneArray{}); FILT = true: bam_tag_filter_plan / _emit<SRC>.
template <bool FILT, class SRC>
__global__ __launch_bounds__(BAMTAG_T) void bam_tag_sources_plan_kernel(BamTagIn in, BamParseCfg pc, BamTagCfg tc, BamTagNames names, BamTagFilt filt, uint32_t *__restrict__ size,
                                                                         uint32_t *__restrict__ flags, SRC src, BamTagSrc ts) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t r = bt_u(blockIdx.x * BAMTAG_WAVES + (threadIdx.x >> 6));
	if (r >= in.n_rec) return;
	uint32_t mark, g_len; const uint8_t *g; bool use_override, over = false;
	uint32_t bytes = 0;
	BamTagFix fx{};
	BamTagRowStrings rs;
	if ((!FILT || bamtag_decision(in, filt, src, r, fx, flags, lane)) && bamtag_inputs<true>(in, names, r, mark, g, g_len, use_override, flags, lane, &ts, &rs))
		bytes = bamtag_record<false, FILT, true>(in.data + in.rec_off[r], lane, pc, tc, mark, g, g_len, use_override, nullptr, 0u, over, fx, rs);
	if (lane == 0) size[r] = bytes;
}

template <bool FILT, class SRC>
__global__ __launch_bounds__(BAMTAG_T) void bam_tag_sources_emit_kernel(BamTagIn in, BamParseCfg pc, BamTagCfg tc, BamTagNames names, BamTagFilt filt, const uint32_t *__restrict__ size,
                                                                         const uint64_t *__restrict__ out_off, uint8_t *__restrict__ out, uint64_t out_total, uint32_t *__restrict__ flags, SRC src,
                                                                         BamTagSrc ts) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t r = bt_u(blockIdx.x * BAMTAG_WAVES + (threadIdx.x >> 6));
	if (r >= in.n_rec) return;
	const uint32_t cap = bt_u(size[r]);
	if (!cap) return;
	const uint64_t at = out_off[r];
	if (at + cap > out_total) { if (lane == 0) atomicOr(flags, BAMTAG_FLAG_SIZE); return; }
	uint32_t mark, g_len; const uint8_t *g; bool use_override, over = false;
	BamTagFix fx{};
	BamTagRowStrings rs;
	if ((FILT && !bamtag_decision(in, filt, src, r, fx, flags, lane)) || !bamtag_inputs<true>(in, names, r, mark, g, g_len, use_override, flags, lane, &ts, &rs)) return;
	bamtag_record<true, FILT, true>(in.data + in.rec_off[r], lane, pc, tc, mark, g, g_len, use_override, out + at, cap, over, fx, rs);
	if (over && lane == 0) atomicOr(flags, BAMTAG_FLAG_SIZE);
}

// ---- -F: rank[r] = accepted records of the window before r, in the three steps of the size scan below ---------------------------------------
// tile_ok[t] = accepted records in tile t of 4 096 records
__global__ __launch_bounds__(256) void bam_tag_rank_tile_kernel(const uint8_t *__restrict__ status, uint32_t n, uint32_t *__restrict__ tile_ok) {
	__shared__ uint32_t s_ok;
	if (threadIdx.x == 0) s_ok = 0;
	__syncthreads();
	const uint32_t first = blockIdx.x * BAMTAG_SCAN_TILE + threadIdx.x * BAMTAG_SCAN_PER;
	uint32_t ok = 0;
	for (uint32_t j = 0; j < BAMTAG_SCAN_PER && first + j < n; ++j) ok += status[first + j] == BAM_OK ? 1u : 0u;
	if (ok) atomicAdd(&s_ok, ok);
	__syncthreads();
	if (threadIdx.x == 0) tile_ok[blockIdx.x] = s_ok;
}

// exclusive scan of the tiles' counts by ONE workgroup; total[0] = the window's accepted records
__global__ __launch_bounds__(1024) void bam_tag_rank_scan_kernel(uint32_t *__restrict__ tile_ok, uint32_t n, uint32_t *__restrict__ total) {
	__shared__ uint32_t sa[1024];
	__shared__ uint32_t carry;
	if (threadIdx.x == 0) carry = 0;
	__syncthreads();
	for (uint32_t base = 0; base < n; base += 1024) {
		const uint32_t i = base + threadIdx.x;
		const uint32_t va = i < n ? tile_ok[i] : 0u;
		sa[threadIdx.x] = va;
		__syncthreads();
		for (uint32_t dd = 1; dd < 1024; dd <<= 1) {
			const uint32_t xa = threadIdx.x >= dd ? sa[threadIdx.x - dd] : 0u;
			__syncthreads();
			sa[threadIdx.x] += xa;
			__syncthreads();
		}
		if (i < n) tile_ok[i] = carry + sa[threadIdx.x] - va;
		__syncthreads();
		if (threadIdx.x == 1023) carry += sa[1023];
		__syncthreads();
	}
	if (threadIdx.x == 0) total[0] = carry;
}

// rank[r] = the tile's base + the accepted records of the tile before r
__global__ __launch_bounds__(256) void bam_tag_rank_kernel(const uint8_t *__restrict__ status, uint32_t n, const uint32_t *__restrict__ tile_base, uint32_t *__restrict__ rank) {
	__shared__ uint32_t s[256];
	const uint32_t first = blockIdx.x * BAMTAG_SCAN_TILE + threadIdx.x * BAMTAG_SCAN_PER;
	uint32_t mine = 0;
	for (uint32_t j = 0; j < BAMTAG_SCAN_PER && first + j < n; ++j) mine += status[first + j] == BAM_OK ? 1u : 0u;
	s[threadIdx.x] = mine;
	__syncthreads();
	for (uint32_t dd = 1; dd < 256; dd <<= 1) {
		const uint32_t x = threadIdx.x >= dd ? s[threadIdx.x - dd] : 0u;
		__syncthreads();
		s[threadIdx.x] += x;
		__syncthreads();
	}
	uint32_t at = tile_base[blockIdx.x] + s[threadIdx.x] - mine;
	for (uint32_t j = 0; j < BAMTAG_SCAN_PER && first + j < n; ++j) { rank[first + j] = at; at += status[first + j] == BAM_OK ? 1u : 0u; }
}

// ---- the exclusive scan over the sizes: 64-bit offsets, as rec_off ----------------------------------------------------------------------
// bytes and records written per tile of 4 096 records
__global__ __launch_bounds__(256) void bam_tag_tile_sum_kernel(const uint32_t *__restrict__ size, uint32_t n, unsigned long long *__restrict__ tile_bytes, uint32_t *__restrict__ tile_written) {
	__shared__ unsigned long long s_bytes;
	__shared__ uint32_t s_written;
	if (threadIdx.x == 0) { s_bytes = 0; s_written = 0; }
	__syncthreads();
	const uint32_t first = blockIdx.x * BAMTAG_SCAN_TILE + threadIdx.x * BAMTAG_SCAN_PER;
	unsigned long long b = 0; uint32_t w = 0;
	for (uint32_t j = 0; j < BAMTAG_SCAN_PER && first + j < n; ++j) { const uint32_t s = size[first + j]; b += s; w += s ? 1u : 0u; }
	if (w) { atomicAdd(&s_bytes, b); atomicAdd(&s_written, w); }
	__syncthreads();
	if (threadIdx.x == 0) { tile_bytes[blockIdx.x] = s_bytes; tile_written[blockIdx.x] = s_written; }
}

// exclusive scan of the tiles' bytes by ONE workgroup (a window has a few thousand tiles); result[0] = all bytes, result[1] = records written,
// result[2] = the flags so far -- in pinned host memory, written by this kernel's stores
__global__ __launch_bounds__(1024) void bam_tag_tile_scan_kernel(unsigned long long *__restrict__ tile_bytes, const uint32_t *__restrict__ tile_written, uint32_t n, const uint32_t *__restrict__ flags,
                                                                  unsigned long long *result) {
	__shared__ unsigned long long sa[1024];
	__shared__ uint32_t sb[1024];
	__shared__ unsigned long long carry;
	__shared__ uint32_t written;
	if (threadIdx.x == 0) { carry = 0; written = 0; }
	__syncthreads();
	for (uint32_t base = 0; base < n; base += 1024) {
		const uint32_t i = base + threadIdx.x;
		const unsigned long long va = i < n ? tile_bytes[i] : 0ull;
		sa[threadIdx.x] = va; sb[threadIdx.x] = i < n ? tile_written[i] : 0u;
		__syncthreads();
		for (uint32_t dd = 1; dd < 1024; dd <<= 1) {
			const unsigned long long xa = threadIdx.x >= dd ? sa[threadIdx.x - dd] : 0ull;
			const uint32_t xb = threadIdx.x >= dd ? sb[threadIdx.x - dd] : 0u;
			__syncthreads();
			sa[threadIdx.x] += xa; sb[threadIdx.x] += xb;
			__syncthreads();
		}
		if (i < n) tile_bytes[i] = carry + sa[threadIdx.x] - va;
		__syncthreads();
		if (threadIdx.x == 1023) { carry += sa[1023]; written += sb[1023]; }
		__syncthreads();
	}
	if (threadIdx.x == 0) { result[0] = carry; result[1] = written; result[2] = flags[0]; }
}

// out_off[r] = the tile's base + the bytes of the tile's records before r
__global__ __launch_bounds__(256) void bam_tag_offsets_kernel(const uint32_t *__restrict__ size, uint32_t n, const unsigned long long *__restrict__ tile_base, uint64_t *__restrict__ out_off) {
	__shared__ unsigned long long s[256];
	const uint32_t first = blockIdx.x * BAMTAG_SCAN_TILE + threadIdx.x * BAMTAG_SCAN_PER;
	unsigned long long mine = 0;
	for (uint32_t j = 0; j < BAMTAG_SCAN_PER && first + j < n; ++j) mine += size[first + j];
	s[threadIdx.x] = mine;
	__syncthreads();
	for (uint32_t dd = 1; dd < 256; dd <<= 1) {
		const unsigned long long x = threadIdx.x >= dd ? s[threadIdx.x - dd] : 0ull;
		__syncthreads();
		s[threadIdx.x] += x;
		__syncthreads();
	}
	unsigned long long at = tile_base[blockIdx.x] + s[threadIdx.x] - mine;
	for (uint32_t j = 0; j < BAMTAG_SCAN_PER && first + j < n; ++j) { out_off[first + j] = at; at += size[first + j]; }
}

}  // namespace dropest
