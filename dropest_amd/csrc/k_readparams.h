// k_readparams.h -- the read-parameter files of -r as a table on the device: read name -> barcode, UMI, UMI quality, quality verdict.
//
// What it replaces: ReadMapParamsParser::init (Estimation/BamProcessing/ReadMapParamsParser.cpp:50-108), which fills an unordered_map row by row
// on one thread, and ReadMapParamsParser::get_read_params (:22-48), which looks a read's name up and ERASES the entry: a name serves once, the
// first record of the file order that asks for it.  Here the host only inflates the files and finds the line starts; a lane per line does what
// ReadParameters::parse_from_string / check_quality (Tools/ReadParameters.cpp:58-78, 118-136) do (rp_rows_kernel), a lane per valid row enters
// it into an open-addressed table keyed by the name (rp_insert_kernel: the first row of a name is the canonical one, as emplace keeps the first),
// and "serves once" is an array of 64-bit claims: every record that finds row r does atomicMin(&claim[r], its ordinal in the stream), and a later
// launch serves the record whose ordinal stands there (bam_params_settle_kernel, k_bamparse.h).
// Byte work over text, a few dependent loads per probe; no MFMA.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dropest {

constexpr uint32_t RP_NONE = 0xFFFFFFFFu;

// One line of the files (the layout of dropest_read_params_row, include/dropest_bgzf.h).  Offsets are into the table's text: the bytes of every
// _add_text call one after the other.
struct RpRow {
	unsigned long long hash;                 // FNV-1a 64 of the name under the table's hash mask
	unsigned long long cb_code, umi_code;    // bam_pack_bases: 0 = does not pack (an N, more than 31 bases)
	unsigned long long name_off, cb_off, umi_off, quality_off;
	uint32_t name_len, cb_len, umi_len, quality_len;
	uint32_t canonical;                      // the first row of this name (itself when it is the first), RP_NONE in a row that is not valid: filled
	                                         // on the way to the host from an array of its own (rp_canonical_kernel), RP_NONE on the device
	uint8_t valid, pass, empty, pad;
};

// what the look-ups read (every array finished before the launch that probes)
struct RpTable {
	const uint32_t *slots;                   // row + 1, 0 = empty
	uint32_t mask;
	const RpRow *rows;
	const uint8_t *text;
	unsigned long long *claim;               // per row: the lowest ordinal that asked for it, all ones = nobody yet
	unsigned long long hash_mask;
};

__host__ __device__ inline uint32_t rp_slot(unsigned long long h, uint32_t mask) { return uint32_t((h ^ (h >> 29)) * 0x9E3779B97F4A7C15ull >> 40) & mask; }

__device__ inline unsigned long long rp_hash(const uint8_t *s, uint32_t n, unsigned long long hash_mask) {
	unsigned long long h = 1469598103934665603ull;
	for (uint32_t i = 0; i < n; ++i) { h ^= s[i]; h *= 1099511628211ull; }
	return h & hash_mask;
}

__device__ inline unsigned long long rp_pack_bases(const uint8_t *s, uint32_t n) {   // = bam_pack_bases (k_bamparse.h)
	if (n == 0u || n > 31u) return 0ull;
	unsigned long long c = 1;
	for (uint32_t i = 0; i < n; ++i) {
		const uint8_t ch = s[i];
		uint32_t b;
		if (ch == 'A') b = 0; else if (ch == 'C') b = 1; else if (ch == 'G') b = 2; else if (ch == 'T') b = 3; else return 0ull;
		c = (c << 2) | b;
	}
	return c;
}

__device__ inline bool rp_same_name(const RpTable &t, const RpRow &r, unsigned long long h, const uint8_t *name, uint32_t n) {
	if (r.hash != h || r.name_len != n) return false;
	const uint8_t *q = t.text + r.name_off;
	for (uint32_t i = 0; i < n; ++i) if (q[i] != name[i]) return false;
	return true;
}

// The canonical row of `name` (no '@' in front any more), RP_NONE when the files do not list it.  `name` may stand in LDS or in memory.
__device__ inline uint32_t rp_lookup(const RpTable &t, const uint8_t *name, uint32_t n) {
	const unsigned long long h = rp_hash(name, n, t.hash_mask);
	uint32_t sl = rp_slot(h, t.mask);
	for (uint32_t step = 0; step <= t.mask; ++step) {      // (the table is never full: at least as many empty slots as rows)
		const uint32_t v = t.slots[sl];
		if (!v) return RP_NONE;
		if (rp_same_name(t, t.rows[v - 1], h, name, n)) return v - 1;
		sl = (sl + 1) & t.mask;
	}
	return RP_NONE;
}

// A lane per line first .. first + n of the text: line k is text[line_be[2 k] .. line_be[2 k + 1]) with its '\n' (the last line of a file may
// have none).  BamController::load_read_params restated: a '\r' in front of the '\n' goes with it; an empty line is nothing; four fields that
// end at a single space, the fifth is the rest; one '@' off the name; an empty barcode or UMI is no row; the quality verdict.
__global__ __launch_bounds__(256) void rp_rows_kernel(const uint8_t *__restrict__ text, const unsigned long long *__restrict__ line_be, uint32_t first, uint32_t n,
                                                      int32_t min_phred, unsigned long long hash_mask, RpRow *__restrict__ rows) {
	const uint32_t k = blockIdx.x * 256 + threadIdx.x;
	if (k >= n) return;
	unsigned long long b = line_be[2ull * (first + k)], e = line_be[2ull * (first + k) + 1];
	RpRow r{};
	r.canonical = RP_NONE;
	if (e > b && text[e - 1] == '\n') { --e; if (e > b && text[e - 1] == '\r') --e; }
	r.empty = e == b;
	unsigned long long at = b, field_b[5], field_e[5];
	bool ok = !r.empty;
	for (int f = 0; f < 4 && ok; ++f) {
		unsigned long long sp = at;
		while (sp < e && text[sp] != ' ') ++sp;
		if (sp == e) { ok = false; break; }
		field_b[f] = at; field_e[f] = sp;
		at = sp + 1;
	}
	if (ok) {
		field_b[4] = at; field_e[4] = e;
		if (field_e[0] > field_b[0] && text[field_b[0]] == '@') ++field_b[0];
		ok = field_e[1] > field_b[1] && field_e[2] > field_b[2];
	}
	if (ok) {
		bool pass = true;
		if (min_phred > 33)
			for (int f = 3; f < 5; ++f)
				for (unsigned long long j = field_b[f]; j < field_e[f]; ++j) pass &= int32_t(int8_t(text[j])) >= int32_t(int8_t(min_phred));
		r.valid = 1; r.pass = pass ? 1 : 0;
		r.name_off = field_b[0]; r.name_len = uint32_t(field_e[0] - field_b[0]);
		r.cb_off = field_b[1]; r.cb_len = uint32_t(field_e[1] - field_b[1]);
		r.umi_off = field_b[2]; r.umi_len = uint32_t(field_e[2] - field_b[2]);
		r.quality_off = field_b[4]; r.quality_len = uint32_t(field_e[4] - field_b[4]);
		r.cb_code = rp_pack_bases(text + r.cb_off, r.cb_len); r.umi_code = rp_pack_bases(text + r.umi_off, r.umi_len);
		r.hash = rp_hash(text + r.name_off, r.name_len, hash_mask);
	}
	rows[first + k] = r;
}

// A lane per row enters the valid ones.  The slot word (row + 1) is the only thing the workgroups of this launch exchange, and only through
// atomics; rows and text were finished by earlier launches.  A slot, once taken, keeps its NAME for good -- atomicMin only ever puts another row
// of the same name there -- so every probe sequence sees the same names in the same places whoever came first, and the lowest row of a name, the
// first in the files, is what stands there in the end.
__global__ __launch_bounds__(256) void rp_insert_kernel(RpTable t, uint32_t *__restrict__ slots, uint32_t n_rows) {
	const uint32_t k = blockIdx.x * 256 + threadIdx.x;
	if (k >= n_rows) return;
	const RpRow me = t.rows[k];
	if (!me.valid) return;
	uint32_t sl = rp_slot(me.hash, t.mask);
	for (uint32_t step = 0; step <= t.mask; ++step) {
		const uint32_t was = atomicCAS(&slots[sl], 0u, k + 1);
		if (!was) return;
		if (rp_same_name(t, t.rows[was - 1], me.hash, t.text + me.name_off, me.name_len)) { atomicMin(&slots[sl], k + 1); return; }
		sl = (sl + 1) & t.mask;
	}
}

// ... and, in a launch of its own, every valid row's canonical row (an array beside the rows, which the probes of this launch read);
// counts: valid rows, rows that are neither valid nor empty, valid rows that repeat an earlier name
__global__ __launch_bounds__(256) void rp_canonical_kernel(RpTable t, uint32_t *__restrict__ canonical, uint32_t n_rows, uint32_t *__restrict__ counts) {
	const uint32_t k = blockIdx.x * 256 + threadIdx.x;
	if (k >= n_rows) return;
	const RpRow me = t.rows[k];
	if (!me.valid) { canonical[k] = RP_NONE; if (!me.empty) atomicAdd(&counts[1], 1u); return; }
	const uint32_t c = rp_lookup(t, t.text + me.name_off, me.name_len);
	canonical[k] = c;
	atomicAdd(&counts[0], 1u);
	if (c != k) atomicAdd(&counts[2], 1u);
}

// names[off[k] .. off[k + 1]) -> the canonical row (one '@' in front is passed over, as the reader does with a record's name)
__global__ __launch_bounds__(256) void rp_lookup_kernel(RpTable t, const uint8_t *__restrict__ names, const unsigned long long *__restrict__ off, uint32_t n,
                                                        uint32_t *__restrict__ out_row) {
	const uint32_t k = blockIdx.x * 256 + threadIdx.x;
	if (k >= n) return;
	const uint8_t *s = names + off[k];
	uint32_t len = uint32_t(off[k + 1] - off[k]);
	if (len && s[0] == '@') { ++s; --len; }
	out_row[k] = rp_lookup(t, s, len);
}

}  // namespace dropest
