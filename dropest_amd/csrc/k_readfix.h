// k_readfix.h -- what the FINAL container made of every resident read: the decision FilteringBamProcessor::write_alignment takes per
// BAM record (Estimation/BamProcessing/FilteringBamProcessor.cpp:14-40, :61-96), for all reads at once.  Host side: read_corrections.h.
//
//   rule      read i, in stream order:
//               1 no gene                                                      (read_info.gene.empty(), :63-64)
//               2 its barcode's cell b has merge target t and t is not a filtered cell            (_merge_cbs, :22-37, :66-68)
//               3 cell t has no such gene                                                                       (:70-76)
//               0 (t, gene) has the read's UMI as a SOURCE of Gene::merge_targets(): the UMI becomes that target -- one hop, not
//                 looked up among the molecules, and before the next test                                      (:79-83)
//               0 (t, gene) has the read's UMI as a molecule: the read keeps it                                 (:84-87)
//               4 neither                                                                                       (:88-92)
//
//   shape     One lane per read, blocks of 256 over a grid-stride loop: the three columns are read once, coalesced (8 + 4 + 8 bytes), the
//             three results written once, coalesced (1 + 4 + 8 bytes).  Everything between is dependent look-ups, so the kernel lives on
//             occupancy: no LDS, no MFMA, few registers.
//   cell      barcode -> table slot -> cell id through the barcode table the pass built (cb_find, k_cbhash.h): one divergent 16-byte
//             gather per read, the access that bounds cb_insert.  No per-read cell id outlives the pass.  What does is cb_insert's `slot`
//             array: a table slot per read, or an index into the hot-barcode list.  The cell id lives IN the slot, so going through that
//             array would still gather the slot's line per read and save only the hash and the key compare, at the price of tying this
//             kernel to cb_insert's encodings: not used.
//   kept      cell id -> rank among the filtered cells (merge targets folded in on the host: a merged cell holds its target's rank), or
//             none: one u32 array over the cells.  rank -> cell id and the row ranges below are arrays over the filtered cells.
//   molecules the filtered cells' molecules as keys rank | gene | UMI field, sorted (k_radix.h); a cell's rows are one range, and ONE binary
//             search for the read's own key inside it answers both "is a molecule" (the row found) and "has the gene" (the row found or
//             the one before it is a row of the gene).  A cell of a thousand molecules costs about ten dependent loads, not the 22 of the
//             whole table.  Searching the gene first and the UMI from there took twice the loads and twice the time.
//   sources   the UMI merge targets of the filtered cells under the same keys, sorted, with the target codes beside them: usually a tiny
//             array, empty unless dropest_set_save_umi_merge_targets is on.  Searched first, inside the cell's own range.
//   diverge   reads that fail tests 1-2 leave their lane idle while the others search.  Compacting the survivors first would cost a pass of
//             its own over a stream where at least a quarter, usually most, of the reads survive: not done.
//   counts    one count per verdict: every lane keeps five wave-uniform sums (ballots), lane 0 of each wave adds them once at the end.
//   look-up   the step barcode -> rank is the kernel's template parameter.  RfOwnCells: the one context's, as above.  RfColumnTable: a shard
//             of a sharded run (shard_read_corrections.h) sees reads whose barcodes other shards own, so it asks a table that every shard
//             holds alike: barcode -> column of cm, one open-addressed probe of a 16-byte slot {barcode, column, set}, hashed with mix64 and
//             probed linearly like the pass's own table; key 0 is the empty slot (a packed code carries a sentinel bit, an escaped one bit
//             63).  rank = column = what is written as the target, so rank -> cell id falls away.  bc_insert_kernel builds the table: a
//             barcode that arrives with two different columns raises a flag, nothing is overwritten.  The table is kept cells plus their
//             merged sources -- tens of thousands of slots, L2-resident -- and lives in global memory only.
#pragma once

#include "k_cbhash.h"

namespace dropest {

constexpr uint32_t RF_NONE = 0xFFFFFFFFu;
enum : uint8_t { RF_WRITTEN = 0, RF_NO_GENE = 1, RF_CELL_NOT_KEPT = 2, RF_WRONG_GENE = 3, RF_WRONG_UMI = 4 };

// barcode -> column of cm, replicated on every shard.  `set`: 0 = no column yet, 1 = column written (one 64-bit word with it: one CAS)
struct BcColSlot {
	unsigned long long key;                      // barcode code, 0 = empty
	uint32_t column;
	uint32_t set;
};
static_assert(sizeof(BcColSlot) == 16, "slot layout");

struct ReadFixArgs {
	const unsigned long long *cb, *umi;          // the resident columns
	const uint32_t *gene;
	uint32_t n;
	CbTable table;
	const uint32_t *cell_rank;                   // [cells] rank of the cell's merge target among the filtered cells, RF_NONE: not kept
	const uint32_t *kept_cell;                   // [F] rank -> cell id
	const unsigned long long *mol_key;           // sorted: rank | gene | UMI field
	const uint32_t *mol_begin, *mol_end;         // [F] rows of a rank
	const unsigned long long *src_key;           // sorted: rank | gene | source UMI field
	const unsigned long long *src_target;        // the corrected UMI of each, packed / escaped
	const uint32_t *src_begin, *src_end;         // [F]
	uint32_t n_src;
	int gene_bits, umi_bits;
	unsigned long long gene_none, umi_strip_mask, umi_escape_base;
	uint8_t *verdict;
	uint32_t *cell;                              // target cell id; RF_NONE for verdicts 1 and 2
	unsigned long long *umi_out;                 // corrected UMI (verdict 0), the read's own otherwise
	unsigned long long *counts;                  // [5], zeroed by the caller
	// RfColumnTable only (behind everything RfOwnCells reads: that instantiation's argument offsets stay what they were)
	const BcColSlot *bc_slots;
	uint32_t bc_mask;                            // capacity - 1
};

struct BcPair { unsigned long long barcode; uint32_t column, pad; };   // what the shards gather: one per own cell whose target is a column
static_assert(sizeof(BcPair) == 16, "pair layout");

enum : uint32_t { BC_FLAG_DUPLICATE = 1u, BC_FLAG_FULL = 2u, BC_FLAG_BAD_KEY = 4u };

// One lane per (barcode, column) pair.  capacity = mask + 1 is a power of two of at least twice n, so a free slot always exists; the probe
// is bounded by the capacity all the same.  flags: BC_FLAG_* of what went wrong (the host turns any of them into an error).
__global__ __launch_bounds__(256) void bc_insert_kernel(const BcPair *__restrict__ pairs, uint32_t n, BcColSlot *slots, uint32_t mask, uint32_t *flags) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const unsigned long long k = pairs[i].barcode;
	if (k == 0ull) { atomicOr(flags, BC_FLAG_BAD_KEY); return; }
	const unsigned long long mine = (1ull << 32) | pairs[i].column;   // {column, set = 1} as the slot's second word
	uint32_t h = uint32_t(mix64(k)) & mask;
	for (uint32_t probe = 0; probe <= mask; ++probe, h = (h + 1) & mask) {
		unsigned long long cur = slots[h].key;
		if (cur == 0ull) cur = atomicCAS(&slots[h].key, 0ull, k);   // (the CAS's answer is the authority; 0: the slot is mine now)
		if (cur != 0ull && cur != k) continue;
		const unsigned long long was = atomicCAS(reinterpret_cast<unsigned long long *>(&slots[h].column), 0ull, mine);
		if (was != 0ull && was != mine) atomicOr(flags, BC_FLAG_DUPLICATE);
		return;
	}
	atomicOr(flags, BC_FLAG_FULL);
}

__device__ inline uint32_t bc_find(const BcColSlot *__restrict__ slots, uint32_t mask, unsigned long long k) {   // the column, RF_NONE if absent
	uint32_t h = uint32_t(mix64(k)) & mask;
	for (uint32_t probe = 0; probe <= mask; ++probe, h = (h + 1) & mask) {
		const unsigned long long cur = slots[h].key;
		if (cur == k) return slots[h].column;
		if (cur == 0ull) return 0xFFFFFFFFu;
	}
	return 0xFFFFFFFFu;
}

// (test hook and nothing else: the columns of `n` barcodes, one lane each)
__global__ __launch_bounds__(256) void bc_probe_kernel(const unsigned long long *__restrict__ barcode, uint32_t n, const BcColSlot *__restrict__ slots, uint32_t mask,
                                                       uint32_t *__restrict__ column) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i < n) column[i] = barcode[i] ? bc_find(slots, mask, barcode[i]) : 0xFFFFFFFFu;
}

// barcode -> rank among the kept cells, and rank -> what is written as the read's target
struct RfOwnCells {      // one context: the pass's barcode table, the cells' ranks, the kept cells' ids
	__device__ static uint32_t rank(const ReadFixArgs &a, unsigned long long cb) {
		const uint32_t s = cb_find(a.table, cb);
		return s == 0xFFFFFFFFu ? 0xFFFFFFFFu : a.cell_rank[a.table.slots[s].cell_id];
	}
	__device__ static uint32_t target(const ReadFixArgs &a, uint32_t rank) { return a.kept_cell[rank]; }
};
struct RfColumnTable {   // a shard: the replicated table; the rank IS the column of cm
	__device__ static uint32_t rank(const ReadFixArgs &a, unsigned long long cb) { return cb ? bc_find(a.bc_slots, a.bc_mask, cb) : 0xFFFFFFFFu; }
	__device__ static uint32_t target(const ReadFixArgs &, uint32_t rank) { return rank; }
};

__device__ inline uint32_t rf_lower_bound(const unsigned long long *__restrict__ k, uint32_t lo, uint32_t hi, unsigned long long want) {
	while (lo < hi) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (k[mid] < want) lo = mid + 1; else hi = mid;
	}
	return lo;
}

template <class Lookup>
__global__ __launch_bounds__(256) void read_corrections_kernel(ReadFixArgs a) {
	uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;   // wave-uniform
	const size_t stride = size_t(gridDim.x) * 256u;
	for (size_t base = size_t(blockIdx.x) * 256u; base < a.n; base += stride) {   // (every lane of a wave makes the same trips: the ballots below)
		const size_t i = base + threadIdx.x;
		uint32_t v = 0xFFu;
		if (i < a.n) {
			const uint32_t g = a.gene[i];
			const unsigned long long u = a.umi[i];
			uint32_t cell = RF_NONE;
			unsigned long long fixed = u;
			v = RF_NO_GENE;
			if (g != NO_GENE) {
				v = RF_CELL_NOT_KEPT;
				const uint32_t rank = Lookup::rank(a, a.cb[i]);
				if (rank != RF_NONE) {
					cell = Lookup::target(a, rank);
					v = RF_WRONG_GENE;
					if (g < a.gene_none) {
						const uint32_t b = a.mol_begin[rank], e = a.mol_end[rank];
						const unsigned long long cg = ((unsigned long long)rank << a.gene_bits) | g;
						const unsigned long long field = (u & ESCAPE_BIT) ? (a.umi_escape_base + (u & ~ESCAPE_BIT)) : (u & a.umi_strip_mask);
						// (a UMI the key's field cannot hold is no molecule's and no source's: both come out of such keys; the search then
						// only looks for the gene)
						const bool fits = a.umi_bits >= 64 || (field >> a.umi_bits) == 0;
						const unsigned long long want = (cg << a.umi_bits) | (fits ? field : 0ull);
						// ONE search answers both questions: q is the first row not below the wanted key, so the gene's rows, if it has any,
						// include row q (a row of the gene at or above the key) or row q - 1 (the gene's last row, below it)
						const uint32_t q = rf_lower_bound(a.mol_key, b, e, want);
						const unsigned long long at = q < e ? a.mol_key[q] : ~0ull;
						const bool is_molecule = fits && q < e && at == want;
						bool has_gene = q < e && (at >> a.umi_bits) == cg;
						if (!has_gene && q > b) has_gene = (a.mol_key[q - 1] >> a.umi_bits) == cg;
						if (has_gene) {
							v = is_molecule ? RF_WRITTEN : RF_WRONG_UMI;
							if (fits && a.n_src) {   // a source goes to its target whether or not it is a molecule too
								const uint32_t se = a.src_end[rank];
								const uint32_t p = rf_lower_bound(a.src_key, a.src_begin[rank], se, want);
								if (p < se && a.src_key[p] == want) { fixed = a.src_target[p]; v = RF_WRITTEN; }
							}
						}
					}
				}
			}
			a.verdict[i] = uint8_t(v);
			a.cell[i] = cell;
			a.umi_out[i] = fixed;
		}
		c0 += uint32_t(__popcll(__ballot(v == RF_WRITTEN)));
		c1 += uint32_t(__popcll(__ballot(v == RF_NO_GENE)));
		c2 += uint32_t(__popcll(__ballot(v == RF_CELL_NOT_KEPT)));
		c3 += uint32_t(__popcll(__ballot(v == RF_WRONG_GENE)));
		c4 += uint32_t(__popcll(__ballot(v == RF_WRONG_UMI)));
	}
	if (lane_id() == 0) {
		if (c0) atomicAdd(a.counts + 0, (unsigned long long)c0);
		if (c1) atomicAdd(a.counts + 1, (unsigned long long)c1);
		if (c2) atomicAdd(a.counts + 2, (unsigned long long)c2);
		if (c3) atomicAdd(a.counts + 3, (unsigned long long)c3);
		if (c4) atomicAdd(a.counts + 4, (unsigned long long)c4);
	}
}

// The molecules a device UMI merge re-keyed (k_umi_directional.h writes the new key of every row beside the old one): (old key, new key)
// of the rows whose keys differ, in no particular order -- what Gene::merge(source, target) would have recorded for them (Gene.cpp:54-57).
// `cap` = the number the merge counted; a row beyond it is not written.
__global__ __launch_bounds__(256) void umi_rekeyed_rows_kernel(const unsigned long long *__restrict__ old_key, const unsigned long long *__restrict__ new_key,
                                                               uint32_t n, uint32_t cap, unsigned long long *__restrict__ out_old,
                                                               unsigned long long *__restrict__ out_new, uint32_t *__restrict__ count) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	const bool hit = i < n && old_key[i] != new_key[i];
	const unsigned long long m = __ballot(hit);
	uint32_t base = 0;
	if (lane_id() == 0 && m) base = atomicAdd(count, uint32_t(__popcll(m)));
	base = __shfl(base, 0, 64);
	if (hit) {
		const uint32_t at = base + uint32_t(__popcll(m & ((1ull << lane_id()) - 1ull)));
		if (at < cap) { out_old[at] = old_key[i]; out_new[at] = new_key[i]; }
	}
}

}  // namespace dropest
