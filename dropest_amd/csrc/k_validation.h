// k_validation.h -- the pair sampler of `dropest -S` (Estimation/Merge/MergeProbabilityValidator.cpp:8-46) and the kernels that build the
// validation view of the filtered cells' molecules (validation.h).
//
// Sampler: the host draws rand() values, two per candidate pair; one lane per candidate takes a = r0 % F, b = r1 % F, rejects a == b (:29-30)
// and otherwise runs Tools::edit_distance(barcode a, barcode b, skip_n = true, max_ed = min_ed) exactly as Tools/UtilFunctions.cpp:32-65
// writes it: a banded DP over ONE column that is a plain array, so cells outside the band keep what an earlier row left there, with the early
// return of the row minimum once that exceeds the band.  The value it returns is what the sample tests and records, so nothing of this may
// be "improved" into a Levenshtein distance.
//
// The column (at most VAL_COL cells) and the two barcodes of a lane live in LDS: a per-lane array indexed by a loop variable would go to
// scratch.  Cell i of thread t stands at word i * VAL_THREADS + t, so the lanes of a wave read 64 consecutive words: every lane of a 32-lane
// half on its own bank.  Only the band of a row is touched (2 * band + 1 cells at most).
//
// Compaction in candidate order: the sample kernel leaves one word per candidate (0, or VAL_ACCEPT | distance) and the number of accepted
// candidates per block; after the scan of those (scan_counts) the scatter kernel places the k-th accepted candidate of the round at
// found_before + k -- ballot + popcount inside the wave, wave offsets in the block, the scanned block offsets -- and drops what lies
// beyond the n-th.
#pragma once

#include "util.h"

namespace dropest {

constexpr int VAL_THREADS = 256;
constexpr int VAL_STRIDE = 32;            // bytes of a barcode row: up to 31 characters, the length in the last byte
constexpr int VAL_COL = 32;               // column cells per lane: barcodes of up to 31 characters
constexpr uint32_t VAL_ACCEPT = 0x80000000u;

__device__ inline uint32_t val_byte(const uint32_t *words, int i) { return (words[(i >> 2) * VAL_THREADS] >> ((i & 3) * 8)) & 0xFFu; }

// Tools::edit_distance(s1, s2, true, band); col / s1 / s2: this lane's words, VAL_THREADS apart
__device__ inline uint32_t val_banded_distance(uint32_t *col, const uint32_t *s1, const uint32_t *s2, int n1, int n2, int band) {
	for (int i = 0; i <= n1; ++i) col[i * VAL_THREADS] = uint32_t(i);
	for (int j = 1; j <= n2; ++j) {
		const int lower = max(0, j - band), upper = min(n1, j + band);
		if (lower > n1) return uint32_t(j);   // (an empty s1 only: the reference reads outside its array there)
		int lastdiag = int(col[lower * VAL_THREADS]);
		col[lower * VAL_THREADS] = uint32_t(j);
		int left = j, min_ed = j;
		const uint32_t c2 = val_byte(s2, j - 1);
		for (int i = lower + 1; i <= upper; ++i) {
			const int olddiag = int(col[i * VAL_THREADS]);
			const uint32_t c1 = val_byte(s1, i - 1);
			const bool match = c1 == c2 || c1 == 'N' || c2 == 'N';
			const int v = min(min(olddiag + 1, left + 1), lastdiag + int(!match));
			min_ed = min(min_ed, v + abs(i - j));
			col[i * VAL_THREADS] = uint32_t(v);
			left = v;
			lastdiag = olddiag;
		}
		if (min_ed > band) return uint32_t(min_ed);
	}
	return col[n1 * VAL_THREADS];
}

// candidate i of the round: rnd[2 i], rnd[2 i + 1] -> result[i], block_count[block]
__global__ __launch_bounds__(VAL_THREADS) void validation_sample_kernel(const uint32_t *__restrict__ rnd, uint32_t n_cand, uint32_t F,
                                                                        const uint4 *__restrict__ barcodes, uint32_t min_ed, uint32_t max_ed,
                                                                        uint32_t *__restrict__ result, uint32_t *__restrict__ block_count) {
	__shared__ uint32_t col[VAL_COL * VAL_THREADS];
	__shared__ uint32_t text[2 * (VAL_STRIDE / 4) * VAL_THREADS];
	__shared__ uint32_t wave_n[VAL_THREADS / 64];
	const uint32_t i = blockIdx.x * VAL_THREADS + threadIdx.x;
	uint32_t res = 0;
	if (i < n_cand) {
		const uint32_t a = rnd[2 * size_t(i)] % F, b = rnd[2 * size_t(i) + 1] % F;
		if (a != b) {
			uint32_t *s1 = text + threadIdx.x, *s2 = s1 + (VAL_STRIDE / 4) * VAL_THREADS;
			const uint4 a0 = barcodes[2 * size_t(a)], a1 = barcodes[2 * size_t(a) + 1], b0 = barcodes[2 * size_t(b)], b1 = barcodes[2 * size_t(b) + 1];
			s1[0 * VAL_THREADS] = a0.x; s1[1 * VAL_THREADS] = a0.y; s1[2 * VAL_THREADS] = a0.z; s1[3 * VAL_THREADS] = a0.w;
			s1[4 * VAL_THREADS] = a1.x; s1[5 * VAL_THREADS] = a1.y; s1[6 * VAL_THREADS] = a1.z; s1[7 * VAL_THREADS] = a1.w;
			s2[0 * VAL_THREADS] = b0.x; s2[1 * VAL_THREADS] = b0.y; s2[2 * VAL_THREADS] = b0.z; s2[3 * VAL_THREADS] = b0.w;
			s2[4 * VAL_THREADS] = b1.x; s2[5 * VAL_THREADS] = b1.y; s2[6 * VAL_THREADS] = b1.z; s2[7 * VAL_THREADS] = b1.w;
			const int n1 = min(int(a1.w >> 24), VAL_COL - 1), n2 = min(int(b1.w >> 24), VAL_COL - 1);   // (the host refuses longer barcodes)
			const uint32_t ed = val_banded_distance(col + threadIdx.x, s1, s2, n1, n2, int(min_ed));
			if (ed >= min_ed && ed <= max_ed) res = VAL_ACCEPT | ed;
		}
		result[i] = res;
	}
	const unsigned long long m = __ballot(res != 0);
	if (lane_id() == 0) wave_n[wave_id()] = uint32_t(__popcll(m));
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t t = 0;
#pragma unroll
		for (int w = 0; w < VAL_THREADS / 64; ++w) t += wave_n[w];
		block_count[blockIdx.x] = t;
	}
}

// the k-th accepted candidate of the round -> entry found_before + k of the sample, while that is below n_want
__global__ __launch_bounds__(VAL_THREADS) void validation_scatter_kernel(const uint32_t *__restrict__ rnd, const uint32_t *__restrict__ result,
                                                                         uint32_t n_cand, uint32_t F, const uint32_t *__restrict__ block_off,
                                                                         uint32_t found_before, uint32_t n_want, uint32_t *__restrict__ out_a,
                                                                         uint32_t *__restrict__ out_b, uint32_t *__restrict__ out_ed,
                                                                         uint32_t *__restrict__ out_cand) {
	__shared__ uint32_t wave_n[VAL_THREADS / 64];
	const uint32_t i = blockIdx.x * VAL_THREADS + threadIdx.x;
	const uint32_t res = i < n_cand ? result[i] : 0u;
	const unsigned long long m = __ballot(res != 0);
	if (lane_id() == 0) wave_n[wave_id()] = uint32_t(__popcll(m));
	__syncthreads();
	if (!res) return;
	uint32_t pos = block_off[blockIdx.x] + uint32_t(__popcll(m & ((1ull << lane_id()) - 1ull)));
	for (uint32_t w = 0; w < wave_id(); ++w) pos += wave_n[w];
	if (pos >= n_want - found_before) return;   // beyond the n-th accepted pair
	pos += found_before;
	out_a[pos] = rnd[2 * size_t(i)] % F;
	out_b[pos] = rnd[2 * size_t(i) + 1] % F;
	out_ed[pos] = res & ~VAL_ACCEPT;
	out_cand[pos] = i;
}

// ---- the validation view (validation.h) ----------------------------------------------------------------------------------------------
// molecule rows of the filtered cells -> view keys rank(cell) << (gene_bits + view_umi_bits) | gene << view_umi_bits | UMI field; rows of
// gene-less reads, of cells that are not filtered and of the (cell, gene) groups in `rewritten` (ascending keys >> umi_bits; the host
// appends their current contents) are dropped.  Any order: the keys are sorted afterwards.
__global__ __launch_bounds__(256) void validation_view_keys_kernel(const unsigned long long *__restrict__ mol_key, uint32_t n_mol, int umi_bits,
                                                                   int gene_bits, unsigned long long gene_none, int view_umi_bits,
                                                                   const uint32_t *__restrict__ cell_rank,
                                                                   const unsigned long long *__restrict__ rewritten, uint32_t n_rewritten,
                                                                   unsigned long long *__restrict__ out, uint32_t *__restrict__ count) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	bool keep = false;
	unsigned long long key = 0;
	if (i < n_mol) {
		const unsigned long long k = mol_key[i], cg = k >> umi_bits, g = cg & gene_none;
		const uint32_t rank = cell_rank[uint32_t(cg >> gene_bits)];
		keep = g != gene_none && rank != 0xFFFFFFFFu;
		if (keep && n_rewritten) {
			uint32_t lo = 0, hi = n_rewritten;
			while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (rewritten[mid] < cg) lo = mid + 1; else hi = mid; }
			keep = !(lo < n_rewritten && rewritten[lo] == cg);
		}
		key = ((((unsigned long long)rank << gene_bits) | g) << view_umi_bits) | (k & ((1ull << umi_bits) - 1ull));
	}
	const unsigned long long m = __ballot(keep);
	uint32_t base = 0;
	if (lane_id() == 0 && m) base = atomicAdd(count, uint32_t(__popcll(m)));
	base = __shfl(base, 0, 64);
	if (keep) out[base + __popcll(m & ((1ull << lane_id()) - 1ull))] = key;
}

__global__ __launch_bounds__(256) void validation_shift_keys_kernel(const unsigned long long *__restrict__ in, uint32_t n, int shift,
                                                                    unsigned long long mask, unsigned long long *__restrict__ out) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i < n) out[i] = (in[i] >> shift) & mask;
}

// (cell, gene) runs of one cell: run r of the cells that have molecules -> cell_cg_begin / cell_cg_count of its rank
__global__ __launch_bounds__(256) void validation_cell_rows_kernel(const unsigned long long *__restrict__ run_cell, const uint32_t *__restrict__ run_count,
                                                                   const uint32_t *__restrict__ run_begin, uint32_t n_runs,
                                                                   uint32_t *__restrict__ cell_cg_begin, uint32_t *__restrict__ cell_cg_count) {
	const uint32_t r = blockIdx.x * 256 + threadIdx.x;
	if (r >= n_runs) return;
	const uint32_t cell = uint32_t(run_cell[r]);
	cell_cg_begin[cell] = run_begin[r];
	cell_cg_count[cell] = run_count[r];
}

// ---- the view across shards (shard_validation.h) ---------------------------------------------------------------------------------------
// One shard's sorted view keys: first row and the row behind the last one of every cell that has rows (cell = key >> shift, a position in
// the global filtered order; seg_begin / seg_end have one word per position and were zeroed).
__global__ __launch_bounds__(256) void validation_cell_segments_kernel(const unsigned long long *__restrict__ keys, uint32_t n, int shift,
                                                                       uint32_t n_cells, uint32_t *__restrict__ seg_begin,
                                                                       uint32_t *__restrict__ seg_end) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const unsigned long long cell = keys[i] >> shift;
	if (cell >= n_cells) return;
	if (i == 0 || (keys[i - 1] >> shift) != cell) seg_begin[cell] = i;
	if (i + 1 == n || (keys[i + 1] >> shift) != cell) seg_end[cell] = i + 1;
}

// The all-gathered view is `world` sorted blocks, and every cell's rows lie in one of them: a cell-granular interleave, so the global order
// is a copy of every cell's segment to its place and no sort.  Per cell: first row in the gathered buffer, rows, first row in the global
// order.  Cells are cut into pieces of VAL_SEG rows (piece s = rows [piece_first[s], + VAL_SEG) of cell piece_cell[s]) so that one huge cell
// is many blocks' work; a block takes pieces grid-stride.  16 bytes per lane where source and destination sit alike in their 16-byte lines
// (both bases are 16-byte aligned, a piece starts at a multiple of VAL_SEG rows: the question is one bit per cell), 8 bytes per lane otherwise.
constexpr uint32_t VAL_SEG = 4096;
__global__ __launch_bounds__(256) void validation_place_kernel(const unsigned long long *__restrict__ gathered, unsigned long long *__restrict__ placed,
                                                               const uint32_t *__restrict__ cell_src, const uint32_t *__restrict__ cell_cnt,
                                                               const uint32_t *__restrict__ cell_dst, const uint32_t *__restrict__ piece_cell,
                                                               const uint32_t *__restrict__ piece_first, uint32_t n_pieces) {
	for (uint32_t s = blockIdx.x; s < n_pieces; s += gridDim.x) {
		const uint32_t c = piece_cell[s], first = piece_first[s], cnt = cell_cnt[c];
		if (first >= cnt) continue;
		const uint32_t n = min(VAL_SEG, cnt - first);
		const size_t src = size_t(cell_src[c]) + first, dst = size_t(cell_dst[c]) + first;
		const unsigned long long *in = gathered + src;
		unsigned long long *out = placed + dst;
		if (((src ^ dst) & 1u) == 0) {
			const uint32_t head = uint32_t(src & 1u);   // (n >= 1)
			if (head && threadIdx.x == 0) out[0] = in[0];
			const uint32_t pairs = (n - head) >> 1;
			const ulonglong2 *in2 = reinterpret_cast<const ulonglong2 *>(in + head);
			ulonglong2 *out2 = reinterpret_cast<ulonglong2 *>(out + head);
			for (uint32_t i = threadIdx.x; i < pairs; i += 256) out2[i] = in2[i];
			if (((n - head) & 1u) && threadIdx.x == 0) out[n - 1] = in[n - 1];
		} else
			for (uint32_t i = threadIdx.x; i < n; i += 256) out[i] = in[i];
	}
}

}  // namespace dropest
