// k_shard.h -- the small kernels of a sharded pass (shard_run.h, shard_matrix.h): gathers by index, the placing of a shard's matrix
// columns in the global matrix (32-bit, 16-bit and byte form), cm_raw's column plan, local read position -> global stream ordinal, and the
// row sums / minima of tables gathered from every shard.
#pragma once

namespace dropest {

__global__ __launch_bounds__(256) void take_u32_kernel(const uint32_t *__restrict__ table, const uint32_t *__restrict__ pos, uint32_t n, uint32_t *__restrict__ out) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i < n) out[i] = table[pos[i]];
}
__global__ __launch_bounds__(256) void gather_u32_rows_kernel(const uint32_t *__restrict__ in, const uint32_t *__restrict__ row, uint32_t n, uint32_t width,
                                                              uint32_t *__restrict__ out) {
	for (uint64_t k = uint64_t(blockIdx.x) * 256 + threadIdx.x; k < uint64_t(n) * width; k += uint64_t(gridDim.x) * 256)
		out[k] = in[uint64_t(row[k / width]) * width + k % width];
}
struct ImportGatherArgs { const uint32_t *row; uint32_t n; const unsigned long long *low_all; const uint32_t *col_all[4]; unsigned long long *o_low; uint32_t *o_col[4]; };
__global__ __launch_bounds__(256) void import_gather_kernel(ImportGatherArgs a) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= a.n) return;
	const uint32_t r = a.row[i];
	a.o_low[i] = a.low_all[r];
#pragma unroll
	for (int k = 0; k < 4; ++k) a.o_col[k][i] = a.col_all[k][r];
}
// desc[3c .. 3c+2] = (src_start, dst_start, len) of column c; rows / values go to their places in the global matrix
struct ColumnDesc { unsigned long long s, d, len; };
__device__ inline ColumnDesc load_column_desc(const unsigned long long *__restrict__ desc, uint32_t c) { return ColumnDesc{desc[3ull * c], desc[3ull * c + 1], desc[3ull * c + 2]}; }
__global__ __launch_bounds__(256) void place_columns_kernel(const unsigned long long *__restrict__ desc, const uint32_t *__restrict__ src_rows,
                                                            const uint32_t *__restrict__ src_vals, uint32_t *__restrict__ dst_rows, uint32_t *__restrict__ dst_vals) {
	const auto [s, d, len] = load_column_desc(desc, blockIdx.x);
	for (unsigned long long t = threadIdx.x; t < len; t += 256) { dst_rows[d + t] = src_rows[s + t]; dst_vals[d + t] = src_vals[s + t]; }
}
// The same, narrowing on the way out (16-bit row indices and values: half the bytes over this shard's PCIe link); a value beyond
// 65534 is stored as 0xFFFF and listed exactly with its GLOBAL entry index (ovf[0] = count, then (position lo, position hi,
// value) triples, at most ovf_cap of them).
__global__ __launch_bounds__(256) void place_columns_narrow_kernel(const unsigned long long *__restrict__ desc, const uint32_t *__restrict__ src_rows,
                                                                   const uint32_t *__restrict__ src_vals, uint16_t *__restrict__ dst_rows, uint16_t *__restrict__ dst_vals,
                                                                   uint32_t *__restrict__ ovf, uint32_t ovf_cap) {
	const auto [s, d, len] = load_column_desc(desc, blockIdx.x);
	for (unsigned long long t = threadIdx.x; t < len; t += 256) {
		const uint32_t v = src_vals[s + t];
		dst_rows[d + t] = uint16_t(src_rows[s + t]);
		dst_vals[d + t] = v >= 0xFFFFu ? uint16_t(0xFFFFu) : uint16_t(v);
		if (v >= 0xFFFFu) {
			const uint32_t at = atomicAdd(ovf, 1u);
			if (at < ovf_cap) { ovf[1 + 3 * at] = uint32_t(d + t); ovf[2 + 3 * at] = uint32_t((d + t) >> 32); ovf[3 + 3 * at] = v; }
		}
	}
}
// The BYTE form (dropest_matrix_bytes, include/dropest_amd.h): u8 row delta + u8 value at the entry's GLOBAL place, two bytes per entry
// on the PCIe link.  A workgroup takes one column.  A lane takes SIXTEEN consecutive entries of an aligned group: a group that lies inside
// the column leaves as one 16-byte store per array (a wave writes 1 KB of each array in one piece: the link takes whole lines -- with
// 4-byte stores per lane the placing kernels of a C2 pass reached ~30 GB/s of the link's ~52), the ragged groups at a column's ends byte by
// byte (the neighbouring column may be another shard's).  Entries that do not fit a byte (255 = listed) go to this shard's segment of the
// shared buffer with their global position: a wave counts what its lanes list, takes its places with ONE atomic per kind on the shard's
// counters, and the lanes write their entries there (no LDS, no workgroup barrier); the readers concatenate the segments (the lists
// carry no order).
__global__ __launch_bounds__(256) void place_columns_bytes_kernel(const unsigned long long *__restrict__ desc, const uint32_t *__restrict__ src_rows,
                                                                  const uint32_t *__restrict__ src_vals, uint8_t *__restrict__ dst_delta,
                                                                  uint8_t *__restrict__ dst_val, uint32_t *__restrict__ counters /* [2] */,
                                                                  uint32_t *__restrict__ rl_pos, uint32_t *__restrict__ rl_row,
                                                                  uint32_t *__restrict__ vl_pos, uint32_t *__restrict__ vl_val, uint32_t cap,
                                                                  uint32_t *__restrict__ slot_rows = nullptr, uint32_t *__restrict__ slot_vals = nullptr,
                                                                  uint32_t *flag = nullptr, uint32_t epoch = 0) {
	// flag / epoch (matrix_decode.h): the arrival flag of the chunk of columns placed BEFORE this launch on the stream -- this kernel runs, so
	// that chunk is complete and visible to the host threads that widen it into the 32-bit slots.  slot_rows / slot_vals: the slots
	// themselves (node-shared host memory); a listed entry is written there directly, so the widening needs no list at all.
	if (flag && blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(flag, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
	const auto [s, d, len] = load_column_desc(desc, blockIdx.x);
	const uint32_t lane = threadIdx.x & 63u;
	const unsigned long long g0 = d >> 4, g1 = (d + len + 15) >> 4;
	for (unsigned long long gb = g0; gb < g1; gb += blockDim.x) {   // (256 threads for cm's long columns, one wave for cm_raw's mostly short ones)
		const unsigned long long gq = gb + threadIdx.x, first = 16 * gq;
		uint32_t dd[4] = {0, 0, 0, 0}, vv[4] = {0, 0, 0, 0}, inside = 0, n_listed[2] = {0, 0};
		if (gq < g1) {
			uint32_t prev = (first > d && first <= d + len) ? src_rows[s + (first - d) - 1] : 0xFFFFFFFFu;
#pragma unroll
			for (uint32_t b = 0; b < 16; ++b) {
				const unsigned long long g = first + b;
				if (g < d || g >= d + len) continue;
				const unsigned long long t = g - d;
				const uint32_t row = src_rows[s + t], v = src_vals[s + t];
				const uint32_t delta = row - prev;
				prev = row;
				inside |= 1u << b;
				dd[b >> 2] |= (delta >= 255u ? 255u : delta) << (8 * (b & 3u));
				vv[b >> 2] |= (v >= 255u ? 255u : v) << (8 * (b & 3u));
				if (delta >= 255u) { ++n_listed[0]; if (slot_rows) slot_rows[g] = row; }
				if (v >= 255u) { ++n_listed[1]; if (slot_vals) slot_vals[g] = v; }
			}
			if (inside == 0xFFFFu) {
				reinterpret_cast<uint4 *>(dst_delta)[gq] = make_uint4(dd[0], dd[1], dd[2], dd[3]);
				reinterpret_cast<uint4 *>(dst_val)[gq] = make_uint4(vv[0], vv[1], vv[2], vv[3]);
			} else {
#pragma unroll
				for (uint32_t b = 0; b < 16; ++b) if (inside >> b & 1u) { dst_delta[first + b] = uint8_t(dd[b >> 2] >> (8 * (b & 3u))); dst_val[first + b] = uint8_t(vv[b >> 2] >> (8 * (b & 3u))); }
			}
		}
#pragma unroll
		for (uint32_t k = 0; k < 2; ++k) {
			if (!__ballot(n_listed[k] != 0)) continue;
			const uint32_t incl = wave_incl_scan_u32(n_listed[k]);
			const uint32_t total = uint32_t(__shfl(int(incl), 63, 64));
			uint32_t base = 0;
			if (lane == 0) base = atomicAdd(&counters[k], total);
			base = uint32_t(__shfl(int(base), 0, 64));
			uint32_t at = base + incl - n_listed[k];
			if (n_listed[k]) {
				uint32_t *pos = k ? vl_pos : rl_pos, *x = k ? vl_val : rl_row;
				const uint32_t *src = k ? src_vals : src_rows;
#pragma unroll
				for (uint32_t b = 0; b < 16; ++b)
					if ((inside >> b & 1u) && (((k ? vv[b >> 2] : dd[b >> 2]) >> (8 * (b & 3u))) & 0xFFu) == 255u) {
						if (at < cap) { pos[at] = uint32_t(first + b); x[at] = src[s + (first + b - d)]; }
						++at;
					}
			}
		}
	}
}
// cm_raw planned on the device (assemble_raw_device): the shards' real cells, each list ascending by the stream ordinal of the cell's
// first read, merged by rank -- a cell's global column = its local place + the cells of every other shard that come before it.
// which block [off[s], off[s + 1]) of `n` consecutive ones holds index i (an index at or beyond off[n - 1] belongs to the last)
__device__ inline uint32_t block_of(const uint64_t *off, uint32_t n, uint64_t i) {
	uint32_t s = 0;
	while (s + 1 < n && i >= off[s + 1]) ++s;
	return s;
}
struct RawPlanTable { uint32_t world, rank; uint64_t off[64]; uint32_t n[64]; };   // shard s: first[n] at all + off, nnz prefix[n + 1] behind it
struct QueryTable { uint32_t world; uint64_t in_off[65], part_off[64], out_off[65], first_ord[64]; };
__global__ __launch_bounds__(256) void answer_queries_kernel(QueryTable t, const uint32_t *__restrict__ q_in, uint32_t n, const uint32_t *__restrict__ part_idx,
                                                             uint32_t *__restrict__ out) {
	const uint32_t k = blockIdx.x * 256 + threadIdx.x;
	if (k >= n) return;
	out[k] = part_idx[t.part_off[block_of(t.in_off, t.world, k)] + q_in[k]];
}
__global__ __launch_bounds__(256) void ordinals_from_answers_kernel(QueryTable t, const uint32_t *__restrict__ back, uint32_t n, unsigned long long *__restrict__ first) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	first[i] = t.first_ord[block_of(t.out_off, t.world, i)] + back[i];
}
__global__ __launch_bounds__(256) void plan_raw_columns_kernel(RawPlanTable t, const unsigned long long *__restrict__ all, const uint32_t *__restrict__ col_cell,
                                                               const unsigned long long *__restrict__ cell_barcode, uint32_t n,
                                                               unsigned long long *__restrict__ desc, unsigned long long *__restrict__ colptr64,
                                                               uint32_t *__restrict__ colptr32, unsigned long long *__restrict__ barcodes,
                                                               uint32_t *__restrict__ h_begin = nullptr, uint32_t *__restrict__ h_end = nullptr) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const unsigned long long *mine = all + t.off[t.rank], *my_pre = mine + t.n[t.rank];
	const unsigned long long f = mine[i];
	unsigned long long col = i, at = my_pre[i];
	for (uint32_t s = 0; s < t.world; ++s) {
		if (s == t.rank) continue;
		const unsigned long long *fs = all + t.off[s];
		uint32_t lo = 0, hi = t.n[s];
		while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (fs[mid] < f) lo = mid + 1; else hi = mid; }
		col += lo; at += fs[t.n[s] + lo];
	}
	desc[3ull * i] = my_pre[i]; desc[3ull * i + 1] = at; desc[3ull * i + 2] = my_pre[i + 1] - my_pre[i];
	colptr64[col] = at; colptr32[col] = uint32_t(at); barcodes[col] = cell_barcode[col_cell[i]];
	if (h_begin) { h_begin[i] = uint32_t(at); h_end[i] = uint32_t(at + my_pre[i + 1] - my_pre[i]); }   // (pinned: what the host threads that widen this shard's columns walk by)
}
__global__ void copy_words_kernel(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, uint32_t n) { if (threadIdx.x < n) dst[threadIdx.x] = src[threadIdx.x]; }
// local read position -> global stream ordinal: position p came from source rank s = the block [recv_off[s], recv_off[s+1])
// it lies in, as that rank's idx[p]-th resident read
// (every shard's resident reads are ONE contiguous range of the stream and the ranges ascend with the rank: the blocks a
// shard receives, concatenated in source-rank order, are then in stream order, which is what makes a read's POSITION
// on its shard a valid first-seen ordinal there)
struct OrdinalMap { const uint32_t *idx; uint32_t world; uint64_t recv_off[65]; uint64_t first_ord[64]; };
__device__ inline unsigned long long to_global_ordinal(const OrdinalMap &m, uint32_t p) {
	const uint32_t s = block_of(m.recv_off, m.world, p);
	return m.first_ord[s] + (m.idx ? m.idx[p] : p - uint32_t(m.recv_off[s]));
}
__global__ __launch_bounds__(256) void ordinals_kernel(OrdinalMap m, const uint32_t *__restrict__ pos, uint32_t n, unsigned long long *__restrict__ out) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i < n) out[i] = pos[i] == 0xFFFFFFFFu ? ~0ull : to_global_ordinal(m, pos[i]);
}

// -u across shards: smallest global ordinal of every UMI over the shards' tables; then the table becomes a rank table
__global__ __launch_bounds__(256) void min_rows_kernel(const unsigned long long *__restrict__ all, uint32_t rows, uint64_t n, unsigned long long *__restrict__ out) {
	for (uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += uint64_t(gridDim.x) * 256) {
		unsigned long long m = ~0ull;
		for (uint32_t r = 0; r < rows; ++r) { const unsigned long long v = all[uint64_t(r) * n + i]; m = v < m ? v : m; }
		out[i] = m;
	}
}
// rows of `len` bytes gathered by index: out[i] = in[idx[i]] (the quality strings follow the stable partition of their reads)
__global__ __launch_bounds__(256) void gather_byte_rows_kernel(const uint8_t *__restrict__ in, const uint32_t *__restrict__ idx, uint32_t n, uint32_t len,
                                                               uint8_t *__restrict__ out) {
	for (uint64_t k = uint64_t(blockIdx.x) * 256 + threadIdx.x; k < uint64_t(n) * len; k += uint64_t(gridDim.x) * 256) {
		const uint32_t i = uint32_t(k / len), b = uint32_t(k % len);
		out[k] = in[uint64_t(idx[i]) * len + b];
	}
}
// -M across shards: the UMI histograms of the shards added up
__global__ __launch_bounds__(256) void sum_rows_kernel(const uint32_t *__restrict__ all, uint32_t rows, uint64_t n, uint32_t *__restrict__ out) {
	for (uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += uint64_t(gridDim.x) * 256) {
		uint32_t sum = 0;
		for (uint32_t r = 0; r < rows; ++r) sum += all[uint64_t(r) * n + i];
		out[i] = sum;
	}
}
__global__ __launch_bounds__(256) void ranks_to_table_kernel(const unsigned long long *__restrict__ sorted_ord, const uint32_t *__restrict__ code, uint32_t n,
                                                             uint32_t *__restrict__ table) {
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i < n) table[code[i]] = sorted_ord[i] == ~0ull ? 0xFFFFFFFFu : i;
}

}  // namespace dropest
