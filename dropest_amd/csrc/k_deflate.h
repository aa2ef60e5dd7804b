// k_deflate.h -- BGZF blocks written on the device: raw DEFLATE (RFC 1951) inside gzip members with the BC field (RFC 1952, SAMv1 §4.1).
//
// What it is for: the last host stage of BAM -> .rds.  Rds::save cuts the serialisation into pieces and deflates them with zlib on host threads;
// a .rds body is a sequence of gzip members, and a BGZF block is a gzip member, so the device writes BGZF and any gzip reader takes it.
//
// The input is cut into chunks of at most DFL_CHUNK = 65 280 bytes (htslib's block size: a stored block then always fits a BGZF block) and ONE
// 64-LANE WAVE (a workgroup of its own) takes one chunk.  Why a wave and not a workgroup of several: the parse is a chain -- where the next token
// starts depends on the length of this one -- so one chunk has work for 64 lanes at a time (the candidates of ONE position), not for 256, and
// a wave needs no workgroup barrier between its steps.  The chunks are the parallel axis: a 256 MB input is 4 113 chunks.
//   1. Parse (greedy LZ77): at position p lane k < 63 tries the fixed distance DFL_DIST(k) -- 1 .. 24, the multiples of 4 to 64, of 8 to 256, of 16 to
//      336: what XDR integers and doubles repeat at -- and lane 63 the last earlier position with the same 4-byte hash (a table of 2 048 heads in
//      LDS).  Every lane compares the bytes themselves, up to 258 of them and never past the chunk's end; the longest match wins, the nearest among
//      equals (a max over len << 16 | 0xFFFF - distance: by value, not by arrival).  The token goes to a list in device memory and into the two
//      histograms (lane 0).  The positions a token covers (the first 64 of them) enter the hash table by atomicMax on position + 1: racing lanes of one
//      step are decided by value.
//   2. Codes: the used symbols are ranked by (count, symbol) by all lanes; lane 0 builds the Huffman tree from the sorted counts with two queues,
//      and takes the number of codes of every length from the tree's internal nodes, root first -- a node deeper than 14 splits the deepest
//      shorter code that is still free instead -- which keeps the code COMPLETE and at most 15 bits long.  The rarest symbols
//      get the longest codes.  A distance alphabet with one used symbol is one code of length 1; one with none is two codes of length 1 (zlib's form).
//   3. Size: the dynamic block's bits are summed from the histograms; a chunk it would not make smaller is written as a stored block, so a
//      member is never longer than chunk + 5 + 26 bytes.
//   4. Emit: 64 tokens per round, a prefix sum of their bit counts, every lane ORs its bits into a zeroed LDS buffer, whole words leave with
//      plain stores.  The code lengths in the header are spelt one by one (no 16 / 17 / 18 runs) under a flat 4-bit code-length code: at most
//      (286 + 30) * 4 + 74 bits = 167 bytes a chunk, 0.26 %.
//   5. CRC-32 of the chunk (k_crc32.h: 64 partial values joined in GF(2)), ISIZE, the 18-byte header.
// Members are written at a fixed stride into a staging buffer; deflate_scan_kernel turns the member sizes into offsets and deflate_copy_kernel
// packs them into the caller's buffer, nothing beyond its capacity.  Integer work, no MFMA.  14.6 KB of LDS a wave (no opt-in needed).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_crc32.h"

namespace dropest {

constexpr uint32_t DFL_CHUNK = 65280;
constexpr uint32_t DFL_STRIDE = 65320;        // staging bytes a member: 2 (so that the payload at + 20 is word-aligned) + 18 + 5 + DFL_CHUNK + 8, rounded up to 8
constexpr uint32_t DFL_PAD = 2;
constexpr uint32_t DFL_HASH_BITS = 11;
constexpr uint32_t DFL_MAX_DIST = 32768, DFL_MAX_LEN = 258, DFL_MIN_LEN = 3;
constexpr uint32_t DFL_TOKEN_MATCH = 0x80000000u;   // token: a literal's byte, or this | length - 3 | (distance - 1) << 8
constexpr uint32_t DFL_EOF_BYTES = 28;

__constant__ const uint8_t DFL_EOF_BLOCK[DFL_EOF_BYTES] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

struct DflHuffTmp {          // what the code builder needs, in the place of the hash table (the parse is over by then)
	uint32_t sfreq[288];     // counts of the used symbols, ascending
	uint32_t iw[288];        // weights of the internal nodes, in the order they were made
	uint16_t ssym[288];      // the used symbols in that order
	uint16_t ip[288];        // parent of an internal node
	uint16_t idepth[288];
	uint32_t cnt[17];        // codes per length
	uint32_t next[17];
};

struct DflLds {
	uint32_t crc_tab[4 * 256];
	uint32_t x2n[32];
	uint32_t lfreq[288], dfreq[32];
	uint16_t lcode[288], dcode[32];      // as they enter the stream: bit-reversed
	uint8_t llen[288], dlen[32];
	uint32_t obuf[104];                  // the bits of one round: at most 31 carried + 64 * 48
	union {
		uint32_t hash[1u << DFL_HASH_BITS];
		DflHuffTmp h;
	};
};

__device__ inline uint32_t dfl_uni(uint32_t v) { return uint32_t(__builtin_amdgcn_readfirstlane(int(v))); }

__device__ inline uint32_t dfl_dist_of_lane(uint32_t lane) {     // lanes 0 .. 62
	return lane < 24u ? lane + 1u : lane < 34u ? 24u + 4u * (lane - 23u) : lane < 58u ? 64u + 8u * (lane - 33u) : 256u + 16u * (lane - 57u);
}
__device__ inline uint32_t dfl_hash4(const uint8_t *p) {
	const uint32_t v = uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24);
	return (v * 2654435761u) >> (32u - DFL_HASH_BITS);
}
// length 3 .. 258 -> symbol, extra bits, their value (RFC 1951 3.2.5)
__device__ inline void dfl_len_symbol(uint32_t len, uint32_t &sym, uint32_t &ebits, uint32_t &eval) {
	if (len == 258u) { sym = 285u; ebits = 0; eval = 0; return; }
	const uint32_t l = len - 3u;
	ebits = l < 8u ? 0u : uint32_t(31 - __clz(int(l))) - 2u;
	sym = 257u + 4u * ebits + (l >> ebits);
	eval = l & ((1u << ebits) - 1u);
}
__device__ inline void dfl_dist_symbol(uint32_t dist, uint32_t &sym, uint32_t &ebits, uint32_t &eval) {
	const uint32_t d = dist - 1u;
	if (d < 4u) { sym = d; ebits = 0; eval = 0; return; }
	ebits = uint32_t(31 - __clz(int(d))) - 1u;
	sym = 2u * ebits + 2u + ((d >> ebits) & 1u);
	eval = d & ((1u << ebits) - 1u);
}
__device__ inline uint32_t dfl_len_extra_of_symbol(uint32_t s) { return s < 265u || s >= 285u ? 0u : (s - 261u) >> 2; }
__device__ inline uint32_t dfl_dist_extra_of_symbol(uint32_t s) { return s < 4u ? 0u : (s - 2u) >> 1; }

__device__ inline uint32_t dfl_wave_max(uint32_t v) {
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) { const uint32_t o = uint32_t(__shfl_xor(int(v), d)); v = o > v ? o : v; }
	return dfl_uni(v);
}
__device__ inline uint32_t dfl_wave_sum(uint32_t v) {
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) v += uint32_t(__shfl_xor(int(v), d));
	return dfl_uni(v);
}

// bytes a[0 .. ) == b[0 .. ), at most `maxlen` of them (both ranges end inside the chunk: maxlen is what is left of it behind a)
__device__ inline uint32_t dfl_match_length(const uint8_t *a, const uint8_t *b, uint32_t maxlen) {
	uint32_t n = 0;
	while (n + 8u <= maxlen) {
		uint32_t x[8], y[8];
#pragma unroll
		for (int k = 0; k < 8; ++k) { x[k] = a[n + k]; y[k] = b[n + k]; }
		uint32_t same = 0;
#pragma unroll
		for (int k = 7; k >= 0; --k) same = x[k] == y[k] ? same + 1u : 0u;      // -> leading equal bytes
		n += same;
		if (same < 8u) return n;
	}
	while (n < maxlen && a[n] == b[n]) ++n;
	return n;
}

// The canonical, complete, length-limited Huffman code of freq[0 .. nsym) (nsym <= 288): len[s] (0 = unused) and the bit-reversed code[s].
// All 64 lanes; returns the number of used symbols.  0 or 1 used symbols: only len is set (0 / 1) and the caller decides the form.
__device__ inline uint32_t dfl_build_code(const uint32_t *freq, uint32_t nsym, uint32_t maxlen, uint16_t *code, uint8_t *len, DflHuffTmp &H, uint32_t lane) {
	uint32_t used = 0;
	for (uint32_t s0 = 0; s0 < nsym; s0 += 64u) {
		const uint32_t s = s0 + lane;
		const uint32_t f = s < nsym ? freq[s] : 0u;
		if (s < nsym) { len[s] = 0; code[s] = 0; }
		used += uint32_t(__popcll(__ballot(f != 0u)));
	}
	used = dfl_uni(used);
	for (uint32_t s = lane; s < nsym; s += 64u) {
		const uint32_t f = freq[s];
		if (!f) continue;
		uint32_t rank = 0;
		for (uint32_t j = 0; j < nsym; ++j) { const uint32_t g = freq[j]; rank += (g != 0u && (g < f || (g == f && j < s))) ? 1u : 0u; }
		H.ssym[rank] = uint16_t(s); H.sfreq[rank] = f;
	}
	__syncthreads();
	if (used == 1u && lane == 0) len[H.ssym[0]] = 1;
	if (used >= 2u && lane == 0) {
		const int n = int(used);
		int li = 0, ii = 0;
		for (int e = 0; e < n - 1; ++e) {            // two queues: the sorted leaves, and the internal nodes (made in ascending weight)
			uint32_t w = 0;
			for (int t = 0; t < 2; ++t) {
				if (li < n && (ii >= e || H.sfreq[li] <= H.iw[ii])) w += H.sfreq[li++];
				else { w += H.iw[ii]; H.ip[ii] = uint16_t(e); ++ii; }
			}
			H.iw[e] = w;
		}
		for (uint32_t l = 0; l <= 16u; ++l) H.cnt[l] = 0;
		H.cnt[1] = 2;                                // the root's two children
		H.idepth[n - 2] = 0;
		for (int node = n - 3; node >= 0; --node) {  // every further internal node turns one code of its depth into two that are one longer
			const uint32_t depth = uint32_t(H.idepth[H.ip[node]]) + 1u;
			H.idepth[node] = uint16_t(depth);
			uint32_t l = depth;
			if (l >= maxlen) { l = maxlen; do { --l; } while (H.cnt[l] == 0u); }
			H.cnt[l] -= 1u; H.cnt[l + 1u] += 2u;
		}
		int at = 0;
		for (uint32_t l = maxlen; l >= 1u; --l) for (uint32_t c = H.cnt[l]; c; --c) len[H.ssym[at++]] = uint8_t(l);
	}
	__syncthreads();
	return used;
}
// codes from lengths (RFC 1951 3.2.2), bit-reversed: they enter the stream most significant bit first
__device__ inline void dfl_assign_codes(const uint8_t *len, uint32_t nsym, uint16_t *code, DflHuffTmp &H, uint32_t lane) {
	if (lane == 0) {
		for (uint32_t l = 0; l <= 16u; ++l) H.cnt[l] = 0;
		for (uint32_t s = 0; s < nsym; ++s) H.cnt[len[s]] += 1u;
		H.cnt[0] = 0;
		uint32_t c = 0;
		for (uint32_t l = 1; l <= 15u; ++l) { c = (c + H.cnt[l - 1u]) << 1; H.next[l] = c; }
		for (uint32_t s = 0; s < nsym; ++s) {
			const uint32_t l = len[s];
			if (l) { const uint32_t v = H.next[l]++; code[s] = uint16_t(__brev(v) >> (32u - l)); }
		}
	}
	__syncthreads();
}

struct DflOut {
	uint32_t *words;     // the payload as aligned words
	uint32_t bitpos;     // bits written so far (the ones above a word boundary wait in obuf[0])
};
// One round: lane k appends the low `nbits` (<= 48) bits of `v`, lane after lane.  All 64 lanes.
__device__ inline void dfl_emit_round(DflOut &o, DflLds &L, uint64_t v, uint32_t nbits, uint32_t lane) {
	uint32_t incl = nbits;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) { const uint32_t up = uint32_t(__shfl_up(int(incl), d)); if (lane >= uint32_t(d)) incl += up; }
	const uint32_t total = dfl_uni(uint32_t(__shfl(int(incl), 63)));
	const uint32_t carried = o.bitpos & 31u;
	const uint32_t at = carried + incl - nbits;
	if (nbits) {
		const uint32_t w = at >> 5, s = at & 31u;
		const uint32_t w0 = uint32_t(v << s), w1 = uint32_t(v >> (32u - s)), w2 = s ? uint32_t(v >> (64u - s)) : 0u;
		if (w0) atomicOr(&L.obuf[w], w0);
		if (w1) atomicOr(&L.obuf[w + 1u], w1);
		if (w2) atomicOr(&L.obuf[w + 2u], w2);
	}
	__syncthreads();
	const uint32_t end = carried + total, full = end >> 5;                 // whole words of this round (<= 97)
	uint32_t *dst = o.words + (o.bitpos >> 5);
	const uint32_t a = lane < full ? L.obuf[lane] : 0u, b = lane + 64u < full ? L.obuf[lane + 64u] : 0u;
	const uint32_t rest = L.obuf[full];
	if (lane < full) dst[lane] = a;
	if (lane + 64u < full) dst[lane + 64u] = b;
	__syncthreads();
	for (uint32_t k = lane; k < 104u; k += 64u) L.obuf[k] = 0;
	__syncthreads();
	if (lane == 0) L.obuf[0] = rest;
	__syncthreads();
	o.bitpos += total;
}

// One wave (= one workgroup of 64 threads) per chunk; block n_chunks, when there is one, writes the BGZF end-of-file block.
__global__ __launch_bounds__(64) void bgzf_deflate_kernel(const uint8_t *__restrict__ d_in, uint64_t len, uint32_t n_chunks, uint8_t *__restrict__ staging,
                                                         uint32_t *__restrict__ tokens, uint32_t *__restrict__ member_len) {
	__shared__ DflLds L;
	const uint32_t lane = threadIdx.x, chunk = blockIdx.x;
	uint8_t *const member = staging + uint64_t(chunk) * DFL_STRIDE + DFL_PAD;
	if (chunk >= n_chunks) {
		if (lane < DFL_EOF_BYTES) member[lane] = DFL_EOF_BLOCK[lane];
		if (lane == 0) member_len[chunk] = DFL_EOF_BYTES;
		return;
	}
	const uint64_t start = uint64_t(chunk) * DFL_CHUNK;
	const uint32_t n = uint32_t(len - start < DFL_CHUNK ? len - start : DFL_CHUNK);
	const uint8_t *const in = d_in + start;
	uint32_t *const tok = tokens + uint64_t(chunk) * DFL_CHUNK;

	for (uint32_t k = lane; k < 256u; k += 64u) {
		uint32_t c = k;
		for (int b = 0; b < 8; ++b) c = (c & 1u) ? (c >> 1) ^ INF_CRC_POLY : c >> 1;
		L.crc_tab[k] = c;
	}
	for (uint32_t k = lane; k < (1u << DFL_HASH_BITS); k += 64u) L.hash[k] = 0;
	for (uint32_t k = lane; k < 288u; k += 64u) L.lfreq[k] = 0;
	if (lane < 32u) L.dfreq[lane] = 0;
	for (uint32_t k = lane; k < 104u; k += 64u) L.obuf[k] = 0;
	__syncthreads();
	for (int t = 1; t < 4; ++t) {
		for (uint32_t k = lane; k < 256u; k += 64u) { const uint32_t c = L.crc_tab[(t - 1) * 256 + k]; L.crc_tab[t * 256 + k] = (c >> 8) ^ L.crc_tab[c & 0xFFu]; }
		__syncthreads();
	}

	// ---- 1. parse ------------------------------------------------------------------------------------------------------------------
	uint32_t n_tok = 0;
	for (uint32_t p = 0; p < n;) {
		const uint32_t left = n - p, maxlen = left < DFL_MAX_LEN ? left : DFL_MAX_LEN;
		uint32_t best = 0;
		if (maxlen >= DFL_MIN_LEN) {
			uint32_t d = 0;
			if (lane < 63u) d = dfl_dist_of_lane(lane);
			else if (left >= 4u) { const uint32_t c = L.hash[dfl_hash4(in + p)]; d = c ? p + 1u - c : 0u; }
			uint32_t score = 0;
			if (d >= 1u && d <= p && d <= DFL_MAX_DIST) {
				const uint32_t ml = dfl_match_length(in + p, in + p - d, maxlen);
				if (ml >= DFL_MIN_LEN) score = (ml << 16) | (0xFFFFu - (d - 1u));
			}
			best = dfl_wave_max(score);
		}
		uint32_t step = 1;
		if (best) {
			const uint32_t ml = best >> 16, d = (0xFFFFu - (best & 0xFFFFu)) + 1u;
			step = ml;
			if (lane == 0) {
				uint32_t ls, le, lv, ds, de, dv;
				dfl_len_symbol(ml, ls, le, lv); dfl_dist_symbol(d, ds, de, dv);
				L.lfreq[ls] += 1u; L.dfreq[ds] += 1u;
				tok[n_tok] = DFL_TOKEN_MATCH | (ml - 3u) | ((d - 1u) << 8);
			}
		} else if (lane == 0) {
			const uint32_t b = in[p];
			L.lfreq[b] += 1u;
			tok[n_tok] = b;
		}
		++n_tok;
		if (lane < step && p + lane + 4u <= n) atomicMax(&L.hash[dfl_hash4(in + p + lane)], p + lane + 1u);
		__syncthreads();
		p += step;
	}
	if (lane == 0) L.lfreq[256] = 1;
	__syncthreads();

	// ---- 2. codes (the hash table's LDS is the builder's from here on) ---------------------------------------------------------------
	dfl_build_code(L.lfreq, 286u, 15u, L.lcode, L.llen, L.h, lane);
	dfl_assign_codes(L.llen, 286u, L.lcode, L.h, lane);
	const uint32_t d_used = dfl_build_code(L.dfreq, 30u, 15u, L.dcode, L.dlen, L.h, lane);
	if (d_used == 0u && lane < 2u) L.dlen[lane] = 1;      // no match in the chunk: two codes of one bit, neither of them used
	__syncthreads();
	dfl_assign_codes(L.dlen, 30u, L.dcode, L.h, lane);
	uint32_t hlit = 0, hdist = 0;
	for (uint32_t s0 = 0; s0 < 320u; s0 += 64u) {
		const uint32_t s = s0 + lane;
		const uint32_t v = dfl_wave_max(s < 286u && L.llen[s] ? s + 1u : 0u);
		hlit = v > hlit ? v : hlit;
	}
	hdist = dfl_wave_max(lane < 30u && L.dlen[lane] ? lane + 1u : 0u);
	hlit = hlit < 257u ? 257u : hlit;

	// ---- 3. size -------------------------------------------------------------------------------------------------------------------
	uint32_t bits = 0;
	for (uint32_t s = lane; s < 286u; s += 64u) bits += L.lfreq[s] * (uint32_t(L.llen[s]) + dfl_len_extra_of_symbol(s));
	if (lane < 30u) bits += L.dfreq[lane] * (uint32_t(L.dlen[lane]) + dfl_dist_extra_of_symbol(lane));
	const uint32_t total_bits = dfl_wave_sum(bits) + 17u + 57u + 4u * (hlit + hdist);
	const uint32_t dyn_bytes = (total_bits + 7u) >> 3;
	const bool stored = dyn_bytes >= n;
	const uint32_t payload = stored ? n + 5u : dyn_bytes;
	uint8_t *const body = member + 18;

	// ---- 4. emit -------------------------------------------------------------------------------------------------------------------
	if (stored) {
		if (lane == 0) { body[0] = 1; body[1] = uint8_t(n); body[2] = uint8_t(n >> 8); body[3] = uint8_t(~n); body[4] = uint8_t((~n) >> 8); }
		for (uint32_t k = lane; k < n; k += 64u) body[5u + k] = in[k];
	} else {
		DflOut o{reinterpret_cast<uint32_t *>(body), 0u};
		{	// BFINAL = 1, BTYPE = 10, HLIT, HDIST, HCLEN = 19; the code-length code: 16 / 17 / 18 unused, 0 .. 15 four bits each
			uint64_t v = 0; uint32_t nb = 0;
			if (lane == 0) { v = 5u | ((hlit - 257u) << 3) | ((hdist - 1u) << 8) | (15u << 13); nb = 17; }
			else if (lane == 1) { v = 0; nb = 9; }
			else if (lane == 2 || lane == 3) { v = 0x924924u; nb = 24; }
			dfl_emit_round(o, L, v, nb, lane);
		}
		for (uint32_t s0 = 0; s0 < hlit + hdist; s0 += 64u) {
			const uint32_t s = s0 + lane;
			uint32_t l = 0, nb = 0;
			if (s < hlit + hdist) { l = s < hlit ? L.llen[s] : L.dlen[s - hlit]; nb = 4; }
			dfl_emit_round(o, L, uint64_t(__brev(l) >> 28), nb, lane);        // symbol l of the flat code = the value l, most significant bit first
		}
		for (uint32_t t0 = 0; t0 < n_tok + 1u; t0 += 64u) {                   // (+ 1: the end-of-block symbol)
			const uint32_t t = t0 + lane;
			uint64_t v = 0; uint32_t nb = 0;
			if (t < n_tok) {
				const uint32_t k = tok[t];
				if (k & DFL_TOKEN_MATCH) {
					uint32_t ls, le, lv, ds, de, dv;
					dfl_len_symbol((k & 0xFFu) + 3u, ls, le, lv); dfl_dist_symbol(((k >> 8) & 0x7FFFu) + 1u, ds, de, dv);
					v = L.lcode[ls]; nb = L.llen[ls];
					v |= uint64_t(lv) << nb; nb += le;
					v |= uint64_t(L.dcode[ds]) << nb; nb += L.dlen[ds];
					v |= uint64_t(dv) << nb; nb += de;
				} else { v = L.lcode[k]; nb = L.llen[k]; }
			} else if (t == n_tok) { v = L.lcode[256]; nb = L.llen[256]; }
			dfl_emit_round(o, L, v, nb, lane);
		}
		if (lane == 0 && (o.bitpos & 31u)) o.words[o.bitpos >> 5] = L.obuf[0];   // (the staging stride leaves room for the whole last word)
		__syncthreads();
	}
	__threadfence();      // the payload's words are through before the trailer's bytes land beside (or on) the last of them

	// ---- 5. header and trailer -----------------------------------------------------------------------------------------------------
	const uint32_t crc = inf_crc32_block(in, n, L.crc_tab, L.x2n, lane);
	const uint32_t size = 18u + payload + 8u;
	if (lane < 16u) member[lane] = DFL_EOF_BLOCK[lane];                         // the same 16 bytes open every BGZF block
	if (lane == 16u) member[16] = uint8_t(size - 1u);
	if (lane == 17u) member[17] = uint8_t((size - 1u) >> 8);
	if (lane < 4u) { body[payload + lane] = uint8_t(crc >> (8u * lane)); body[payload + 4u + lane] = uint8_t(n >> (8u * lane)); }
	if (lane == 0) member_len[chunk] = size;
}

// off[k] = sum of member_len[0 .. k); totals = {members, bytes of the whole stream, 1 if that is more than out_cap}.  One workgroup of 256.
__global__ __launch_bounds__(256) void deflate_scan_kernel(const uint32_t *__restrict__ member_len, uint32_t n, uint64_t *__restrict__ off, uint64_t out_cap,
                                                          uint64_t *__restrict__ totals) {
	__shared__ uint32_t ws[256];
	__shared__ uint64_t carry;
	const uint32_t t = threadIdx.x;
	if (t == 0) carry = 0;
	__syncthreads();
	for (uint32_t base = 0; base < n; base += 256u) {
		const uint32_t v = base + t < n ? member_len[base + t] : 0u;
		ws[t] = v;
		__syncthreads();
		for (uint32_t d = 1; d < 256u; d <<= 1) {
			const uint32_t add = t >= d ? ws[t - d] : 0u;
			__syncthreads();
			ws[t] += add;
			__syncthreads();
		}
		if (base + t < n) off[base + t] = carry + ws[t] - v;
		__syncthreads();
		if (t == 255u) carry += ws[255];
		__syncthreads();
	}
	if (t == 0) { totals[0] = n; totals[1] = carry; totals[2] = carry > out_cap ? 1u : 0u; }
}

// member k from its staging slot to out + off[k]; a member that does not fit below out_cap whole is not written at all
__global__ __launch_bounds__(256) void deflate_copy_kernel(const uint8_t *__restrict__ staging, const uint32_t *__restrict__ member_len, const uint64_t *__restrict__ off,
                                                          uint8_t *__restrict__ out, uint64_t out_cap) {
	const uint32_t k = blockIdx.x, size = member_len[k];
	const uint64_t at = off[k];
	if (at + size > out_cap) return;
	const uint8_t *src = staging + uint64_t(k) * DFL_STRIDE + DFL_PAD;
	for (uint32_t i = threadIdx.x; i < size; i += 256u) out[at + i] = src[i];
}

}  // namespace dropest
