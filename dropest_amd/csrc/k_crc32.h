// k_crc32.h -- CRC-32 (RFC 1952 8.) of a byte range by one 64-lane wave: shared by the inflate kernels (k_inflate.h, k_inflate_par.h: the
// trailer is checked) and the deflate kernel (k_deflate.h: the trailer is written).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dropest {

// ---- CRC-32 of the inflated block (the gzip trailer's, RFC 1952 8.) ----------------------------------------------------------------
// Every lane takes 1 KB of the block, four bytes per step through four 256-entry tables (LDS, one set per workgroup); the 64 partial values are joined
// in GF(2): crc(A || B) = crc(A) * x^(8 |B|) mod P  xor  crc(B), with x^(2^k) mod P squared up in LDS once per wave (the scheme of zlib's
// crc32_combine).
constexpr uint32_t INF_CRC_POLY = 0xEDB88320u;   // reflected
// x^(2^k) mod P, k = 0 .. 31 (x^1 squared up; checked against zlib.crc32 of concatenations when the constants were made)
__constant__ const uint32_t INF_X2N[32] = {0x40000000u, 0x20000000u, 0x08000000u, 0x00800000u, 0x00008000u, 0xedb88320u, 0xb1e6b092u, 0xa06a2517u,
                                           0xed627daeu, 0x88d14467u, 0xd7bbfe6au, 0xec447f11u, 0x8e7ea170u, 0x6427800eu, 0x4d47bae0u, 0x09fe548fu,
                                           0x83852d0fu, 0x30362f1au, 0x7b5a9cc3u, 0x31fec169u, 0x9fec022au, 0x6c8dedc4u, 0x15d6874du, 0x5fde7a4eu,
                                           0xbad90e37u, 0x2e4e5eefu, 0x4eaba214u, 0xa8a472c0u, 0x429a969eu, 0x148d302au, 0xc40ba6d0u, 0xc4e22c3cu};
__device__ inline uint32_t inf_multmodp(uint32_t a, uint32_t b) {   // a(x) * b(x) mod P, reflected representation (bit 31 = x^0)
	uint32_t m = 1u << 31, p = 0;
	for (;;) {
		if (a & m) { p ^= b; if ((a & (m - 1u)) == 0u) break; }
		m >>= 1;
		b = (b & 1u) ? (b >> 1) ^ INF_CRC_POLY : b >> 1;
	}
	return p;
}
__device__ inline uint32_t inf_x8n(const uint32_t *x2n, uint32_t n_bytes) {   // x^(8 n) mod P
	uint32_t p = 1u << 31, k = 3;
	for (uint32_t n = n_bytes; n; n >>= 1, ++k) if (n & 1u) p = inf_multmodp(x2n[k & 31u], p);
	return p;
}
// crc_tab: [4][256] of the workgroup; x2n: [32] of the wave.  All 64 lanes; returns the CRC-32 of out[0 .. len) in every lane.
// A lane takes ONE 128-byte line per round (a kilobyte per lane re-fetched every line 32 times: + 19 % on the kernel), the 64 values of a
// round of 8 KB are joined pairwise over six levels of shuffles -- the operator of a piece of 128 * 2^d bytes IS x2n[10 + d] -- and the rounds
// one after the other.
__device__ inline uint32_t inf_crc32_block(const uint8_t *out, uint32_t len, const uint32_t *crc_tab, uint32_t *x2n, uint32_t lane) {
	if (lane < 32u) x2n[lane] = INF_X2N[lane];
	uint32_t total = 0;
	for (uint32_t base = 0; base < len; base += 8192u) {
		const uint32_t begin = base + lane * 128u;
		const uint32_t mine = begin < len ? (len - begin < 128u ? len - begin : 128u) : 0u;
		uint32_t c = 0xFFFFFFFFu;
		const uint8_t *p = out + begin;
		uint32_t i = 0;
		for (; i < mine && (uintptr_t(p + i) & 3u); ++i) c = crc_tab[(c ^ p[i]) & 0xFFu] ^ (c >> 8);      // to a word boundary
		auto step4 = [&](uint32_t w) {                                                                   // four bytes per step (slicing by 4)
			c ^= w;
			c = crc_tab[768u + (c & 0xFFu)] ^ crc_tab[512u + ((c >> 8) & 0xFFu)] ^ crc_tab[256u + ((c >> 16) & 0xFFu)] ^ crc_tab[c >> 24];
		};
		for (; i + 32u <= mine; i += 32u) {              // eight words in flight before the chain through the tables waits for any of them
			const uint32_t *q = reinterpret_cast<const uint32_t *>(p + i);
			const uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3], w4 = q[4], w5 = q[5], w6 = q[6], w7 = q[7];
			step4(w0); step4(w1); step4(w2); step4(w3); step4(w4); step4(w5); step4(w6); step4(w7);
		}
		for (; i + 4u <= mine; i += 4u) step4(*reinterpret_cast<const uint32_t *>(p + i));
		for (; i < mine; ++i) c = crc_tab[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
		c = ~c;                                          // (an empty piece: 0)
		uint32_t clen = mine;
#pragma unroll
		for (int d = 0; d < 6; ++d) {
			const uint32_t oc = uint32_t(__shfl_xor(int(c), 1 << d)), ol = uint32_t(__shfl_xor(int(clen), 1 << d));
			if (!(lane & ((2u << d) - 1u))) {            // the left piece (lanes 0, 2^(d+1), ...) takes the right one in
				const uint32_t op = ol == (128u << d) ? x2n[10 + d] : inf_x8n(x2n, ol);
				c = inf_multmodp(op, c) ^ oc;
				clen += ol;
			}
		}
		const uint32_t rc = uint32_t(__shfl(int(c), 0)), rl = uint32_t(__shfl(int(clen), 0));
		total = base ? (inf_multmodp(rl == 8192u ? x2n[16] : inf_x8n(x2n, rl), total) ^ rc) : rc;
	}
	return total;
}

}  // namespace dropest
