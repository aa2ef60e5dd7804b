// bgzf_blocks.h -- where the BGZF blocks of a BAM file are (SAMv1 §4.1): one parse of a block's header, and the walks over it that the host
// reader (bam_ingest.cpp) and the device path (bam_device.cpp) make.  Host-only, no library behind it: the walks differ in what they take
// for an error and say so themselves; the header is read in one place.  Also the walk of the C-ABI (scan_blocks: dropest_bgzf_scan) and the block
// table of the device decoder (BlockTable), which csrc/bgzf_api.hip includes from here.  Nothing here reads the environment.
#pragma once

#include <unistd.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <future>
#include <stdexcept>
#include <string>
#include <vector>

namespace Estimation {
namespace BamProcessing {
namespace bgzf {

inline uint16_t le16(const uint8_t *p) { return uint16_t(p[0] | (p[1] << 8)); }
inline uint32_t le32(const uint8_t *p) { return uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24); }

// A block's header: gzip member, FEXTRA with subfield 'B','C' = total block size - 1.  The last BC subfield of length 2 counts.
struct Header {
	bool magic_ok = false;          // 31, 139, deflate, FEXTRA
	bool header_complete = false;   // the 12 fixed bytes and the XLEN extra bytes lie within what was given
	size_t xlen = 0;
	size_t bsize = 0;               // the whole block's bytes; 0: no BC subfield
	size_t bsize_cut = 0;           // ... counting a BC subfield whose two bytes lie beyond XLEN as well (the window-size probe alone takes it)
};
// h[0 .. n): reads nothing beyond n; with n < 12 nothing at all (magic_ok stays false)
inline Header parse_header(const uint8_t *h, size_t n) {
	Header r;
	if (n < 12) return r;
	r.magic_ok = h[0] == 31 && h[1] == 139 && h[2] == 8 && (h[3] & 4);
	r.xlen = le16(h + 10);
	r.header_complete = n >= 12 + r.xlen;
	for (size_t x = 0; x + 4 <= r.xlen && 12 + x + 6 <= n;) {
		const uint8_t *sf = h + 12 + x;
		const size_t sl = le16(sf + 2);
		if (sf[0] == 'B' && sf[1] == 'C' && sl == 2) { r.bsize_cut = size_t(le16(sf + 4)) + 1; if (x + 6 <= r.xlen) r.bsize = r.bsize_cut; }
		x += 4 + sl;
	}
	return r;
}

struct RawBlock { const uint8_t *cdata = nullptr; size_t clen = 0; uint32_t isize = 0, crc = 0; };

// one BGZF block of a MAPPED file: a block is described in place (header walk only), the inflating workers read the compressed bytes straight
// from the page cache -- a serial fread of every block into a vector of its own capped the reader at ~2 GB/s of BAM whatever the thread count.
// (the only walk that throws, and the only one that names a payload of negative length)
inline bool read_block(const uint8_t *map, size_t size, size_t &at, RawBlock &b, const std::string &path) {
	if (at >= size) return false;
	const Header hd = parse_header(map + at, size - at);
	if (!hd.magic_ok) throw std::runtime_error("Not a BGZF/BAM file: " + path);
	if (!hd.header_complete) throw std::runtime_error("Truncated BGZF header: " + path);
	if (!hd.bsize) throw std::runtime_error("BGZF block without BC subfield: " + path);
	const long clen = long(hd.bsize) - long(hd.xlen) - 20;
	if (clen < 0) throw std::runtime_error("Corrupt BGZF block size: " + path);
	if (size - at < size_t(12) + hd.xlen + size_t(clen) + 8) throw std::runtime_error("Truncated BGZF block: " + path);
	b.cdata = map + at + 12 + hd.xlen; b.clen = size_t(clen);
	const uint8_t *tail = b.cdata + clen;
	b.crc = le32(tail); b.isize = le32(tail + 4);
	at += size_t(12) + hd.xlen + size_t(clen) + 8;
	return true;
}

// whole blocks of p[0 .. got): up to `want` bytes of them (at least one), and no more than the device inflates at once (block_cap)
// (laxer than walk_blocks: a BC size below the block's own header and trailer, and any ISIZE, pass here)
inline size_t whole_blocks(const uint8_t *p, size_t got, size_t want, size_t block_cap, std::string &error) {
	size_t o = 0, n_blocks = 0;
	while (o + 18 <= got && (o < want || o == 0) && n_blocks < block_cap) {
		const Header hd = parse_header(p + o, got - o);
		if (!hd.magic_ok) { error = "Not a BGZF/BAM file"; return 0; }
		if (!hd.header_complete) break;
		if (!hd.bsize) { error = "BGZF block without BC subfield"; return 0; }
		if (o + hd.bsize > got) break;
		o += hd.bsize; ++n_blocks;
	}
	if (!o && got) error = "Truncated BGZF block";
	return o;
}

// the block table the inflate kernel takes (offsets relative to the window)
struct Blocks {
	std::vector<uint64_t> in_off; std::vector<uint32_t> in_len, out_len, crc;
	void clear() { in_off.clear(); in_len.clear(); out_len.clear(); crc.clear(); }
	void append(const Blocks &o) {
		in_off.insert(in_off.end(), o.in_off.begin(), o.in_off.end()); in_len.insert(in_len.end(), o.in_len.begin(), o.in_len.end());
		out_len.insert(out_len.end(), o.out_len.begin(), o.out_len.end()); crc.insert(crc.end(), o.crc.begin(), o.crc.end());
	}
};

// The walk of the C-ABI (dropest_bgzf_scan) over data[0 .. len): whole, sound blocks into the caller's arrays (crc may be null), at most cap of
// them; a block that is cut off ends the walk without a word.  Returns what is wrong ("": nothing), and writes n / used / total only then.
// (as strict as walk_blocks, and the only walk that says where: the offset of the block's first byte)
inline std::string scan_blocks(const uint8_t *data, uint64_t len, uint64_t cap, uint64_t *in_off, uint32_t *in_len, uint64_t *out_off, uint32_t *out_len,
                               uint32_t *crc, uint64_t &n_blocks, uint64_t &used, uint64_t &out_total) {
	uint64_t at = 0, n = 0, total = 0;
	while (n < cap && at + 18 <= len) {
		const Header hd = parse_header(data + at, size_t(len - at));
		if (!hd.magic_ok) return "not a BGZF block header at offset " + std::to_string(at);
		if (!hd.header_complete) break;
		if (!hd.bsize || hd.bsize < 12 + hd.xlen + 8) return "BGZF block without a BC subfield at offset " + std::to_string(at);
		if (at + hd.bsize > len) break;
		const uint8_t *const tail = data + at + hd.bsize - 8;
		in_off[n] = at + 12 + hd.xlen; in_len[n] = uint32_t(hd.bsize - 12 - hd.xlen - 8);
		out_off[n] = total; out_len[n] = le32(tail + 4);
		if (out_len[n] > 65536u) return "BGZF block with ISIZE beyond 64 KB at offset " + std::to_string(at);
		if (crc) crc[n] = le32(tail);
		total += out_len[n];
		at += hd.bsize; ++n;
	}
	n_blocks = n; used = at; out_total = total;
	return std::string();
}

// The block table of a window as the device's inflate and the host fall-back take it: five arrays of one capacity (kept from window to window),
// offsets in relative to the window's compressed bytes, offsets out to its inflated ones.
struct BlockTable {
	std::vector<uint64_t> in_off, out_off; std::vector<uint32_t> in_len, out_len, crc;
	uint64_t n = 0, used = 0, total = 0;
	bool ok = false;
	std::string error;      // !ok: what scan_blocks said

	void grow(uint64_t cap) {
		if (in_off.size() >= cap) return;
		const uint64_t c2 = cap + cap / 2;
		in_off.resize(c2); out_off.resize(c2); in_len.resize(c2); out_len.resize(c2); crc.resize(c2);
	}
	void swap(BlockTable &o) {
		in_off.swap(o.in_off); out_off.swap(o.out_off); in_len.swap(o.in_len); out_len.swap(o.out_len); crc.swap(o.crc);
		std::swap(n, o.n); std::swap(used, o.used); std::swap(total, o.total); std::swap(ok, o.ok); error.swap(o.error);
	}
	// comp[0 .. len) walked from block header to block header.  !ok: not whole, sound blocks
	bool fill(const uint8_t *comp, uint64_t len) {
		// counted first: arrays for the smallest possible block, 26 bytes, would be 36 MB of page faults per 32 MB window
		uint64_t cap = 1;
		for (uint64_t at = 0; at + 18 <= len; ++cap) {
			const Header hd = parse_header(comp + at, size_t(len - at));
			if (!hd.magic_ok || !hd.bsize) break;                      // (scan_blocks says what is wrong)
			at += hd.bsize;
		}
		grow(cap);
		n = used = total = 0;
		error = len ? scan_blocks(comp, len, cap, in_off.data(), in_len.data(), out_off.data(), out_len.data(), crc.data(), n, used, total) : std::string();
		return ok = error.empty();
	}
	// A table the caller made while it read the file (block k: payload at c_in_off[k], c_in_len[k] bytes, ISIZE c_out_len[k], CRC-32 c_crc[k]),
	// checked for what the kernel relies on: blocks in order with room for a header in front of each, the last one ending at len, no ISIZE beyond
	// 64 KB.  A table that is not given (a null array, no block) or not sound: the walk over host[0 .. len) decides.
	bool fill(uint64_t c_n, const uint64_t *c_in_off, const uint32_t *c_in_len, const uint32_t *c_out_len, const uint32_t *c_crc, const uint8_t *host, uint64_t len) {
		ok = false;
		if (c_n && c_in_off && c_in_len && c_out_len && c_crc) {
			grow(c_n);
			uint64_t sum = 0, at = 0;
			bool sound = true;
			for (uint64_t k = 0; k < c_n && sound; ++k) {
				sound = c_in_off[k] >= at + 18 && c_in_off[k] + c_in_len[k] + 8 <= len && c_out_len[k] <= 65536u;
				in_off[k] = c_in_off[k]; in_len[k] = c_in_len[k]; out_off[k] = sum; out_len[k] = c_out_len[k]; crc[k] = c_crc[k];
				sum += c_out_len[k]; at = c_in_off[k] + c_in_len[k] + 8;
			}
			if (sound && at == len) { n = c_n; used = len; total = sum; error.clear(); return ok = true; }
		}
		return fill(host, len);
	}
};

// The same from the file itself, one pread per block (the eight bytes that end a block and the header of the next), with the block table the
// inflate kernel takes as a by-product -- the mapped file is then not touched at all (walking it there mapped half a million pages of a
// 683 MB file, 38 ms to unmap when the file was done).  One window of a file: offsets are relative to file_at.
struct FileWalk {
	int fd = -1;
	size_t file_at = 0;                        // where the window begins in the file
	size_t block_cap = size_t(-1);             // blocks the device takes at once
	size_t avg_block = size_t(1) << 14;        // what a block of this file is expected to take
	size_t least_bytes = size_t(8) << 20, least_blocks = 8192;   // a span below either goes to one walker
	bool one_walker = false;

	bool get(uint8_t *to, size_t off, size_t n) const {
		size_t g = 0;
		while (g < n) { const ssize_t r = pread(fd, to + g, n - g, off_t(file_at + off + g)); if (r <= 0) return false; g += size_t(r); }
		return true;
	}
	// blocks from offset `from` of the window (a block's first byte) until one begins at or behind `until` (and at least one), none beyond `avail`,
	// at most max_blocks; their table appended to B (offsets relative to the window); returns where it stopped
	// (the strictest walk: the only one that rejects a BC size below header + trailer and an ISIZE beyond 64 KB)
	size_t walk_blocks(size_t from, size_t until, size_t avail, size_t max_blocks, Blocks &B, std::string &error) const {
		uint8_t hb[8 + 64];
		std::vector<uint8_t> big;
		size_t o = from, n_blocks = 0, h_len = std::min<size_t>(avail - from, 64);
		if (!get(hb + 8, from, h_len)) { error = "Can't read BAM file"; return from; }
		while (o + 18 <= avail && (o < until || o == from) && n_blocks < max_blocks) {
			if (h_len < 18) break;
			Header hd = parse_header(hb + 8, h_len);
			if (!hd.magic_ok) { error = "Not a BGZF/BAM file"; return from; }
			const size_t xlen = hd.xlen;
			if (o + 12 + xlen > avail) break;
			if (!hd.header_complete) {      // (an extra field beyond the 52 bytes read ahead: never from htslib)
				big.resize(12 + xlen);
				if (!get(big.data(), o, 12 + xlen)) { error = "Can't read BAM file"; return from; }
				hd = parse_header(big.data(), big.size());
			}
			const size_t bsize = hd.bsize;
			if (!bsize || bsize < 12 + xlen + 8) { error = "BGZF block without BC subfield"; return from; }
			if (o + bsize > avail) break;
			const size_t t_off = o + bsize - 8, t_len = std::min<size_t>(avail - t_off, sizeof(hb));
			if (!get(hb, t_off, t_len)) { error = "Can't read BAM file"; return from; }
			const uint32_t isize = le32(hb + 4);
			if (isize > 65536u) { error = "BGZF block with ISIZE beyond 64 KB"; return from; }
			B.in_off.push_back(o + 12 + xlen); B.in_len.push_back(uint32_t(bsize - 12 - xlen - 8)); B.out_len.push_back(isize); B.crc.push_back(le32(hb));
			o += bsize; ++n_blocks;
			h_len = t_len - 8;
		}
		return o;
	}
	// The first block that begins at or behind `from`, found by its first sixteen bytes as htslib and bgzip write them (gzip magic, FEXTRA, XLEN 6,
	// the BC subfield of two bytes) and by the block behind it beginning the same way; size_t(-1): none in the next 64 KB + (not such a file)
	size_t find_block(size_t from, size_t avail) const {
		static const uint8_t magic[16] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0};
		if (from + 64 >= avail) return size_t(-1);
		std::vector<uint8_t> buf(std::min<size_t>(avail - from, (size_t(1) << 16) + 32));
		if (!get(buf.data(), from, buf.size())) return size_t(-1);
		for (size_t i = 0; i + 18 <= buf.size(); ++i) {
			if (buf[i] != 31 || std::memcmp(buf.data() + i, magic, 16)) continue;
			const size_t bsize = size_t(le16(buf.data() + i + 16)) + 1, next = from + i + bsize;
			if (bsize < 26 || next + 16 > avail) continue;
			uint8_t nb[16];
			if (!get(nb, next, 16)) return size_t(-1);
			if (!std::memcmp(nb, magic, 16)) return from + i;
		}
		return size_t(-1);
	}
	// The whole blocks of a window and their table.  A walk from header to header is one pread per block (~0.7 us): 270 000 blocks of a
	// 1.6 GB file of 6 KB blocks are 0.2 s on one thread -- more than the device needs for the file -- so a long window is cut into four
	// stretches, each begun at a block found by its magic bytes; the stretches must meet (a stretch ends where the next one began), else
	// one walk from the start decides.  *stretched: the table came from the four stretches.
	size_t whole_blocks_of_file(size_t avail, size_t want, Blocks &B, std::string &error, bool *stretched = nullptr) const {
		B.clear();
		if (stretched) *stretched = false;
		constexpr size_t STRETCHES = 4;
		// (no further than the blocks the device takes at once are expected to reach: beyond that the stretches' blocks would be thrown away)
		const size_t reach = block_cap == size_t(-1) ? want : std::min<size_t>(want, size_t(double(block_cap) * double(avg_block) * 0.9));
		const size_t span = std::min(reach, avail);
		if (span >= least_bytes && span / avg_block >= least_blocks && !one_walker) {      // (measured: files of 6 KB blocks 213-250 -> 196-200 ms for 64 M reads; windows of fewer, larger blocks the same or a little slower)
			Blocks part[STRETCHES];
			size_t begin[STRETCHES], end[STRETCHES];
			std::string err[STRETCHES];
			std::vector<std::future<void>> th;
			bool found = true;
			begin[0] = 0;
			for (size_t k = 1; k < STRETCHES && found; ++k) { begin[k] = find_block(span / STRETCHES * k, avail); found = begin[k] != size_t(-1); }
			if (found) {
				auto stretch = [&](size_t k) { end[k] = walk_blocks(begin[k], k + 1 < STRETCHES ? span / STRETCHES * (k + 1) : reach, avail, size_t(-1), part[k], err[k]); };
				for (size_t k = 1; k < STRETCHES; ++k) th.push_back(std::async(std::launch::async, stretch, k));
				stretch(0);
				for (auto &f : th) f.get();
				bool meet = true;
				for (size_t k = 0; k < STRETCHES; ++k) meet = meet && err[k].empty() && (k + 1 == STRETCHES || end[k] == begin[k + 1]);
				size_t total = 0;
				for (size_t k = 0; k < STRETCHES; ++k) total += part[k].in_off.size();
				if (meet && total && total <= block_cap) {
					for (size_t k = 0; k < STRETCHES; ++k) B.append(part[k]);
					if (stretched) *stretched = true;
					return end[STRETCHES - 1];
				}
			}
			B.clear();
		}
		const size_t o = walk_blocks(0, want, avail, block_cap, B, error);
		if (!error.empty()) return 0;
		if (!o && avail) error = "Truncated BGZF block";
		return o;
	}
};

}  // namespace bgzf
}  // namespace BamProcessing
}  // namespace Estimation
