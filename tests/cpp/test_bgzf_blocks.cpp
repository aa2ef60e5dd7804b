// test_bgzf_blocks.cpp -- the BGZF block walks of dropest_amd/csrc/host/bgzf_blocks.h on their own (no library): tests/test_bgzf_blocks_cpu.py
// writes the files, gives one command per line of a script and compares the answers with what it reads from the files itself.
//   usage: test_bgzf_blocks FILE SCRIPT        answers on stdout, one line per command: o <tab> stretched <tab> error <tab> table
//   table = "offset,compressed length,ISIZE,CRC;" per block, offset = the file offset of the block's deflate stream
//   rb SIZE FROM                                   read_block over FILE[0 .. SIZE) from FROM until it says false or throws (o = where it stopped)
//   wb SIZE FROM WANT CAP                          whole_blocks(FILE + FROM, SIZE - FROM, WANT, CAP)
//   wbt SIZE FROM                                  whole_blocks with want = 1 again and again: a block per call, the table from the bytes
//   walk FROM START UNTIL AVAIL MAX                FileWalk{file_at = FROM}.walk_blocks(START, UNTIL, AVAIL, MAX)
//   wbf FROM AVAIL WANT CAP AVG BYTES BLOCKS ONE   FileWalk{...}.whole_blocks_of_file(AVAIL, WANT)
//   hdr FROM N                                     parse_header(FILE + FROM, N): magic_ok,header_complete,xlen,bsize,bsize_cut in the error column
//   tab SIZE FROM                                  BlockTable::fill(FILE + FROM, SIZE - FROM): o = used, the stretched column = ok, the error column =
//                                                  the table's error or "n=N,total=T"; the table with a fifth number per block, its offset out
//   cal SIZE FROM HOW                              the same through BlockTable::fill(a caller's table, FILE + FROM, SIZE - FROM): the caller's table is
//                                                  the walk's own with every CRC + 1 (so that a table taken from the caller shows), and HOW spoils it:
//                                                  good | gap (block 1 left out) | overlap (block 1 begins inside block 0) | short (the last block left
//                                                  out) | big (block 1 with ISIZE 65537) | null (no CRC array)
#include "../../dropest_amd/csrc/host/bgzf_blocks.h"

#include <fcntl.h>

#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>

using namespace Estimation::BamProcessing::bgzf;

static std::string table_of(const Blocks &B, size_t base) {
	std::ostringstream s;
	for (size_t k = 0; k < B.in_off.size(); ++k) s << base + B.in_off[k] << ',' << B.in_len[k] << ',' << B.out_len[k] << ',' << B.crc[k] << ';';
	return s.str();
}
static void answer_of(const BlockTable &T, size_t base, size_t &o, bool &ok, std::string &error, std::string &table) {
	std::ostringstream s, e;
	for (size_t k = 0; k < T.n; ++k) s << base + T.in_off[k] << ',' << T.in_len[k] << ',' << T.out_len[k] << ',' << T.crc[k] << ',' << T.out_off[k] << ';';
	e << "n=" << T.n << ",total=" << T.total;
	o = T.used; ok = T.ok; error = T.ok ? e.str() : T.error; table = s.str();
}
static size_t num(std::istream &in) { long long v = 0; in >> v; return v < 0 ? size_t(-1) : size_t(v); }

int main(int argc, char **argv) {
	if (argc != 3) return 2;
	std::ifstream f(argv[1], std::ios::binary);
	const std::string bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
	const int fd = open(argv[1], O_RDONLY);
	if (!f || fd < 0) return 2;
	std::ifstream script(argv[2]);
	std::string line;
	while (std::getline(script, line)) {
		std::istringstream in(line);
		std::string cmd, error, table;
		size_t o = 0;
		bool stretched = false;
		in >> cmd;
		if (cmd == "rb" || cmd == "wb" || cmd == "wbt") {
			// (a copy of exactly SIZE bytes: a read beyond the prefix is the sanitizer's to see)
			const size_t size = num(in), from = num(in);
			std::vector<uint8_t> copy(bytes.begin(), bytes.begin() + size);
			Blocks B;
			if (cmd == "rb") {
				o = from;
				RawBlock b;
				try { while (read_block(copy.data(), size, o, b, "FILE")) { B.in_off.push_back(size_t(b.cdata - copy.data())); B.in_len.push_back(uint32_t(b.clen)); B.out_len.push_back(b.isize); B.crc.push_back(b.crc); } }
				catch (const std::exception &e) { error = e.what(); }
			} else if (cmd == "wb") {
				const size_t want = num(in), cap = num(in);
				o = whole_blocks(copy.data() + from, size - from, want, cap, error);
			} else
				for (size_t at = from;;) {
					const size_t len = whole_blocks(copy.data() + at, size - at, 1, size_t(-1), error);
					if (!len) break;
					const Header hd = parse_header(copy.data() + at, size - at);
					B.in_off.push_back(at + 12 + hd.xlen); B.in_len.push_back(uint32_t(len - 12 - hd.xlen - 8)); B.out_len.push_back(le32(copy.data() + at + len - 4)); B.crc.push_back(le32(copy.data() + at + len - 8));
					o = at += len;
				}
			table = table_of(B, 0);
		} else if (cmd == "walk" || cmd == "wbf") {
			FileWalk w;
			w.fd = fd; w.file_at = num(in);
			Blocks B;
			if (cmd == "walk") {
				const size_t start = num(in), until = num(in), avail = num(in), max_blocks = num(in);
				o = w.walk_blocks(start, until, avail, max_blocks, B, error);
			} else {
				const size_t avail = num(in), want = num(in);
				w.block_cap = num(in); w.avg_block = num(in); w.least_bytes = num(in); w.least_blocks = num(in); w.one_walker = num(in) != 0;
				o = w.whole_blocks_of_file(avail, want, B, error, &stretched);
			}
			table = table_of(B, w.file_at);
		} else if (cmd == "tab" || cmd == "cal") {
			const size_t size = num(in), from = num(in);
			std::vector<uint8_t> copy(bytes.begin() + from, bytes.begin() + size);      // (exactly the bytes given: a read beyond them is the sanitizer's to see)
			BlockTable T;
			T.n = T.used = T.total = 77;      // (what a table kept from the window before holds)
			if (cmd == "tab") T.fill(copy.data(), copy.size());
			else {
				std::string how;
				in >> how;
				BlockTable W;
				if (!W.fill(copy.data(), copy.size()) || W.n < 3) return 2;
				std::vector<uint64_t> c_off(W.in_off.begin(), W.in_off.begin() + W.n);
				std::vector<uint32_t> c_len(W.in_len.begin(), W.in_len.begin() + W.n), c_out(W.out_len.begin(), W.out_len.begin() + W.n), c_crc(W.crc.begin(), W.crc.begin() + W.n);
				for (uint32_t &c : c_crc) c += 1;
				auto drop = [&](size_t k) { c_off.erase(c_off.begin() + k); c_len.erase(c_len.begin() + k); c_out.erase(c_out.begin() + k); c_crc.erase(c_crc.begin() + k); };
				if (how == "gap") drop(1);
				else if (how == "overlap") { c_off[1] = c_off[0] + c_len[0] + 8 + 17; c_len[1] += 1; }      // (one byte short of the room a header takes; the block still ends where it did)
				else if (how == "short") drop(c_off.size() - 1);
				else if (how == "big") c_out[1] = 65537;
				else if (how != "good" && how != "null") return 2;
				T.fill(c_off.size(), c_off.data(), c_len.data(), c_out.data(), how == "null" ? nullptr : c_crc.data(), copy.data(), copy.size());
			}
			answer_of(T, from, o, stretched, error, table);
		} else if (cmd == "hdr") {
			const size_t from = num(in), n = num(in);
			std::vector<uint8_t> copy(bytes.begin() + from, bytes.begin() + from + n);
			const Header hd = parse_header(copy.data(), n);
			std::ostringstream s;
			s << hd.magic_ok << ',' << hd.header_complete << ',' << hd.xlen << ',' << hd.bsize << ',' << hd.bsize_cut;
			error = s.str();
		} else return 2;
		std::cout << o << '\t' << stretched << '\t' << error << '\t' << table << '\n';
	}
	return 0;
}
