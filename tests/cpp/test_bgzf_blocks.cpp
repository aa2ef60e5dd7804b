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
