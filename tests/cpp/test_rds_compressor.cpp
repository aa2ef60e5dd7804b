// The value of test_rds_writer.cpp saved twice: by the default writer, and through Rds::save's compressor overload with a compressor that cuts
// every piece into zlib members of at most 65 280 bytes -- the shape a device compressor writes (tests/test_rds_compressor_cpu.py reads both).
// Host-only.   test_rds_compressor <default.rds> <chunked.rds> <batch_bytes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../dropest_amd/csrc/host/rds_writer.h"

namespace {
struct Chunked : Rds::Compressor {
	size_t batch, calls = 0, pieces_seen = 0;
	explicit Chunked(size_t batch_) : batch(batch_) {}
	size_t batch_bytes() const override { return batch; }
	void compress(const std::vector<std::vector<unsigned char>> &pieces, std::vector<std::vector<unsigned char>> &out) override {
		++calls; pieces_seen += pieces.size();
		out.assign(pieces.size(), {});
		for (size_t k = 0; k < pieces.size(); ++k)
			for (size_t at = 0; at < pieces[k].size(); at += 65280) Rds::gzip_member(pieces[k].data() + at, std::min<size_t>(65280, pieces[k].size() - at), out[k], 4);
	}
};
}  // namespace

int main(int argc, char **argv) {
	if (argc < 4) return 2;
	using namespace Rds;
	const size_t n = 700001;
	std::vector<uint32_t> colptr(1001), rows(n), vals(n);
	for (size_t c = 0; c <= 1000; ++c) colptr[c] = uint32_t(c * n / 1000);
	for (size_t c = 0; c < 1000; ++c) for (uint32_t k = colptr[c]; k < colptr[c + 1]; ++k) { rows[k] = k - colptr[c]; vals[k] = uint32_t((k * 2654435761u) >> 12) + 1u; }
	std::vector<std::string> genes(701), cells(1000), many(300001);
	for (size_t g = 0; g < genes.size(); ++g) genes[g] = "G" + std::to_string(g);
	for (size_t c = 0; c < cells.size(); ++c) cells[c] = "C" + std::to_string(c);
	for (size_t k = 0; k < many.size(); ++k) many[k] = std::string(k % 37, char('A' + k % 4)) + std::to_string(k);
	std::vector<int32_t> ints(1000003);
	std::vector<double> dbl(500009);
	for (size_t k = 0; k < ints.size(); ++k) ints[k] = int32_t(uint32_t(k * 7919u) - 1000000u);
	for (size_t k = 0; k < dbl.size(); ++k) dbl[k] = double(k) * 0.37 - 11.0;
	auto big = [&] {
		std::vector<uint64_t> codes(200003);
		for (size_t k = 0; k < codes.size(); ++k) { const int len = int(k % 32); uint64_t c = len ? 1 : 0; for (int b = 0; b < len; ++b) c = (c << 2) | ((k >> (b % 17)) & 3); codes[k] = c; }
		return named_list({{"cm", dgCMatrix(colptr, rows, vals, genes, cells)}, {"ints", integers(ints)}, {"reals", reals(dbl)}, {"strs", strings(many)},
		                   {"packed", strings_from_packed(codes)}, {"tail", integers({1, 2, 3})}});
	};
	save(big(), argv[1]);
	Chunked chunked(size_t(std::atoll(argv[3])));
	save(big(), argv[2], chunked, 4);
	HostCompressor host(4);
	save(big(), std::string(argv[2]) + ".host", host);
	std::printf("ok calls=%zu pieces=%zu\n", chunked.calls, chunked.pieces_seen);
	return 0;
}
