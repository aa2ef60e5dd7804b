// read_corrections_dump.cpp -- `dropest -F`, the decisions, through the C++ facade (dropest_amd/csrc/host/facade.h) on a container of one
// device or sharded over a device list ("0,0,0": three shards on device 0).  Needs a GPU (run by tests/test_gpu_facade_read_corrections_sharded.py).
//   read_corrections_dump <devices> <records.txt> <whitelist file | -> <min genes before> <min genes after> <out.txt>
// records.txt: "<barcode> <UMI> <gene | ->" per read.  With a whitelist the barcodes are merged by RealBarcodesMergeStrategy (constant length).
// out.txt: "<verdict> <target barcode code> <corrected UMI code>" per read, in the order of the records.  Prints "shards <n>" and exits 0; any
// error: its text on stderr, exit 1.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>

#include "../../dropest_amd/csrc/host/facade.h"

using namespace Estimation;

int main(int argc, char **argv) {
	if (argc != 7) { std::fprintf(stderr, "usage: %s devices records.txt whitelist|- min_before min_after out.txt\n", argv[0]); return 2; }
	try {
		std::vector<int> devices;
		{
			std::istringstream list(argv[1]);
			std::string item;
			while (std::getline(list, item, ',')) if (!item.empty()) devices.push_back(std::atoi(item.c_str()));
		}
		if (devices.empty()) throw std::runtime_error("no device in the list");
		const size_t before = size_t(std::atoll(argv[4])), after = size_t(std::atoll(argv[5]));
		std::shared_ptr<Merge::MergeStrategyAbstract> merge;
		if (std::string(argv[3]) == "-") merge = std::make_shared<Merge::DummyMergeStrategy>(before, after);
		else merge = std::make_shared<Merge::RealBarcodesMergeStrategy>(Merge::RealBarcodesMergeStrategy::CONST_LENGTH, argv[3], before, after, 2, 0.2);
		CellsDataContainer c(merge, std::make_shared<Merge::UMIs::MergeUMIsStrategySimple>(1), UMI::Mark::get_by_code(UMI::Mark::DEFAULT_CODE),
		                     /*save_umi_merge_targets=*/true, -1, devices);
		std::ifstream in(argv[2]);
		if (!in) throw std::runtime_error(std::string("cannot read ") + argv[2]);
		std::string line, cb, umi, gene;
		uint64_t n = 0;
		while (std::getline(in, line)) {
			std::istringstream fields(line);
			if (!(fields >> cb >> umi >> gene)) continue;
			const bool has_gene = gene != "-";
			c.add_record(ReadInfo(Tools::ReadParameters(cb, umi, "", umi), has_gene ? gene : "", "chr1", has_gene ? UMI::Mark(UMI::Mark::HAS_EXONS) : UMI::Mark()));
			++n;
		}
		c.set_initialized();
		c.merge_and_filter();
		std::vector<uint8_t> verdict(n);
		std::vector<uint64_t> barcode(n), corrected(n);
		c.read_corrections_host(0, n, verdict.data(), barcode.data(), corrected.data());
		std::ofstream out(argv[6]);
		for (uint64_t i = 0; i < n; ++i) out << int(verdict[i]) << ' ' << barcode[i] << ' ' << corrected[i] << '\n';
		if (!out) throw std::runtime_error(std::string("cannot write ") + argv[6]);
		std::printf("shards %d\n", c.sharded() ? int(devices.size()) : 1);
		return 0;
	} catch (const std::exception &e) {
		std::fprintf(stderr, "%s\n", e.what());
		return 1;
	}
}
