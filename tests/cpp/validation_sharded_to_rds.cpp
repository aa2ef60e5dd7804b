// validation_sharded_to_rds.cpp -- `dropest -S` through the C++ facade on a SHARDED container (dropest_amd/csrc/host/facade.h): what
// validation_to_rds does, with the container owning the devices of a leading list ("0,0,0": three shards on device 0).  Needs a GPU (run by
// tests/test_gpu_validation_sharded_facade.py).
//   validation_sharded_to_rds <devices> <records.txt> <out.rds> <validation_stats 0|1> <distant pairs> <adjacent pairs> <max_draws> <min genes>
// Prints "truncated <0|1>" and "shards <n>" and exits 0; any error: its text on stderr, exit 1.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>

#include "../../dropest_amd/csrc/host/facade.h"

using namespace Estimation;

int main(int argc, char **argv) {
	if (argc != 9) { std::fprintf(stderr, "usage: %s devices records.txt out.rds validation_stats distant adjacent max_draws min_genes\n", argv[0]); return 2; }
	try {
		std::vector<int> devices;
		{
			std::istringstream list(argv[1]);
			std::string item;
			while (std::getline(list, item, ',')) if (!item.empty()) devices.push_back(std::atoi(item.c_str()));
		}
		if (devices.empty()) throw std::runtime_error("no device in the list");
		const size_t min_genes = size_t(std::atoll(argv[8]));
		CellsDataContainer c(std::make_shared<Merge::DummyMergeStrategy>(min_genes, min_genes), std::make_shared<Merge::UMIs::MergeUMIsStrategySimple>(1),
		                     UMI::Mark::get_by_code(UMI::Mark::DEFAULT_CODE), false, -1, devices);
		std::ifstream in(argv[2]);
		if (!in) throw std::runtime_error(std::string("cannot read ") + argv[2]);
		std::string line, cb, umi, gene;
		while (std::getline(in, line)) {
			std::istringstream fields(line);
			if (!(fields >> cb >> umi >> gene)) continue;
			c.add_record(ReadInfo(Tools::ReadParameters(cb, umi, "", umi), gene, "chr1", UMI::Mark(UMI::Mark::HAS_EXONS)));
		}
		c.set_initialized();
		c.merge_and_filter();
		ResultsPrinter printer(false, false, std::atoi(argv[4]) != 0, false);
		printer.set_validation_sizes(size_t(std::atoll(argv[5])), size_t(std::atoll(argv[6])));
		printer.set_validation_max_draws(uint64_t(std::atoll(argv[7])));
		printer.save_results(c, argv[3]);
		std::printf("truncated %d\nshards %d\n", int(printer.validation_truncated()), c.sharded() ? int(devices.size()) : 1);
		return 0;
	} catch (const std::exception &e) {
		std::fprintf(stderr, "%s\n", e.what());
		return 1;
	}
}
