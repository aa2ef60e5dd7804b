// validation_to_rds.cpp -- `dropest -S` through the C++ facade (dropest_amd/csrc/host/facade.h): reads records from a text file, one
// "barcode UMI gene" per line, runs the container (no CB merge, the default UMI merge, every mark) and saves the results list with or
// without validation_stats.  Needs a GPU (run by tests/test_gpu_validation_facade.py).
//   validation_to_rds <records.txt> <out.rds> <validation_stats 0|1> <distant pairs> <adjacent pairs> <max_draws> <min genes>
// Prints "truncated <0|1>" and exits 0; any error: its text on stderr, exit 1.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>

#include "../../dropest_amd/csrc/host/facade.h"

using namespace Estimation;

int main(int argc, char **argv) {
	if (argc != 8) { std::fprintf(stderr, "usage: %s records.txt out.rds validation_stats distant adjacent max_draws min_genes\n", argv[0]); return 2; }
	try {
		const size_t min_genes = size_t(std::atoll(argv[7]));
		CellsDataContainer c(std::make_shared<Merge::DummyMergeStrategy>(min_genes, min_genes), std::make_shared<Merge::UMIs::MergeUMIsStrategySimple>(1),
		                     UMI::Mark::get_by_code(UMI::Mark::DEFAULT_CODE));
		std::ifstream in(argv[1]);
		if (!in) throw std::runtime_error(std::string("cannot read ") + argv[1]);
		std::string line, cb, umi, gene;
		while (std::getline(in, line)) {
			std::istringstream fields(line);
			if (!(fields >> cb >> umi >> gene)) continue;
			c.add_record(ReadInfo(Tools::ReadParameters(cb, umi, "", umi), gene, "chr1", UMI::Mark(UMI::Mark::HAS_EXONS)));
		}
		c.set_initialized();
		c.merge_and_filter();
		ResultsPrinter printer(false, false, std::atoi(argv[3]) != 0, false);
		printer.set_validation_sizes(size_t(std::atoll(argv[4])), size_t(std::atoll(argv[5])));
		printer.set_validation_max_draws(uint64_t(std::atoll(argv[6])));
		printer.save_results(c, argv[2]);
		std::printf("truncated %d\n", int(printer.validation_truncated()));
		return 0;
	} catch (const std::exception &e) {
		std::fprintf(stderr, "%s\n", e.what());
		return 1;
	}
}
