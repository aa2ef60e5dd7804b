// BAM file(s) -> <out_base>.rds through the facade, with the .rds deflated by zlib on host threads or, with --device-compression, on the device
// (ResultsPrinter::set_device_compression).  Used by tests/test_gpu_rds_device.py; bam_to_counts.cpp is the full driver.
//   bam_to_rds <out_base> <min_genes_before> <min_genes_after> <threads> [--device-compression] <bam> [<bam> ...]     (barcodes from the CB / UB / GX tags)
#include <cstdio>
#include <cstdlib>
#include "../../dropest_amd/csrc/host/bam_ingest.h"

using namespace Estimation;

int main(int argc, char **argv) {
	if (argc < 6) { std::fprintf(stderr, "usage: %s out_base min_before min_after threads [--device-compression] bam...\n", argv[0]); return 2; }
	try {
		const std::string out = argv[1];
		std::vector<std::string> bams;
		bool device_compression = false;
		for (int a = 5; a < argc; ++a) { if (std::string(argv[a]) == "--device-compression") device_compression = true; else bams.push_back(argv[a]); }
		auto merge = std::make_shared<Merge::DummyMergeStrategy>(size_t(std::atoi(argv[2])), size_t(std::atoi(argv[3])));
		auto umi = std::make_shared<Merge::UMIs::MergeUMIsStrategySimple>(1);
		CellsDataContainer c(merge, umi, UMI::Mark::get_by_code(UMI::Mark::DEFAULT_CODE), false, -1, std::vector<int>{0});
		BamProcessing::BamController ctl(BamProcessing::BamTags(), true, "", "", false, 0, unsigned(std::atoi(argv[4])));
		ctl.parse_bam_files(bams, c);
		c.set_initialized();
		c.merge_and_filter();
		ResultsPrinter printer(false, false);
		printer.set_device_compression(device_compression, 0);
		printer.save_results(c, out + ".rds");
		if (!printer.device_compression_error().empty()) std::fprintf(stderr, "device compression: %s\n", printer.device_compression_error().c_str());
		std::printf("{\"saved\": %zu}\n", ctl.counters().saved);
	} catch (const std::exception &e) {
		std::fprintf(stderr, "ERROR: %s\n", e.what());
		return 1;
	}
	return 0;
}
