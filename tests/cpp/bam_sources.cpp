// BAM file(s) -> .rds under the two sources the device BAM path takes only behind BamController::set_device_read_sources: -r read-parameter
// files and -P gene = chromosome name (tests/test_gpu_bam_device_sources.py; scripts/bench_bam_params.py).  Like bam_to_counts, plus:
//   bam_sources <out_base> <filled|name|params:files> <chromosome gene 0|1> <device sources 0|1[b|F]> <min_genes_before> <min_genes_after>
//               <whitelist|-> <threads> <devices|-> <quota|0> <bam> [<bam> ...]
//   device sources: the switch; a letter behind it asks for output as well -- b: parse_bam_files(files, true, container), F: write_filtered_bam_files
//   after the estimate (both are refused under -r and -P whatever the switch says).  devices: "0,0,0" shards the container; quota > 0: set_shard_quota.
//   environment: DROPEST_GTF, DROPEST_MIN_PHRED, DROPEST_RPUPC as for bam_to_counts; DROPEST_BAM_DEVICE = 1 and the rest of what BamController reads.
//   Prints the counters as one JSON line.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include "../../dropest_amd/csrc/host/bam_ingest.h"

using namespace Estimation;

int main(int argc, char **argv) {
	if (argc < 12) { std::fprintf(stderr, "usage: %s out_base filled|name|params:files chromosome_gene device_sources min_before min_after whitelist|- threads devices|- quota bam...\n", argv[0]); return 2; }
	try {
		const std::string out = argv[1], mode = argv[2], sources = argv[4], wl = argv[7], dev = argv[9];
		const bool chromosome_gene = std::atoi(argv[3]) != 0, device_sources = sources[0] == '1';
		const char output = sources.size() > 1 ? sources[1] : ' ';
		const size_t min_before = size_t(std::atoi(argv[5])), min_after = size_t(std::atoi(argv[6])), quota = size_t(std::atoll(argv[10]));
		const unsigned threads = unsigned(std::atoi(argv[8]));
		std::vector<std::string> bams(argv + 11, argv + argc);
		std::shared_ptr<Merge::MergeStrategyAbstract> merge;
		if (wl == "-") merge = std::make_shared<Merge::DummyMergeStrategy>(min_before, min_after);
		else merge = std::make_shared<Merge::RealBarcodesMergeStrategy>(Merge::RealBarcodesMergeStrategy::CONST_LENGTH, wl, min_before, min_after, 7, 0.2);
		auto umi = std::make_shared<Merge::UMIs::MergeUMIsStrategySimple>(1);
		std::vector<int> devices;
		if (dev != "-") { size_t at = 0; while (at < dev.size()) { devices.push_back(std::atoi(dev.c_str() + at)); at = dev.find(',', at); if (at == std::string::npos) break; ++at; } }
		if (devices.empty()) devices.push_back(0);
		CellsDataContainer c(merge, umi, UMI::Mark::get_by_code(UMI::Mark::DEFAULT_CODE), false, -1, devices);
		if (quota && c.sharded()) c.set_shard_quota(quota);
		BamProcessing::BamTags tags;
		tags.read_type = "RE"; tags.intronic_read_value = "N"; tags.intergenic_read_value = "I"; tags.exonic_read_value = "E";
		const char *gtf = std::getenv("DROPEST_GTF");
		const std::string param_files = mode.rfind("params:", 0) == 0 ? mode.substr(7) : "";
		const char *phred = std::getenv("DROPEST_MIN_PHRED");
		const auto t0 = std::chrono::steady_clock::now();
		BamProcessing::BamController ctl(tags, mode == "filled", param_files, gtf ? gtf : "", chromosome_gene, phred ? std::atoi(phred) + 33 : 0, threads);
		ctl.set_device_read_sources(device_sources);
		const auto t1 = std::chrono::steady_clock::now();
		ctl.parse_bam_files(bams, output == 'b', c);
		const auto t2 = std::chrono::steady_clock::now();
		c.set_initialized();
		c.merge_and_filter();
		if (output == 'F') ctl.write_filtered_bam_files(bams, c);
		ResultsPrinter(true, false, false, std::getenv("DROPEST_RPUPC") != nullptr).save_results(c, out + ".rds");
		auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
		const auto &k = ctl.counters();
		std::printf("{\"total_reads\": %zu, \"cant_parse\": %zu, \"low_quality\": %zu, \"saved\": %zu, \"load_params_ms\": %.3f, \"ingest_ms\": %.3f}\n",
		            k.total_reads, k.cant_parse, k.low_quality, k.saved, ms(t0, t1), ms(t1, t2));
	} catch (const std::exception &e) {
		std::fprintf(stderr, "ERROR: %s\n", e.what());
		return 1;
	}
	return 0;
}
