// bam_filtered over a sharded or split container: BAM file(s) -> container on the listed devices -> set_initialized -> merge_and_filter ->
// BamController::write_filtered_bam_files (-F) with BamController::set_sharded_filtered_output on: one `<first input's stem>.filtered.bam` in the
// current directory, written under the shards' decisions (dropest_bam_decoder_filter_window_segments).  Prints bam_filtered's JSON line plus the
// shard count.  Used by tests/test_gpu_bam_filtered_file_sharded.py and scripts/bench_bam_filtered.py.
//   bam_filtered_sharded <filled|name|params:files> <none|real:whitelist> <min_genes_before_merge> <min_genes_after_merge> <simple|directional>
//                        <save_umi_merge_targets 0|1> <devices, e.g. 0,0> <shard quota, 0 = the container's own rule> <bam> [<bam> ...]
//   a device list of one device is one context, which splits on its own when its sort key passes 64 bits
//   environment: DROPEST_GTF = annotation file for -g; DROPEST_FILTER_SWITCH_OFF = 1: the switch stays off (refused, as bam_filtered is);
//   DROPEST_FILTER_DUMP = file: the container's decision for every read (CellsDataContainer::read_corrections_host), one line each: verdict,
//   target barcode, corrected UMI ("-" = none)
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include "../../dropest_amd/csrc/host/bam_ingest.h"

using namespace Estimation;

int main(int argc, char **argv) {
	if (argc < 10) { std::fprintf(stderr, "usage: %s filled|name|params:files none|real:whitelist min_before min_after simple|directional save_targets devices quota bam...\n", argv[0]); return 2; }
	try {
		const std::string mode = argv[1], merge_arg = argv[2], umi_arg = argv[5];
		const size_t min_before = size_t(std::atoi(argv[3])), min_after = size_t(std::atoi(argv[4]));
		const bool save_targets = std::atoi(argv[6]) != 0;
		std::vector<int> devices;
		{
			std::istringstream in(argv[7]);
			for (std::string d; std::getline(in, d, ',');) devices.push_back(std::atoi(d.c_str()));
		}
		const size_t quota = size_t(std::atoll(argv[8]));
		std::vector<std::string> bams(argv + 9, argv + argc);
		std::shared_ptr<Merge::MergeStrategyAbstract> merge;
		if (merge_arg.rfind("real:", 0) == 0)
			merge = std::make_shared<Merge::RealBarcodesMergeStrategy>(Merge::RealBarcodesMergeStrategy::CONST_LENGTH, merge_arg.substr(5), min_before, min_after, 2, 0.0);
		else merge = std::make_shared<Merge::DummyMergeStrategy>(min_before, min_after);
		std::shared_ptr<Merge::UMIs::MergeUMIsStrategyAbstract> umi;
		if (umi_arg == "directional") umi = std::make_shared<Merge::UMIs::MergeUMIsStrategyDirectional>();
		else umi = std::make_shared<Merge::UMIs::MergeUMIsStrategySimple>(1);
		const auto marks = UMI::Mark::get_by_code(UMI::Mark::DEFAULT_CODE);
		CellsDataContainer c(merge, umi, marks, save_targets, -1, devices);
		if (quota) c.set_shard_quota(quota);
		BamProcessing::BamTags tags;
		tags.read_type = "RE"; tags.intronic_read_value = "N"; tags.intergenic_read_value = "I"; tags.exonic_read_value = "E";   // as bam_filtered
		const char *gtf = std::getenv("DROPEST_GTF");
		const std::string param_files = mode.rfind("params:", 0) == 0 ? mode.substr(7) : "";
		BamProcessing::BamController ctl(tags, mode == "filled", param_files, gtf ? gtf : "", false, 0, 4);
		if (param_files.empty()) ctl.set_device_decode(true);
		ctl.set_sharded_filtered_output(std::getenv("DROPEST_FILTER_SWITCH_OFF") == nullptr);
		auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
		const auto t0 = std::chrono::steady_clock::now();
		ctl.parse_bam_files(bams, c);
		const auto t1 = std::chrono::steady_clock::now();
		c.set_initialized();
		c.merge_and_filter();
		if (const char *dump = std::getenv("DROPEST_FILTER_DUMP")) {
			const uint64_t n = ctl.counters().saved;      // read i of the container is the i-th record the files' readers accepted
			std::vector<uint8_t> verdict(n); std::vector<uint64_t> target(n), u(n);
			if (n) c.read_corrections_host(0, n, verdict.data(), target.data(), u.data());
			std::ofstream out(dump);
			for (uint64_t i = 0; i < n; ++i) {
				const std::string cb = target[i] ? c.decode(target[i]) : std::string(), um = c.decode(u[i]);
				out << int(verdict[i]) << ' ' << (cb.empty() ? "-" : cb) << ' ' << (um.empty() ? "-" : um) << '\n';
			}
		}
		const auto t2 = std::chrono::steady_clock::now();
		try { ctl.write_filtered_bam_files(bams, c); }
		catch (const std::exception &) {
			const auto &f = ctl.filtered_file();
			std::printf("{\"error\": true, \"name\": \"%s\", \"windows\": %zu, \"total_reads\": %zu, \"written\": %zu, \"shards\": %zu}\n", f.name.c_str(), f.windows, f.total_reads, f.written, c.shards().size());
			throw;
		}
		const auto t3 = std::chrono::steady_clock::now();
		const auto &f = ctl.filtered_file();
		std::printf("{\"name\": \"%s\", \"windows\": %zu, \"total_reads\": %zu, \"written\": %zu, \"wrong_genes\": %zu, \"wrong_umis\": %zu, \"inflated_bytes\": %zu, \"compressed_bytes\": %zu, "
		            "\"batches\": %zu, \"decode_ms\": %.3f, \"tag_ms\": %.3f, \"deflate_ms\": %.3f, \"ingest_ms\": %.3f, \"filtered_ms\": %.3f, \"decisions_ms\": %.3f, \"shards\": %zu}\n",
		            f.name.c_str(), f.windows, f.total_reads, f.written, f.wrong_genes, f.wrong_umis, f.inflated_bytes, f.compressed_bytes, f.batches, f.decode_ms, f.tag_ms, f.deflate_ms,
		            ms(t0, t1), ms(t2, t3), f.decisions_ms, c.shards().size());
	} catch (const std::exception &e) {
		std::fprintf(stderr, "ERROR: %s\n", e.what());
		return 1;
	}
	return 0;
}
