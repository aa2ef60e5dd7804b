// BAM file(s) -> .rds AND tagged / filtered BAM output under the two sources of bam_sources: -r read-parameter files and -P gene = chromosome
// name, which the device BAM path writes output for only behind BamController::set_device_source_output (tests/test_gpu_bam_sources_output.py;
// scripts/bench_bam_params_output.py).  bam_sources' arguments plus that switch:
//   bam_sources_output <out_base> <filled|name|params:files> <chromosome gene 0|1> <device sources 0|1[b|F]> <source output 0|1> <min_genes_before>
//                      <min_genes_after> <whitelist|-> <threads> <devices|-> <quota|0> <bam> [<bam> ...]
//   device sources: set_device_read_sources; a letter behind it asks for output -- b: parse_bam_files(files, true, container) writes
//   `<stem>.tagged.bam` per input, F: write_filtered_bam_files after the estimate writes `<first stem>.filtered.bam` (the container then keeps its
//   UMI merge targets).  devices: "0,0" shards the container (-F over it: set_sharded_filtered_output is on); quota > 0: set_shard_quota.
//   The read-type and -f tags are those of bam_tagged / bam_filtered.
//   environment: DROPEST_GTF, DROPEST_MIN_PHRED, DROPEST_RPUPC as for bam_to_counts; DROPEST_FILTER_DUMP = file: the container's decision for every
//   read as bam_filtered writes it (one context only); DROPEST_FURTHER_FILES = "c.bam:d.bam": parsed into a container of their own by the same
//   controller after everything else ("further" in the output: names the first call consumed must stay consumed).
//   Prints the counters as one JSON line.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include "../../dropest_amd/csrc/host/bam_ingest.h"
#include "../../include/dropest_synth.h"

using namespace Estimation;

static void dump_decisions(CellsDataContainer &c, const char *path) {
	dropest_ctx *ctx = c.handle();
	uint64_t n = 0, n_cells = 0;
	const uint8_t *dv = nullptr; const uint32_t *dc = nullptr; const uint64_t *du = nullptr, *d_codes = nullptr;
	if (!ctx || dropest_read_corrections(ctx, &n, &dv, &dc, &du) || dropest_cell_barcodes_device(ctx, &n_cells, &d_codes)) throw std::runtime_error(dropest_last_error());
	std::vector<uint8_t> verdict(n); std::vector<uint32_t> cell(n); std::vector<uint64_t> u(n), codes(n_cells);
	if (n && dropest_read_corrections_host(ctx, 0, n, verdict.data(), cell.data(), u.data())) throw std::runtime_error(dropest_last_error());
	if (n_cells && dropest_dev_copy_to_host(c.device(), codes.data(), d_codes, n_cells * 8)) throw std::runtime_error("the cells' barcodes cannot be copied to the host");
	std::ofstream out(path);
	for (uint64_t i = 0; i < n; ++i) {
		const std::string cb = cell[i] < n_cells ? c.decode(codes[cell[i]]) : std::string(), um = c.decode(u[i]);
		out << int(verdict[i]) << ' ' << (cb.empty() ? "-" : cb) << ' ' << (um.empty() ? "-" : um) << '\n';
	}
}

int main(int argc, char **argv) {
	if (argc < 13) { std::fprintf(stderr, "usage: %s out_base filled|name|params:files chromosome_gene device_sources source_output min_before min_after whitelist|- threads devices|- quota bam...\n", argv[0]); return 2; }
	try {
		const std::string out = argv[1], mode = argv[2], sources = argv[4], wl = argv[8], dev = argv[10];
		const bool chromosome_gene = std::atoi(argv[3]) != 0, device_sources = sources[0] == '1', source_output = std::atoi(argv[5]) != 0;
		const char output = sources.size() > 1 ? sources[1] : ' ';
		const size_t min_before = size_t(std::atoi(argv[6])), min_after = size_t(std::atoi(argv[7])), quota = size_t(std::atoll(argv[11]));
		const unsigned threads = unsigned(std::atoi(argv[9]));
		std::vector<std::string> bams(argv + 12, argv + argc);
		auto merge_strategy = [&]() -> std::shared_ptr<Merge::MergeStrategyAbstract> {
			if (wl == "-") return std::make_shared<Merge::DummyMergeStrategy>(min_before, min_after);
			return std::make_shared<Merge::RealBarcodesMergeStrategy>(Merge::RealBarcodesMergeStrategy::CONST_LENGTH, wl, min_before, min_after, 7, 0.2);
		};
		auto umi = std::make_shared<Merge::UMIs::MergeUMIsStrategySimple>(1);
		std::vector<int> devices;
		if (dev != "-") { size_t at = 0; while (at < dev.size()) { devices.push_back(std::atoi(dev.c_str() + at)); at = dev.find(',', at); if (at == std::string::npos) break; ++at; } }
		if (devices.empty()) devices.push_back(0);
		const auto marks = UMI::Mark::get_by_code(UMI::Mark::DEFAULT_CODE);
		CellsDataContainer c(merge_strategy(), umi, marks, output == 'F', -1, devices);
		if (quota && c.sharded()) c.set_shard_quota(quota);
		BamProcessing::BamTags tags;
		tags.read_type = "RE"; tags.intronic_read_value = "N"; tags.intergenic_read_value = "I"; tags.exonic_read_value = "E";
		const char *gtf = std::getenv("DROPEST_GTF");
		const std::string param_files = mode.rfind("params:", 0) == 0 ? mode.substr(7) : "";
		const char *phred = std::getenv("DROPEST_MIN_PHRED");
		auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
		const auto t0 = std::chrono::steady_clock::now();
		BamProcessing::BamController ctl(tags, mode == "filled", param_files, gtf ? gtf : "", chromosome_gene, phred ? std::atoi(phred) + 33 : 0, threads);
		ctl.set_device_read_sources(device_sources);
		ctl.set_device_source_output(source_output);
		ctl.set_sharded_filtered_output(c.sharded());
		const auto t1 = std::chrono::steady_clock::now();
		ctl.parse_bam_files(bams, output == 'b', c);
		const auto t2 = std::chrono::steady_clock::now();
		c.set_initialized();
		c.merge_and_filter();
		uint64_t counts[5] = {0, 0, 0, 0, 0};
		auto t3 = std::chrono::steady_clock::now(), t4 = t3;
		if (output == 'F') {
			if (const char *dump = std::getenv("DROPEST_FILTER_DUMP")) dump_decisions(c, dump);
			t3 = std::chrono::steady_clock::now();
			ctl.write_filtered_bam_files(bams, c);
			t4 = std::chrono::steady_clock::now();
			if (!c.sharded() && dropest_read_correction_counts(c.handle(), counts)) throw std::runtime_error(dropest_last_error());
		}
		ResultsPrinter(true, false, false, std::getenv("DROPEST_RPUPC") != nullptr).save_results(c, out + ".rds");
		const BamProcessing::BamController::Counters k = ctl.counters();
		std::printf("{\"total_reads\": %zu, \"cant_parse\": %zu, \"low_quality\": %zu, \"saved\": %zu, \"load_params_ms\": %.3f, \"ingest_ms\": %.3f, \"tagged\": [",
		            k.total_reads, k.cant_parse, k.low_quality, k.saved, ms(t0, t1), ms(t1, t2));
		bool first = true;
		for (const auto &t : ctl.tagged_files()) {
			std::printf("%s{\"name\": \"%s\", \"windows\": %zu, \"records\": %zu, \"tag_ms\": %.3f, \"deflate_ms\": %.3f, \"inflated_bytes\": %zu}", first ? "" : ", ", t.name.c_str(), t.windows, t.records, t.tag_ms,
			            t.deflate_ms, t.inflated_bytes);
			first = false;
		}
		const auto &f = ctl.filtered_file();
		std::printf("], \"filtered\": {\"name\": \"%s\", \"windows\": %zu, \"total_reads\": %zu, \"written\": %zu, \"corrections_written\": %llu, \"decode_ms\": %.3f, \"tag_ms\": %.3f, \"deflate_ms\": %.3f, "
		            "\"decisions_ms\": %.3f, \"filtered_ms\": %.3f}",
		            f.name.c_str(), f.windows, f.total_reads, f.written, (unsigned long long)counts[0], f.decode_ms, f.tag_ms, f.deflate_ms, f.decisions_ms, ms(t3, t4));
		if (const char *further = std::getenv("DROPEST_FURTHER_FILES")) {
			std::vector<std::string> more;
			std::istringstream in(further);
			for (std::string name; std::getline(in, name, ':');) more.push_back(name);
			CellsDataContainer c2(merge_strategy(), umi, marks, false, -1, std::vector<int>{0});
			ctl.parse_bam_files(more, c2);
			const auto &k2 = ctl.counters();
			std::printf(", \"further\": {\"total_reads\": %zu, \"cant_parse\": %zu, \"low_quality\": %zu, \"saved\": %zu}", k2.total_reads - k.total_reads, k2.cant_parse - k.cant_parse,
			            k2.low_quality - k.low_quality, k2.saved - k.saved);
		}
		std::printf("}\n");
	} catch (const std::exception &e) {
		std::fprintf(stderr, "ERROR: %s\n", e.what());
		return 1;
	}
	return 0;
}
