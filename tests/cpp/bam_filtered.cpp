// BAM file(s) -> container -> set_initialized -> merge_and_filter -> BamController::write_filtered_bam_files (-F) through the facade: one
// `<first input's stem>.filtered.bam` in the current directory (device BAM path: the filtered mode of csrc/k_bamtag.h + include/dropest_deflate.h).
// Prints one JSON line with BamController::filtered_file()'s counters.  Used by tests/test_gpu_bam_filtered_file.py and scripts/bench_bam_filtered.py.
//   bam_filtered <filled|name|params:files> <none|real:whitelist> <min_genes_before_merge> <min_genes_after_merge> <simple|directional> <save_umi_merge_targets 0|1> <bam> [<bam> ...]
//   environment: DROPEST_GTF = annotation file for -g; DROPEST_DEVICES = "0,0": a sharded container (refused);
//   DROPEST_FILTER_FILES = "a.bam:b.bam": the files of the SECOND pass when they are not the ones the container was filled from (refused);
//   DROPEST_FILTER_DUMP = file: the container's decision for every read, one line each: verdict, target cell's barcode, corrected UMI ("-" = none)
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include "../../dropest_amd/csrc/host/bam_ingest.h"
#include "../../include/dropest_synth.h"

using namespace Estimation;

int main(int argc, char **argv) {
	if (argc < 8) { std::fprintf(stderr, "usage: %s filled|name|params:files none|real:whitelist min_before min_after simple|directional save_targets bam...\n", argv[0]); return 2; }
	try {
		const std::string mode = argv[1], merge_arg = argv[2], umi_arg = argv[5];
		const size_t min_before = size_t(std::atoi(argv[3])), min_after = size_t(std::atoi(argv[4]));
		const bool save_targets = std::atoi(argv[6]) != 0;
		std::vector<std::string> bams(argv + 7, argv + argc);
		std::shared_ptr<Merge::MergeStrategyAbstract> merge;
		if (merge_arg.rfind("real:", 0) == 0)
			merge = std::make_shared<Merge::RealBarcodesMergeStrategy>(Merge::RealBarcodesMergeStrategy::CONST_LENGTH, merge_arg.substr(5), min_before, min_after, 2, 0.0);
		else merge = std::make_shared<Merge::DummyMergeStrategy>(min_before, min_after);
		std::shared_ptr<Merge::UMIs::MergeUMIsStrategyAbstract> umi;
		if (umi_arg == "directional") umi = std::make_shared<Merge::UMIs::MergeUMIsStrategyDirectional>();
		else umi = std::make_shared<Merge::UMIs::MergeUMIsStrategySimple>(1);
		const auto marks = UMI::Mark::get_by_code(UMI::Mark::DEFAULT_CODE);
		std::unique_ptr<CellsDataContainer> cp;
		if (const char *devs = std::getenv("DROPEST_DEVICES")) {
			std::vector<int> devices;
			std::istringstream in(devs);
			for (std::string d; std::getline(in, d, ',');) devices.push_back(std::atoi(d.c_str()));
			cp.reset(new CellsDataContainer(merge, umi, marks, save_targets, -1, devices));
		} else cp.reset(new CellsDataContainer(merge, umi, marks, save_targets));
		CellsDataContainer &c = *cp;
		BamProcessing::BamTags tags;
		tags.read_type = "RE"; tags.intronic_read_value = "N"; tags.intergenic_read_value = "I"; tags.exonic_read_value = "E";   // as bam_tagged
		const char *gtf = std::getenv("DROPEST_GTF");
		const std::string param_files = mode.rfind("params:", 0) == 0 ? mode.substr(7) : "";
		BamProcessing::BamController ctl(tags, mode == "filled", param_files, gtf ? gtf : "", false, 0, 4);
		if (param_files.empty()) ctl.set_device_decode(true);
		auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
		const auto t0 = std::chrono::steady_clock::now();
		ctl.parse_bam_files(bams, c);
		const auto t1 = std::chrono::steady_clock::now();
		c.set_initialized();
		c.merge_and_filter();
		if (const char *dump = std::getenv("DROPEST_FILTER_DUMP")) {
			dropest_ctx *ctx = c.handle();
			uint64_t n = 0, n_cells = 0;
			const uint8_t *dv = nullptr; const uint32_t *dc = nullptr; const uint64_t *du = nullptr, *d_codes = nullptr;
			if (!ctx || dropest_read_corrections(ctx, &n, &dv, &dc, &du) || dropest_cell_barcodes_device(ctx, &n_cells, &d_codes)) throw std::runtime_error(dropest_last_error());
			std::vector<uint8_t> verdict(n); std::vector<uint32_t> cell(n); std::vector<uint64_t> u(n), codes(n_cells);
			if (n && dropest_read_corrections_host(ctx, 0, n, verdict.data(), cell.data(), u.data())) throw std::runtime_error(dropest_last_error());
			if (n_cells && dropest_dev_copy_to_host(c.device(), codes.data(), d_codes, n_cells * 8)) throw std::runtime_error("the cells' barcodes cannot be copied to the host");
			std::ofstream out(dump);
			for (uint64_t i = 0; i < n; ++i) {
				const std::string cb = cell[i] < n_cells ? c.decode(codes[cell[i]]) : std::string(), um = c.decode(u[i]);
				out << int(verdict[i]) << ' ' << (cb.empty() ? "-" : cb) << ' ' << (um.empty() ? "-" : um) << '\n';
			}
		}
		std::vector<std::string> second = bams;
		if (const char *other = std::getenv("DROPEST_FILTER_FILES")) {
			second.clear();
			std::istringstream in(other);
			for (std::string f; std::getline(in, f, ':');) second.push_back(f);
		}
		const auto t2 = std::chrono::steady_clock::now();
		try { ctl.write_filtered_bam_files(second, c); }
		catch (const std::exception &) {
			const auto &f = ctl.filtered_file();
			std::printf("{\"error\": true, \"name\": \"%s\", \"windows\": %zu, \"total_reads\": %zu, \"written\": %zu}\n", f.name.c_str(), f.windows, f.total_reads, f.written);
			throw;
		}
		const auto t3 = std::chrono::steady_clock::now();
		const auto &f = ctl.filtered_file();
		std::printf("{\"name\": \"%s\", \"windows\": %zu, \"total_reads\": %zu, \"written\": %zu, \"wrong_genes\": %zu, \"wrong_umis\": %zu, \"inflated_bytes\": %zu, \"compressed_bytes\": %zu, "
		            "\"batches\": %zu, \"decode_ms\": %.3f, \"tag_ms\": %.3f, \"deflate_ms\": %.3f, \"ingest_ms\": %.3f, \"filtered_ms\": %.3f, \"cells\": %zu}\n",
		            f.name.c_str(), f.windows, f.total_reads, f.written, f.wrong_genes, f.wrong_umis, f.inflated_bytes, f.compressed_bytes, f.batches, f.decode_ms, f.tag_ms, f.deflate_ms,
		            ms(t0, t1), ms(t2, t3), c.total_cells_number());
	} catch (const std::exception &e) {
		std::fprintf(stderr, "ERROR: %s\n", e.what());
		return 1;
	}
	return 0;
}
