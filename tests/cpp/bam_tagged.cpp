// BAM file(s) -> count matrices AND tagged BAM files (-b) through the facade: BamController::parse_bam_files(files, true, container) writes
// `<input stem>.tagged.bam` into the current directory for every input (device BAM path: csrc/k_bamtag.h + include/dropest_deflate.h), then the
// estimation runs and ResultsPrinter writes <out_base>.rds as bam_to_counts does.  Used by tests/test_gpu_bam_tagged_file.py and
// scripts/bench_bam_tagged.py.
//   bam_tagged <out_base> <filled|name|params:files> <threads> <bam> [<bam> ...]
//   environment: DROPEST_GTF = annotation file for -g; DROPEST_MIN_PHRED = min_barcode_quality; DROPEST_NO_TAGGED = 1: the same ingest without -b
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include "../../dropest_amd/csrc/host/bam_ingest.h"

using namespace Estimation;

int main(int argc, char **argv) {
	if (argc < 5) { std::fprintf(stderr, "usage: %s out_base filled|name threads bam...\n", argv[0]); return 2; }
	try {
		const std::string out = argv[1], mode = argv[2];
		const unsigned threads = unsigned(std::atoi(argv[3]));
		std::vector<std::string> bams(argv + 4, argv + argc);
		auto merge = std::make_shared<Merge::DummyMergeStrategy>(0, 0);
		auto umi = std::make_shared<Merge::UMIs::MergeUMIsStrategySimple>(1);
		CellsDataContainer c(merge, umi, UMI::Mark::get_by_code(UMI::Mark::DEFAULT_CODE), false, -1, std::vector<int>{0});
		BamProcessing::BamTags tags;
		tags.read_type = "RE"; tags.intronic_read_value = "N"; tags.intergenic_read_value = "I"; tags.exonic_read_value = "E";   // as bam_to_counts
		const char *gtf = std::getenv("DROPEST_GTF");
		const std::string param_files = mode.rfind("params:", 0) == 0 ? mode.substr(7) : "";
		const char *phred = std::getenv("DROPEST_MIN_PHRED");
		BamProcessing::BamController ctl(tags, mode == "filled", param_files, gtf ? gtf : "", false, phred ? std::atoi(phred) + 33 : 0, threads);
		const bool print_bams = std::getenv("DROPEST_NO_TAGGED") == nullptr;
		if (!print_bams) ctl.set_device_decode(true);
		const auto t0 = std::chrono::steady_clock::now();
		try { ctl.parse_bam_files(bams, print_bams, c); }
		catch (const std::exception &e) {      // what the container holds after a refusal: nothing was read
			const auto &k = ctl.counters();
			std::printf("{\"error\": true, \"total_reads\": %zu, \"cant_parse\": %zu, \"low_quality\": %zu, \"saved\": %zu, \"files_written\": %zu}\n", k.total_reads, k.cant_parse, k.low_quality, k.saved, ctl.tagged_files().size());
			throw;
		}
		const auto t1 = std::chrono::steady_clock::now();
		c.set_initialized();
		c.merge_and_filter();
		ResultsPrinter(true, false, false, false).save_results(c, out + ".rds");
		auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
		const auto &k = ctl.counters();
		std::printf("{\"total_reads\": %zu, \"cant_parse\": %zu, \"low_quality\": %zu, \"saved\": %zu, \"cells\": %zu, \"ingest_ms\": %.3f, \"files\": [", k.total_reads, k.cant_parse, k.low_quality, k.saved,
		            c.total_cells_number(), ms(t0, t1));
		bool first = true;
		for (const auto &t : ctl.tagged_files()) {
			std::printf("%s{\"name\": \"%s\", \"windows\": %zu, \"records\": %zu, \"inflated_bytes\": %zu, \"compressed_bytes\": %zu, \"batches\": %zu, \"tag_ms\": %.3f, \"deflate_ms\": %.3f, "
			            "\"tag_bytes_in\": %zu, \"tag_bytes_out\": %zu}", first ? "" : ", ", t.name.c_str(), t.windows, t.records, t.inflated_bytes, t.compressed_bytes, t.batches, t.tag_ms, t.deflate_ms,
			            t.tag_bytes_in, t.tag_bytes_out);
			first = false;
		}
		std::printf("]}\n");
	} catch (const std::exception &e) {
		std::fprintf(stderr, "ERROR: %s\n", e.what());
		return 1;
	}
	return 0;
}
