// BAM file(s) -> .rds through a container whose shards are fed by the device BAM path (tests/test_gpu_bam_sharded_device.py).  Like bam_to_counts, plus
// what that test needs: a quota of any number of reads, reads handed over through add_record before the files, and where every read ended up.
//   bam_sharded_device <out_base> <filled|name|params:...> <min_genes_before> <min_genes_after> <whitelist|-> <threads> <quota|0> <reads.tsv|-> <k> <bam> [<bam> ...]
//   quota > 0: set_shard_quota(quota) (0: the container's own rule).  reads.tsv: one read per line, "barcode umi gene|- chromosome mark quality|-"
//   separated by tabs; its first k lines go through add_record before parse_bam_files.
//   environment: DROPEST_DEVICES = "0,0,0" (one entry: one context), DROPEST_GTF, DROPEST_BAM_DEVICE = 1 and the rest of what BamController reads.
//   Prints {"saved": ..., "shard_reads": [...]}: the reads dealt to every shard (empty for one context).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include "../../dropest_amd/csrc/host/bam_ingest.h"

using namespace Estimation;

int main(int argc, char **argv) {
	if (argc < 11) { std::fprintf(stderr, "usage: %s out_base filled|name|params:... min_before min_after whitelist|- threads quota reads.tsv|- k bam...\n", argv[0]); return 2; }
	try {
		const std::string out = argv[1], mode = argv[2], wl = argv[5], pre = argv[8];
		const size_t min_before = size_t(std::atoi(argv[3])), min_after = size_t(std::atoi(argv[4])), quota = size_t(std::atoll(argv[7])), k_pre = size_t(std::atoll(argv[9]));
		const unsigned threads = unsigned(std::atoi(argv[6]));
		std::vector<std::string> bams(argv + 10, argv + argc);
		std::shared_ptr<Merge::MergeStrategyAbstract> merge;
		if (wl == "-") merge = std::make_shared<Merge::DummyMergeStrategy>(min_before, min_after);
		else merge = std::make_shared<Merge::RealBarcodesMergeStrategy>(Merge::RealBarcodesMergeStrategy::CONST_LENGTH, wl, min_before, min_after, 7, 0.2);
		auto umi = std::make_shared<Merge::UMIs::MergeUMIsStrategySimple>(1);
		std::vector<int> devices;
		if (const char *d = std::getenv("DROPEST_DEVICES")) { std::string t(d); size_t at = 0; while (at < t.size()) { devices.push_back(std::atoi(t.c_str() + at)); at = t.find(',', at); if (at == std::string::npos) break; ++at; } }
		if (devices.empty()) devices.push_back(0);
		CellsDataContainer c(merge, umi, UMI::Mark::get_by_code(UMI::Mark::DEFAULT_CODE), false, -1, devices);
		if (quota && c.sharded()) c.set_shard_quota(quota);
		if (pre != "-" && k_pre) {
			std::ifstream f(pre);
			if (!f) throw std::runtime_error("can't open " + pre);
			std::string line;
			for (size_t i = 0; i < k_pre && std::getline(f, line); ++i) {
				std::vector<std::string> col;
				std::stringstream ss(line);
				for (std::string x; std::getline(ss, x, '\t');) col.push_back(x);
				if (col.size() != 6) throw std::runtime_error("six columns per read: " + line);
				c.add_record(ReadInfo(Tools::ReadParameters(col[0], col[1], "", col[5] == "-" ? "" : col[5]), col[2] == "-" ? "" : col[2], col[3],
				                      UMI::Mark(UMI::Mark::MarkType(std::atoi(col[4].c_str())))));
			}
		}
		BamProcessing::BamTags tags;
		tags.read_type = "RE"; tags.intronic_read_value = "N"; tags.intergenic_read_value = "I"; tags.exonic_read_value = "E";
		const char *gtf = std::getenv("DROPEST_GTF");
		const std::string param_files = mode.rfind("params:", 0) == 0 ? mode.substr(7) : "";
		BamProcessing::BamController ctl(tags, mode == "filled", param_files, gtf ? gtf : "", false, 0, threads);
		ctl.parse_bam_files(bams, c);
		c.set_initialized();
		c.merge_and_filter();
		ResultsPrinter(true, false, false, std::getenv("DROPEST_RPUPC") != nullptr).save_results(c, out + ".rds");
		std::printf("{\"saved\": %zu, \"shard_reads\": [", ctl.counters().saved);
		for (size_t k = 0; k < c.shard_reads().size(); ++k) std::printf("%s%zu", k ? ", " : "", c.shard_reads()[k]);
		std::printf("]}\n");
	} catch (const std::exception &e) {
		std::fprintf(stderr, "ERROR: %s\n", e.what());
		return 1;
	}
	return 0;
}
