// umi_merge_targets.cpp -- Gene::merge_targets() through the C++ facade (dropest_amd/csrc/host/facade.h): a container made with
// save_umi_merge_targets keeps what Gene::merge(source, target) stores (Gene.cpp:54-57), one made without keeps nothing.  The reads are the
// reference's testUMIMergeStrategySimple (Tests/TestEstimation.cpp:505-540).  Needs a GPU (run by tests/test_gpu_facade_umi_targets.py).
// Exit code 0 = all checks passed.
#include <cstdio>
#include <iostream>

#include "../../dropest_amd/csrc/host/facade.h"

using namespace Estimation;
using Mark = UMI::Mark;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static ReadInfo read_info(const std::string &cb, const std::string &umi, const std::string &gene) {
	return ReadInfo(Tools::ReadParameters(cb, umi, "", umi), gene, "", Mark(Mark::HAS_EXONS));
}

static void fill(CellsDataContainer &c) {
	for (const char *u : {"AAACCT", "AAACCT", "AAACCG", "AAACCN", "CCCCCT", "ACCCCT"}) c.add_record(read_info("AAATTAGGTCCA", u, "Gene1"));
	for (const char *u : {"TTTTTT", "TTTNNG", "TTGNNG", "ACCCCT", "NNNNNN"}) c.add_record(read_info("AAATTAGGTCCA", u, "Gene2"));
}

int main() {
	auto dummy = std::make_shared<Merge::DummyMergeStrategy>(0, 0);
	auto simple = std::make_shared<Merge::UMIs::MergeUMIsStrategySimple>(1);
	const auto marks = Mark::get_by_code(Mark::DEFAULT_CODE);
	{
		CellsDataContainer c(dummy, simple, marks, /*save_umi_merge_targets=*/true);
		CHECK(c.save_umi_merge_targets());
		fill(c);
		CHECK(c.umi_merge_targets(0, 0).empty());                       // before any merge (answered by the preview)
		c.set_initialized();
		c.merge_and_filter();
		const auto g1 = c.umi_merge_targets(0, 0), g2 = c.umi_merge_targets(0, 1);
		CHECK(g1.size() == 1 && g1.count("AAACCN") && g1.at("AAACCN") == "AAACCT");     // two reads beat one at distance 0
		CHECK(g2.size() == 3 && g2.count("TTTNNG") && g2.count("TTGNNG") && g2.count("NNNNNN"));
		CHECK(g2.count("TTTNNG") && g2.at("TTTNNG") == "TTTTTT");                        // the only clean UMI within one mismatch
		for (auto const &kv : g2) CHECK(kv.second.find('N') == std::string::npos && kv.second.size() == 6);
		CHECK(c.umi_merge_targets(0, 2).empty());
	}
	{
		CellsDataContainer c(dummy, simple, marks);                         // the reference's default: nothing is kept
		CHECK(!c.save_umi_merge_targets());
		fill(c);
		c.set_initialized();
		c.merge_and_filter();
		CHECK(c.umi_merge_targets(0, 0).empty() && c.umi_merge_targets(0, 1).empty());
	}
	{
		CellsDataContainer c(dummy, simple, marks, true);                   // merge_umis by hand, before set_initialized (Tests/TestEstimation.cpp:468-488)
		for (const char *u : {"AAACCT", "CCCCCT", "AAATTN", "ACCCCT"}) c.add_record(read_info("AAATTAGGTCCA", u, "Gene1"));
		c.merge_umis(0, 0, {{"AAACCT", "CCCCCT"}, {"AAATTN", "GGGGGG"}, {"ACCCCT", "ACCCCT"}});
		c.set_initialized();
		const auto g = c.umi_merge_targets(0, 0);
		CHECK(g.size() == 2 && g.count("AAACCT") && g.count("AAATTN"));
		CHECK(g.count("AAACCT") && g.at("AAACCT") == "CCCCCT");
		CHECK(g.count("AAATTN") && g.at("AAATTN") == "GGGGGG");
	}
	if (failures) { std::printf("%d checks failed\n", failures); return 1; }
	std::printf("umi merge targets ok\n");
	return 0;
}
