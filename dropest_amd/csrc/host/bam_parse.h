// bam_parse.h -- what the files behind bam_ingest.h share (not an interface of the library): the switches of one parse_bam_files call, the
// worker pool, one record -> ParsedRead (RecordParser), the host reader's bulk path over a window of records (BulkWindow) and the step that
// enters what a record brings that the dictionaries have not seen.  bam_ingest.cpp: BamReader and the inflate; bam_controller.cpp: the
// controller and the host reader's loop; bam_device.cpp: the device path.
#pragma once

#include "bam_ingest.h"
#include "bgzf_blocks.h"

#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <mutex>
#include <stdexcept>
#include <thread>

struct dropest_read_params;      // include/dropest_bgzf.h: the read-parameter table on the device

namespace Estimation {
namespace BamProcessing {

using bgzf::le16;
using bgzf::le32;
using bgzf::RawBlock;
using bgzf::read_block;

using clk = std::chrono::steady_clock;
inline double since(clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); }

// inflates one block and checks its CRC-32 and ISIZE (bam_ingest.cpp); throws
void inflate_block(const RawBlock &b, uint8_t *out);

inline bool bam_trace_wanted() { return getenv("DROPEST_BAM_TRACE") != nullptr; }

// Every DROPEST_BAM_* variable parse_bam_files looks at (the switch table), read once when a call begins.
// (DROPEST_BAM_ZLIB and DROPEST_BAM_CALLER_WALKS are BamReader's and are read there.)
struct BamSwitches {
	bool trace_on = false, trace_reader_on = false;
	bool device = false, record_by_record = false, keep_decoders = false;
	bool upload_ahead = true, in_pieces = true, pipeline = false, one_walker = false;
	size_t ramp_first = 1, ramp_factor = 8;                       // DROPEST_BAM_RAMP="first MB,factor": the first window and how fast the windows grow to window_max
	bool has_window_mb = false; size_t window_mb = 0;             // DROPEST_BAM_DEVICE_WINDOW_MB (also lifts the cap of blocks per window)
	bool has_window_blocks = false; size_t window_blocks = 0;     // DROPEST_BAM_WINDOW_BLOCKS (also raises the staging ceiling to 512 MB)
	size_t piece_bytes = size_t(2) << 20;
	uint32_t readers = 8;
	size_t stretch_bytes = size_t(8) << 20, stretch_blocks = 8192;   // tests: DROPEST_BAM_TEST_STRETCH="bytes,blocks" lowers the two thresholds so that small files take the four stretches
	size_t tagged_batch = size_t(64) << 20;                          // -b: inflated bytes per launch of the device compressor; DROPEST_BAM_TAGGED_BATCH_KB lowers it (tests: several batches from a small file)

	static BamSwitches from_environment() {
		BamSwitches s;
		auto set = [](const char *name) { return getenv(name) != nullptr; };
		s.trace_on = bam_trace_wanted(); s.trace_reader_on = set("DROPEST_BAM_TRACE_READER");
		if (const char *e = getenv("DROPEST_BAM_DEVICE")) s.device = atoi(e) != 0;
		s.record_by_record = set("DROPEST_BAM_RECORD_BY_RECORD");   // tests: the two paths agree
		s.keep_decoders = set("DROPEST_BAM_KEEP_DECODERS");
		if (const char *e = getenv("DROPEST_BAM_RAMP")) { int a = 0, b = 0; if (std::sscanf(e, "%d,%d", &a, &b) == 2 && a >= 1 && b >= 2) { s.ramp_first = size_t(a); s.ramp_factor = size_t(b); } }
		if (const char *e = getenv("DROPEST_BAM_DEVICE_WINDOW_MB")) { s.has_window_mb = true; s.window_mb = size_t(std::max(1, atoi(e))); }
		if (const char *e = getenv("DROPEST_BAM_WINDOW_BLOCKS")) { s.has_window_blocks = true; s.window_blocks = size_t(std::max(64, atoi(e))); }
		s.upload_ahead = !set("DROPEST_BAM_NO_UPLOAD_AHEAD");
		s.in_pieces = s.upload_ahead && !set("DROPEST_BAM_WHOLE_WINDOW_STAGING");
		const char *piece = getenv("DROPEST_BAM_PIECE_MB"), *readers = getenv("DROPEST_BAM_READERS");
		s.piece_bytes = size_t(std::min(16, std::max(1, piece ? atoi(piece) : 2))) << 20;
		s.readers = uint32_t(std::min(8, std::max(1, readers ? atoi(readers) : 8)));
		const bool pipeline = set("DROPEST_BAM_PIPELINE"), no_pipeline = set("DROPEST_BAM_NO_PIPELINE");
		s.pipeline = s.upload_ahead && pipeline && !no_pipeline;
		s.one_walker = set("DROPEST_BAM_ONE_WALKER");
		if (const char *e = getenv("DROPEST_BAM_TAGGED_BATCH_KB")) s.tagged_batch = std::min(s.tagged_batch, size_t(std::max(64, atoi(e))) << 10);
		if (const char *e = getenv("DROPEST_BAM_TEST_STRETCH")) { long x = 0, y = 0; if (std::sscanf(e, "%ld,%ld", &x, &y) == 2 && x > 0 && y > 0) { s.stretch_bytes = size_t(x); s.stretch_blocks = size_t(y); } }
		return s;
	}
	// a line on stderr when DROPEST_BAM_TRACE (trace) / DROPEST_BAM_TRACE_READER (trace_reader) is set
	void trace(const char *fmt, ...) const __attribute__((format(printf, 2, 3))) { if (!trace_on) return; va_list ap; va_start(ap, fmt); std::vfprintf(stderr, fmt, ap); va_end(ap); }
	void trace_reader(const char *fmt, ...) const __attribute__((format(printf, 2, 3))) { if (!trace_reader_on) return; va_list ap; va_start(ap, fmt); std::vfprintf(stderr, fmt, ap); va_end(ap); }
};

// Worker threads that live as long as the reader / controller: a window of records comes every few milliseconds at the rates
// this path is built for, and creating 64 threads per window costs more than parsing it.  run(fn) executes fn(worker) on every
// worker and returns when all are done; an exception of a worker is rethrown on the caller's thread.
class WorkerPool {
	std::vector<std::thread> threads;
	std::mutex m;
	std::condition_variable cv_go, cv_done;
	std::function<void(unsigned)> job;
	uint64_t generation = 0;
	unsigned pending = 0;
	bool stop = false;
	std::vector<std::string> errors;
public:
	explicit WorkerPool(unsigned n) : errors(n) {
		for (unsigned t = 0; t < n; ++t)
			threads.emplace_back([this, t] {
				uint64_t seen = 0;
				for (;;) {
					std::function<void(unsigned)> fn;
					{
						std::unique_lock<std::mutex> lk(m);
						cv_go.wait(lk, [&] { return stop || generation != seen; });
						if (stop) return;
						seen = generation; fn = job;
					}
					try { fn(t); } catch (const std::exception &e) { errors[t] = e.what(); } catch (...) { errors[t] = "unknown error"; }
					{ std::lock_guard<std::mutex> lk(m); if (--pending == 0) cv_done.notify_all(); }
				}
			});
	}
	~WorkerPool() {
		{ std::lock_guard<std::mutex> lk(m); stop = true; }
		cv_go.notify_all();
		for (auto &t : threads) t.join();
	}
	unsigned size() const { return unsigned(threads.size()); }
	void run(const std::function<void(unsigned)> &fn) {
		{
			std::lock_guard<std::mutex> lk(m);
			job = fn; pending = unsigned(threads.size()); ++generation;
			for (auto &e : errors) e.clear();
		}
		cv_go.notify_all();
		std::unique_lock<std::mutex> lk(m);
		cv_done.wait(lk, [&] { return pending == 0; });
		for (auto const &e : errors) if (!e.empty()) throw std::runtime_error(e);
	}
};

struct Parsed {
	enum : uint8_t { OK = 0, SKIP, CANT_PARSE_NO_COUNT, CANT_PARSE, LOW_QUALITY };
	CellsDataContainer::ParsedRead r; uint8_t status; std::string gene; /* -g: the annotation's answer (owned) */
	std::string_view name;                  // -r: the read name, looked up in file order by the caller's thread
	std::string p_cb, p_umi, p_quality;     // -r: the served parameters (owned: the map entry is erased)
};

// -r: the read-parameter files as the controller keeps them -- the inflated text of every file, one after the other, and the two ends of every
// line in it (a line's '\n' included; a file's last line may have none).  Nothing is split and no map is built here: the host reader builds its
// map from the lines when it first takes a file (BamController::map_read_params), the device path makes a table on the container's GPU
// (include/dropest_bgzf.h: dropest_read_params_*; table_on, bam_device.cpp) and spells a served row's strings from its line (row k = line k).
struct ParamSource {
	std::vector<uint8_t> text;
	std::vector<uint64_t> line_be;              // line k: text[line_be[2 k] .. line_be[2 k + 1])
	std::vector<uint64_t> file_lines;           // the first line of every file, and the number of lines behind the last
	int min_barcode_phred = 0;
	dropest_read_params *table = nullptr;       // on GPU table_device, made when the device path first takes a file; its claims live as long as this
	int table_device = -1;
	uint64_t ordinal = 0;                       // records the device path has been through: the next window's first record claims with this
	bool host_served = false;                   // the host reader's map has served rows the table does not know of: no more files for the device path
	~ParamSource();
	dropest_read_params *table_on(int device);  // null: no table on that GPU (none can be made, or the table lives on another one)
	struct Row { std::string_view name, cb, umi, cb_quality, umi_quality; bool pass; };
	// BamController::load_read_params' row rules (ReadParameters::parse_from_string, check_quality); false: the line gives no row
	bool row(size_t k, Row &out) const {
		const char *b = reinterpret_cast<const char *>(text.data()) + line_be[2 * k], *e = reinterpret_cast<const char *>(text.data()) + line_be[2 * k + 1];
		if (e > b && e[-1] == '\n') { --e; if (e > b && e[-1] == '\r') --e; }
		std::string_view rest(b, size_t(e - b)), part[5];
		for (int i = 0; i < 4; ++i) {
			const size_t sp = rest.find(' ');
			if (sp == std::string_view::npos) return false;
			part[i] = rest.substr(0, sp); rest.remove_prefix(sp + 1);
		}
		part[4] = rest;
		if (!part[0].empty() && part[0][0] == '@') part[0].remove_prefix(1);
		if (part[1].empty() || part[2].empty()) return false;
		out = Row{part[0], part[1], part[2], part[3], part[4], true};
		if (min_barcode_phred > 33) {
			for (char q : part[3]) out.pass &= q >= char(min_barcode_phred);
			for (char q : part[4]) out.pass &= q >= char(min_barcode_phred);
		}
		return true;
	}
	size_t lines() const { return line_be.size() / 2; }
};

// A parse status into the counters (BamController::Counters, or a worker's tally with the same members); true: the record is to be saved.
template <class C> inline bool count_status(C &c, uint8_t status) {
	switch (status) {
		case Parsed::SKIP: return false;
		case Parsed::CANT_PARSE_NO_COUNT: ++c.cant_parse; return false;             // reads with unknown chromosome are not counted (:107)
		case Parsed::CANT_PARSE: ++c.total_reads; ++c.cant_parse; return false;
		case Parsed::LOW_QUALITY: ++c.total_reads; ++c.low_quality; return false;
		default: ++c.total_reads; ++c.saved; return true;
	}
}

// one record -> Parsed; runs on the worker threads (reads the window, writes only its own slot; the dictionaries are read-only meanwhile)
struct RecordParser {
	static constexpr int quality_offset = 33;                            // Tools::ReadParameters::quality_offset
	const BamTags &tags;
	const bool filled_bam, params_from_files, gene_in_chromosome_name;
	const int min_barcode_phred;
	const Tools::GeneAnnotation::RefGenesContainer &genes;
	const std::vector<std::string> &refs;                                // the file's reference names (filled once its header is read)
	CellsDataContainer &container;
	uint16_t wanted_tags[6];

	static uint16_t tag16(const std::string &t) { return t.size() == 2 ? uint16_t(uint8_t(t[0]) | (uint8_t(t[1]) << 8)) : uint16_t(0); }
	RecordParser(const BamTags &tags, bool filled_bam, bool params_from_files, bool gene_in_chromosome_name, int min_barcode_phred,
	             const Tools::GeneAnnotation::RefGenesContainer &genes, const std::vector<std::string> &refs, CellsDataContainer &container)
		: tags(tags), filled_bam(filled_bam), params_from_files(params_from_files), gene_in_chromosome_name(gene_in_chromosome_name),
		  min_barcode_phred(min_barcode_phred), genes(genes), refs(refs), container(container),
		  wanted_tags{tag16(tags.cell_barcode), tag16(tags.umi), tag16(tags.cell_barcode_quality), tag16(tags.umi_quality), tag16(tags.gene), tag16(tags.read_type)} {}

	void parse(const uint8_t *at, Parsed &out) const {
		BamRecord al;
		BamReader::parse_record(at, al);
		CellsDataContainer::ParsedRead &r = out.r;
		r = CellsDataContainer::ParsedRead();
		if (!al.is_mapped() || !al.is_primary()) { out.status = Parsed::SKIP; return; }            // BamController.cpp:87-88
		if (al.ref_id < 0 || size_t(al.ref_id) >= refs.size()) { out.status = Parsed::CANT_PARSE_NO_COUNT; return; }   // :90-104
		r.ref_id = al.ref_id;
		const std::string &chr_name = refs[size_t(al.ref_id)];
		bool pass_quality = true;
		// every tag the record may be asked for, in one walk over its aux data
		enum { T_CB, T_UMI, T_CBQ, T_UMIQ, T_GENE, T_TYPE, T_N };
		std::string_view tv[T_N]; bool tf[T_N];
		al.get_string_tags(wanted_tags, T_N, tv, tf);
		if (filled_bam) {                                             // FilledBamParamsParser.cpp:12-40
			std::string_view cbq, umiq;
			if (!tf[T_CB] || !tf[T_UMI]) { out.status = Parsed::CANT_PARSE; return; }
			r.cb = tv[T_CB]; r.umi = tv[T_UMI];
			if (tf[T_CBQ]) cbq = tv[T_CBQ];
			if (tf[T_UMIQ]) umiq = tv[T_UMIQ];
			if (r.cb.empty() || r.umi.empty()) { out.status = Parsed::CANT_PARSE; return; }       // ReadParameters ctor throws -> false
			if (min_barcode_phred > quality_offset) {                  // ReadParameters::check_quality (:118-136)
				for (char q : cbq) pass_quality &= q >= char(min_barcode_phred);
				for (char q : umiq) pass_quality &= q >= char(min_barcode_phred);
			}
			r.umi_quality_length = uint32_t(umiq.size());
			r.umi_quality = umiq;
		} else if (params_from_files) {                               // ReadMapParamsParser: resolved by the controller, in file order
			out.name = al.name_view;
		} else {                                                      // ReadParamsParser.cpp:20-33: "id!CB#UMI"
			const std::string_view name = al.name_view;
			const size_t up = name.rfind('#');
			const size_t cp = up == std::string_view::npos ? std::string_view::npos : name.rfind('!', up);
			if (up == std::string_view::npos || cp == std::string_view::npos) { out.status = Parsed::CANT_PARSE; return; }
			r.cb = name.substr(cp + 1, up - cp - 1); r.umi = name.substr(up + 1);
			if (r.cb.empty() || r.umi.empty()) { out.status = Parsed::CANT_PARSE; return; }
			// parse_encoded_id builds ReadParameters(cb, umi, "", "") = min_phred_score 0: always passes (ReadParameters.cpp:42-56)
		}
		if (!pass_quality) { out.status = Parsed::LOW_QUALITY; return; }
		// get_gene (ReadParamsParser.cpp:36-65) + parse_read_type (:67-90)
		UMI::Mark mark;
		if (gene_in_chromosome_name) {
			r.gene = chr_name;
			if (!chr_name.empty()) mark.add(UMI::Mark::HAS_EXONS);
		} else if (!genes.is_empty()) {                               // get_gene_from_reference (:92-151)
			int bits;
			try { bits = genes.gene_of_alignment(chr_name, size_t(al.position), size_t(al.end_position), out.gene); }
			catch (const Tools::GeneAnnotation::RefGenesContainer::ChrNotFoundException &) { out.status = Parsed::CANT_PARSE; return; }   // BamController.cpp:153-161
			if (bits & 1) mark.add(UMI::Mark::HAS_NOT_ANNOTATED);
			if (bits & 2) mark.add(UMI::Mark::HAS_EXONS);
			if (bits & 4) mark.add(UMI::Mark::HAS_INTRONS);
			r.gene = out.gene;
		} else if (!tf[T_GENE]) {
			r.gene = std::string_view();
			mark.add(UMI::Mark::HAS_NOT_ANNOTATED);
		} else {
			r.gene = tv[T_GENE];
			std::string_view read_type;
			if (tf[T_TYPE]) read_type = tv[T_TYPE];
			if (tags.read_type.empty() || !tf[T_TYPE]) mark.add(UMI::Mark::HAS_EXONS);
			else if (read_type == tags.intronic_read_value) mark.add(UMI::Mark::HAS_INTRONS);
			else if (!tags.intergenic_read_value.empty() && read_type == tags.intergenic_read_value) mark.add(UMI::Mark::HAS_NOT_ANNOTATED);
			else mark.add(UMI::Mark::HAS_EXONS);
		}
		r.mark = uint8_t(mark.bits());
		if (params_from_files) r.cb_code = r.umi_code = 0;
		else {
			if (!CellsDataContainer::pack_code(r.cb, r.cb_code)) r.cb_code = 0;
			if (!CellsDataContainer::pack_code(r.umi, r.umi_code)) r.umi_code = 0;
		}
		r.gene_hash = CellsDataContainer::hash_name(r.gene);
		if (!r.gene.empty()) r.gene_id = container.lookup_gene(r.gene_hash, r.gene);   // dictionary is read-only while the workers run
		out.status = Parsed::OK;
	}
};

// What one record brings that the dictionaries have not seen; entered on the caller's thread, record by record in file order, and per
// record: barcode, then UMI, gene, chromosome -- the order of add_record.  The host reader's bulk path collects these on its workers
// (BulkWindow), the device path makes them from the records the device handed back (bam_device.cpp): the order exists here alone.
enum : uint8_t { NEED_CB = 1, NEED_UMI = 2, NEED_GENE = 4, NEED_CHR = 8 };
struct NewParts { uint8_t what; int32_t ref; std::string_view cb, umi, gene; uint64_t gene_hash; };
inline void intern_new(CellsDataContainer &container, const NewParts &p, uint64_t &cb, uint64_t &umi, uint32_t &gene, uint32_t &aux) {
	if (p.what & NEED_CB) cb = container.intern_barcode(std::string(p.cb));
	if (p.what & NEED_UMI) umi = container.intern_umi(std::string(p.umi));
	if (p.what & NEED_GENE) gene = container.intern_gene(p.gene, p.gene_hash);
	if (p.what & NEED_CHR) { container.intern_chromosome_of_ref(p.ref); aux |= uint32_t(container.chromosome_of_ref(p.ref)); }
}

// ---- the host reader's bulk path: the workers write packed records, the caller's thread only resolves what is NEW ----
// A record needs the caller's thread when it brings something the dictionaries have not seen: a gene name that is not in the
// gene dictionary yet, a chromosome no counted read touched before, a barcode / UMI that does not pack into a 2-bit code (N).
// After the first windows that is a handful of records per million.  Everything else -- parsing, packing, gene look-up,
// the chromosome index, the compaction of the accepted records -- runs on the workers; the container receives whole arrays
// (CellsDataContainer::add_records_packed).  Order of every dictionary operation = file order, as add_record read by read.
// One per file; its buffers are never shrunk (no refill per window).
class BulkWindow {
	static constexpr uint32_t NO_QL = 0xFFFFFFFFu;
	struct Need { uint32_t idx; NewParts p; std::string gene_owned; /* -g: the annotation's answer lives in the worker's scratch record */ };
	struct Tally { size_t total_reads = 0, cant_parse = 0, low_quality = 0, saved = 0; uint32_t ql = NO_QL; bool mixed = false; char pad[64]; };
	const RecordParser &parser;
	CellsDataContainer &container;
	BamController::Counters &counters;
	WorkerPool workers;
	std::vector<std::vector<Need>> needs;
	// every worker writes the records it accepts densely from the start of ITS range of the window (o_*[n t / NT ...]): the container
	// then takes one call per worker, in worker order = file order -- no second pass that closes the gaps (it was 170 ms of a 930 ms ingest)
	std::vector<uint64_t> o_cb, o_umi;
	std::vector<uint32_t> o_gene, o_aux;
	// UMI quality strings (UQ tags): while every gene-bearing read brings one of the same length, the window still goes in bulk -- every worker
	// keeps where the strings of its records are and, once the length is known for the whole window, copies them into one row per read
	// (CellsDataContainer::add_records_packed with rows); reads of different lengths, or a length other than the container's so far, leave the
	// window to the record-by-record path (UMI::add_read's length check, UMI.cpp:26-28, is per molecule there)
	std::vector<const char *> o_qp;
	std::vector<uint8_t> o_qual;
	std::vector<const uint8_t *> q_rows;
	std::vector<Tally> tally;
	std::vector<CellsDataContainer::PackedRun> runs;
	void parse_and_pack(const uint8_t *data, const std::vector<uint32_t> &offsets, size_t n);
	void add_with_quality_rows(size_t n, uint32_t ql);
public:
	size_t est_reads = 0;          // what the host reader told the container to expect (quality rows are reserved for as many)
	double ms[3] = {0, 0, 0};      // DROPEST_BAM_TRACE: parse + pack on the workers, new dictionary entries on this thread, container
	BulkWindow(unsigned threads, const RecordParser &parser, BamController::Counters &counters)
		: parser(parser), container(parser.container), counters(counters), workers(threads), needs(workers.size()), tally(workers.size()) {}
	unsigned threads() const { return workers.size(); }
	// records data + offsets[0 .. n) into the container; false: refused before anything was added (the caller goes record by record)
	bool ingest(const uint8_t *data, const std::vector<uint32_t> &offsets, size_t n);
};

// One file of a parse_bam_files call: what its two readers (the device path, the host reader) share
struct FileIngest {
	const BamSwitches &sw;
	const std::string &bam_name;
	const size_t n_files;
	CellsDataContainer &container;
	BamController::Counters &counters;
	std::vector<std::string> refs;       // the file's reference names, from whichever reader read its header
	RecordParser parser;
	BulkWindow bulk;
	BamController::TaggedFile *tagged = nullptr;   // -b: this file's tagged BAM is to be written (device path only); what was written is noted here
	struct FilteredPass *filtered = nullptr;       // -F: the file is read for write_filtered_bam_files -- nothing goes into the container
	std::string refusal;                 // why the device path handed the file back (read_file_on_device returned false)
	bool device_sources = false;         // BamController::set_device_read_sources: the device path may take the file under -r and -P
	bool source_output = false;          // BamController::set_device_source_output: ... and write its tagged / filtered records there
	ParamSource *params = nullptr;       // -r with that switch: the rows for the device path's table
	FileIngest(const BamSwitches &sw, const std::string &bam_name, size_t n_files, CellsDataContainer &container, BamController::Counters &counters,
	           const BamTags &tags, bool filled_bam, bool params_from_files, bool gene_in_chromosome_name, int min_barcode_phred,
	           const Tools::GeneAnnotation::RefGenesContainer &genes, unsigned threads)
		: sw(sw), bam_name(bam_name), n_files(n_files), container(container), counters(counters),
		  parser(tags, filled_bam, params_from_files, gene_in_chromosome_name, min_barcode_phred, genes, refs, container), bulk(threads, parser, counters) {}
};

// -F (bam_device.cpp): what the files of one write_filtered_bam_files call share -- the container's decisions on the device, the running count of
// accepted records, the one output and its compressor.  _open throws what the read corrections refuse; _close(ok): what is left over, the
// end-of-file block and the account in `report` when ok, else the output is removed and `report` left empty.
// sharded_output (BamController::set_sharded_filtered_output): a sharded or split container's decisions are its shards', one piece of the stream
// each; off, such a container is handed to the one-context call, which refuses it.
struct FilteredPass;
FilteredPass *filtered_pass_open(const BamSwitches &sw, CellsDataContainer &container, BamController::FilteredFile &report, bool sharded_output);
void filtered_pass_close(FilteredPass *pass, bool ok);
// -r: the pass serves the rows afresh, as the reference's new parser does -- from the first file on the table's claims are an array of the pass's
// own and the stream ordinals restart at 0 (dropest_read_params_replay_begin); _close puts both back, however the pass ended.  Once per pass.
void filtered_pass_replay(FilteredPass *pass, ParamSource &params);
uint64_t filtered_pass_reads(const FilteredPass *pass);      // accepted records of the files read so far
uint64_t filtered_pass_total(const FilteredPass *pass);      // the container's reads
[[noreturn]] void filtered_pass_other_files(const FilteredPass *pass, const std::string &what);

// bam_device.cpp: the file through the GPU (include/dropest_bgzf.h); false: the host reader is to read it, nothing was added
bool read_file_on_device(FileIngest &file);
// -r: per line of src, whether the device path's table served it (empty: there is no table, nothing was served)
std::vector<uint8_t> consumed_read_params(ParamSource &src);
void join_release_thread();
void release_decoders_in_background();

}  // namespace BamProcessing
}  // namespace Estimation
