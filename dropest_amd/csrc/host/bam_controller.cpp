// bam_controller.cpp -- BamController (bam_ingest.h): the files of one call, each through the device path (bam_device.cpp) or the host
// reader (BamReader, bam_ingest.cpp), whose windows go into the container in bulk (BulkWindow, bam_parse.h) or record by record.
#include "bam_parse.h"

#include <zlib.h>

#include <cstring>
#include <sstream>

namespace Estimation {
namespace BamProcessing {

BamController::BamController(const BamTags &tags, bool filled_bam, const std::string &read_param_filenames, const std::string &gtf_path,
                             bool gene_in_chromosome_name, int min_barcode_phred, unsigned threads)
	: _tags(tags), _filled_bam(filled_bam), _gene_in_chromosome_name(gene_in_chromosome_name), _min_barcode_phred(min_barcode_phred),
	  _threads(threads) {
	if (!gtf_path.empty()) _genes = Tools::GeneAnnotation::RefGenesContainer(gtf_path);
	if (!filled_bam && !read_param_filenames.empty()) load_read_params(read_param_filenames);   // BamController::get_parser (:117-130)
	if (!_tags.read_type.empty() && _tags.intronic_read_value.empty())
		throw std::runtime_error("You have to specify tag values to be able to parse info about read types (see conf_desc.xml \"Estimation/BamTags/Type/\")");
}

// ReadMapParamsParser::init (ReadMapParamsParser.cpp:50-108): gzip text files, one "name cb umi cb_quality umi_quality" row per
// read (ReadParameters::parse_from_string, ReadParameters.cpp:58-78).  Here the files are only inflated and their lines found; who splits the
// rows depends on the reader that takes the first file: map_read_params for the host reader, a kernel for the device path (ParamSource).
void BamController::load_read_params(const std::string &filenames) {
	_params_from_files = true;
	_param_source = std::make_shared<ParamSource>();
	ParamSource &src = *_param_source;
	src.min_barcode_phred = _min_barcode_phred;
	std::istringstream names(filenames);
	std::string name;
	while (names >> name) {
		gzFile f = gzopen(name.c_str(), "rb");
		if (!f) throw std::runtime_error("Can't open file with read parameters'" + name + "'");
		(void)gzbuffer(f, 1u << 20);
		const size_t begin = src.text.size();
		for (;;) {
			const size_t at = src.text.size(), chunk = size_t(8) << 20;
			src.text.resize(at + chunk);
			const int got = gzread(f, src.text.data() + at, unsigned(chunk));
			src.text.resize(at + size_t(std::max(got, 0)));
			if (got <= 0) break;
		}
		gzclose(f);
		src.file_lines.push_back(src.lines());
		const uint8_t *const p = src.text.data();
		for (size_t at = begin, end = src.text.size(); at < end;) {
			const void *nl = std::memchr(p + at, '\n', end - at);
			const size_t next = nl ? size_t(static_cast<const uint8_t *>(nl) - p) + 1 : end;
			src.line_be.push_back(at); src.line_be.push_back(next);
			at = next;
		}
	}
	src.file_lines.push_back(src.lines());
}

// The host reader's map, built when it first takes a file: malformed rows are skipped, a repeated name keeps its first row.  Rows that the
// device path's table has served by then (files it took before this one) are consumed: they do not enter the map.
void BamController::map_read_params() {
	if (_read_params_mapped) return;
	_read_params_mapped = true;
	ParamSource &src = *_param_source;
	const std::vector<uint8_t> consumed = consumed_read_params(src);
	_read_params.reserve(src.lines());
	ParamSource::Row r;
	for (size_t k = 0; k < src.lines(); ++k) {
		if (!src.row(k, r)) continue;      // "can't parse read parameters from string", or the ReadParameters constructor throws: skipped
		const auto in = _read_params.emplace(std::string(r.name), ReadParams{std::string(r.cb), std::string(r.umi), std::string(r.umi_quality), r.pass});
		if (in.second && !consumed.empty() && consumed[k]) in.first->second.cb.clear();      // (the first row of a name is the table's canonical one; dropped below)
	}
	if (!consumed.empty())
		for (auto it = _read_params.begin(); it != _read_params.end();) { if (it->second.cb.empty()) it = _read_params.erase(it); else ++it; }
	src.host_served = true;
	if (!_device_read_sources) { std::vector<uint8_t>().swap(src.text); std::vector<uint64_t>().swap(src.line_be); }      // (nobody spells rows from the text any more)
}

// the workers: one record after the other of the worker's range parsed, counted and, if accepted, packed; what it brings new is noted
void BulkWindow::parse_and_pack(const uint8_t *data, const std::vector<uint32_t> &offsets, size_t n) {
	const unsigned NT = workers.size();
	const bool own_gene = !parser.genes.is_empty();
	const uint32_t *const off = offsets.data();
	workers.run([this, data, off, n, NT, own_gene](unsigned t) {
		Parsed tmp;
		std::vector<Need> &mine = needs[t];
		mine.clear();
		Tally tl;
		size_t at = n * t / NT;
		for (size_t i = n * t / NT; i < n * (t + 1) / NT; ++i) {
			parser.parse(data + off[i], tmp);
			if (!count_status(tl, tmp.status)) continue;
			const CellsDataContainer::ParsedRead &r = tmp.r;
			const bool has_gene = !r.gene.empty();
			o_qp[at] = has_gene ? r.umi_quality.data() : nullptr;
			if (has_gene) { if (tl.ql == NO_QL) tl.ql = r.umi_quality_length; else if (tl.ql != r.umi_quality_length) tl.mixed = true; }
			uint8_t what = 0;
			o_cb[at] = r.cb_code; if (!r.cb_code) what |= NEED_CB;
			if (has_gene) {
				o_umi[at] = r.umi_code; if (!r.umi_code) what |= NEED_UMI;
				if (r.gene_id >= 0) o_gene[at] = uint32_t(r.gene_id); else what |= NEED_GENE;
			} else { o_umi[at] = 1; o_gene[at] = DROPEST_NO_GENE; }
			const bool touches = !has_gene || (r.mark & (UMI::Mark::HAS_EXONS | UMI::Mark::HAS_INTRONS));
			uint32_t aux = uint32_t(r.mark) << 16;
			if (touches) {
				const int chr = container.chromosome_of_ref(r.ref_id);   // (the dictionaries are read-only while the workers run)
				if (chr >= 0) aux |= uint32_t(chr); else what |= NEED_CHR;
			}
			o_aux[at] = aux;
			if (what) mine.push_back(Need{uint32_t(at), NewParts{what, r.ref_id, r.cb, r.umi, r.gene, r.gene_hash}, (what & NEED_GENE) && own_gene ? std::string(r.gene) : std::string()});
			++at;
		}
		tally[t] = tl;
	});
}

// one row of ql bytes per accepted read, beside the columns (zeros for reads without a gene)
void BulkWindow::add_with_quality_rows(size_t n, uint32_t ql) {
	const unsigned NT = workers.size();
	container.reserve_quality_rows(est_reads, ql);
	if (o_qual.size() < n * size_t(ql)) o_qual.resize(n * size_t(ql));
	workers.run([this, n, NT, ql](unsigned t) {
		const size_t b0 = n * t / NT;
		for (size_t k = 0; k < tally[t].saved; ++k) {
			uint8_t *row = o_qual.data() + (b0 + k) * size_t(ql);
			if (o_qp[b0 + k]) std::memcpy(row, o_qp[b0 + k], ql); else std::memset(row, 0, ql);
		}
	});
	q_rows.clear();
	for (unsigned t = 0; t < NT; ++t) if (tally[t].saved) q_rows.push_back(o_qual.data() + (n * t / NT) * size_t(ql));
	container.add_records_packed(runs, q_rows, ql);
}

bool BulkWindow::ingest(const uint8_t *data, const std::vector<uint32_t> &offsets, size_t n) {
	const unsigned NT = workers.size();
	auto t_phase = clk::now();
	auto phase = [&](int k) { ms[k] += since(t_phase); t_phase = clk::now(); };
	if (o_cb.size() < n) { o_cb.resize(n); o_umi.resize(n); o_gene.resize(n); o_aux.resize(n); o_qp.resize(n); }   // (never shrunk: no refill per window)
	parse_and_pack(data, offsets, n);
	phase(0);
	uint32_t ql = NO_QL;
	for (unsigned t = 0; t < NT; ++t) {
		if (tally[t].mixed) return false;
		if (tally[t].ql == NO_QL) continue;
		if (ql == NO_QL) ql = tally[t].ql; else if (ql != tally[t].ql) return false;
	}
	const bool with_quality = ql != NO_QL && ql > 0;
	if (with_quality ? !container.bulk_ingest_possible_with_quality(ql) : !container.bulk_ingest_possible()) return false;
	// in file order: what the dictionaries have not seen (intern_new)
	for (unsigned t = 0; t < NT; ++t)
		for (Need &nd : needs[t]) {
			if (!nd.gene_owned.empty()) nd.p.gene = nd.gene_owned;
			intern_new(container, nd.p, o_cb[nd.idx], o_umi[nd.idx], o_gene[nd.idx], o_aux[nd.idx]);
		}
	phase(1);
	runs.clear();
	for (unsigned t = 0; t < NT; ++t) {
		const size_t b0 = n * t / NT;
		if (tally[t].saved) runs.push_back(CellsDataContainer::PackedRun{o_cb.data() + b0, o_umi.data() + b0, o_gene.data() + b0, o_aux.data() + b0, tally[t].saved});
	}
	if (with_quality) add_with_quality_rows(n, ql);
	else container.add_records_packed(runs);
	phase(2);
	for (unsigned t = 0; t < NT; ++t) {
		counters.total_reads += tally[t].total_reads; counters.cant_parse += tally[t].cant_parse; counters.low_quality += tally[t].low_quality; counters.saved += tally[t].saved;
	}
	return true;
}

// -r: ReadMapParamsParser::get_read_params (:22-48) comes BEFORE the gene look-up (BamController.cpp:140-152):
// an unknown name is "can't parse", a served name is erased, its quality verdict precedes the gene's
void BamController::serve_read_params(Parsed &pr) {
	if (pr.status == Parsed::SKIP || pr.status == Parsed::CANT_PARSE_NO_COUNT) return;
	std::string_view nm = pr.name;
	if (!nm.empty() && nm[0] == '@') nm.remove_prefix(1);
	auto it = _read_params.find(std::string(nm));
	if (it == _read_params.end()) { pr.status = Parsed::CANT_PARSE; return; }
	const bool pass = it->second.pass_quality;
	pr.p_cb = std::move(it->second.cb); pr.p_umi = std::move(it->second.umi); pr.p_quality = std::move(it->second.umi_quality);
	_read_params.erase(it);
	if (!pass) pr.status = Parsed::LOW_QUALITY;
	else if (pr.status == Parsed::OK) {
		pr.r.cb = pr.p_cb; pr.r.umi = pr.p_umi; pr.r.umi_quality = pr.p_quality; pr.r.umi_quality_length = uint32_t(pr.p_quality.size());
		if (!CellsDataContainer::pack_code(pr.r.cb, pr.r.cb_code)) pr.r.cb_code = 0;
		if (!CellsDataContainer::pack_code(pr.r.umi, pr.r.umi_code)) pr.r.umi_code = 0;
	}
}

// A window of the host reader record by record: parsed side by side, then in file order into the counters and the container
// (first-seen ids are defined by this order)
void BamController::add_record_by_record(FileIngest &file, const uint8_t *data, const std::vector<uint32_t> &offsets, std::vector<Parsed> &parsed) {
	const auto t_parse = clk::now();
	const size_t n = offsets.size();
	parsed.resize(n);
	const unsigned nt = unsigned(std::min<size_t>(file.bulk.threads(), std::max<size_t>(1, n / 2048)));
	std::vector<std::thread> pool;
	std::vector<std::string> errors(nt);
	const RecordParser &parser = file.parser;
	const uint32_t *const off = offsets.data();
	Parsed *const out = parsed.data();
	for (unsigned t = 0; t < nt; ++t)
		pool.emplace_back([&parser, &errors, data, off, out, n, nt, t] {
			try { for (size_t i = n * t / nt; i < n * (t + 1) / nt; ++i) parser.parse(data + off[i], out[i]); }
			catch (const std::exception &e) { errors[t] = e.what(); }
		});
	for (auto &th : pool) th.join();
	for (auto const &e : errors) if (!e.empty()) throw std::runtime_error(e + ": " + file.bam_name);
	_counters.parse_ms += since(t_parse);
	const auto t_add = clk::now();
	for (size_t i = 0; i < n; ++i) {
		if (_params_from_files) serve_read_params(parsed[i]);
		if (count_status(_counters, parsed[i].status)) file.container.add_record(parsed[i].r);
	}
	_counters.add_ms += since(t_add);
}

// The host reader: BamReader inflates and finds the records, a window at a time
void BamController::read_file_on_host(FileIngest &file, bool first_file) {
	if (_params_from_files) map_read_params();
	BamReader reader(file.bam_name, _threads);       // opened only when it is the one that reads (its loader thread inflates ahead from the start)
	CellsDataContainer &container = file.container;
	file.refs = reader.reference_names();
	container.set_reference_names(file.refs);
	const uint8_t *data = nullptr;
	std::vector<uint32_t> offsets;
	std::vector<Parsed> parsed;
	bool first_window = true;
	for (;;) {
		const auto t_wait = clk::now();
		if (!reader.next_window(data, offsets)) break;
		_counters.wait_ms += since(t_wait);
		if (first_window && first_file) {
			// a container over several GPUs deals contiguous ranges of the stream to its shards: tell it how long the stream
			// will roughly be (records of the first window x file bytes / bytes the window covered, x the number of files)
			file.bulk.est_reads = size_t(double(offsets.size()) * reader.file_over_first_batch() * double(file.n_files) * 1.05);
			container.expect_reads(file.bulk.est_reads);
		}
		first_window = false;
		if (!_params_from_files && !file.sw.record_by_record && file.bulk.threads() <= 256 && container.bulk_ingest_possible_at_all()) {
			const auto t_fast = clk::now();
			const bool done = file.bulk.ingest(data, offsets, offsets.size());
			_counters.parse_ms += since(t_fast);
			if (done) continue;
		}
		add_record_by_record(file, data, offsets, parsed);
	}
	file.sw.trace("[bam] bulk windows: parse + pack on the workers %.1f ms, new dictionary entries %.1f ms, container %.1f ms\n", file.bulk.ms[0], file.bulk.ms[1], file.bulk.ms[2]);
}

void BamController::parse_bam_files(const std::vector<std::string> &bam_files, CellsDataContainer &container) { parse_bam_files(bam_files, false, container); }

void BamController::parse_bam_files(const std::vector<std::string> &bam_files, bool print_result_bams, CellsDataContainer &container) {
	const BamSwitches sw = BamSwitches::from_environment();
	_tagged.clear();
	_saved_per_file.clear();
	const bool source_output = _device_read_sources && _device_source_output;      // -b / -F under -r and -P: the tag kernels read the row and the reference's name
	if (print_result_bams) {      // what the device path refuses, said before any file is read: the host reader does not write BAM
		const char *why = nullptr;
		if (_params_from_files && !source_output) why = "read-parameter files (-r) are served by the host reader";
		else if (_gene_in_chromosome_name && !source_output) why = "gene = chromosome name is resolved by the host reader";
		else if (_tags.intronic_read_value.size() > 24 || _tags.intergenic_read_value.size() > 24 || _tags.exonic_read_value.size() > 24) why = "a read-type value is longer than 24 bytes";
		if (why) throw std::runtime_error(std::string("Tagged BAM output (-b) is written on the device BAM path only, which this configuration cannot take: ") + why);
		_tagged.reserve(bam_files.size());
	}
	const unsigned nthreads = _threads ? _threads : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
	struct SayAll { const BamSwitches &sw; clk::time_point t; ~SayAll() { sw.trace("[bam] parse_bam_files: %.1f ms\n", since(t)); } } say_all{sw, clk::now()};
	join_release_thread();
	for (auto const &bam_name : bam_files) {
		FileIngest file(sw, bam_name, bam_files.size(), container, _counters, _tags, _filled_bam, _params_from_files, _gene_in_chromosome_name, _min_barcode_phred, _genes, nthreads);
		file.device_sources = _device_read_sources && (!print_result_bams || source_output);
		file.source_output = source_output;
		if (file.device_sources && _params_from_files && !_param_source->host_served && !_param_source->text.empty()) file.params = _param_source.get();
		struct NoteSaved { std::vector<size_t> &per_file; const Counters &c; size_t before; ~NoteSaved() { per_file.push_back(c.saved - before); } } note{_saved_per_file, _counters, _counters.saved};
		if (print_result_bams) { _tagged.emplace_back(); file.tagged = &_tagged.back(); }
		if (print_result_bams || _device_decode || sw.device) {
			const auto t_df = clk::now();
			const bool done = read_file_on_device(file);
			sw.trace("[bam] device path: %.1f ms in all for this file (taken: %d)\n", since(t_df), int(done));
			if (done) continue;
			if (print_result_bams)
				throw std::runtime_error("Tagged BAM output (-b) is written on the device BAM path only, which cannot take this file: " + (file.refusal.empty() ? std::string("unknown reason") : file.refusal) + ": " + bam_name);
		}
		read_file_on_host(file, &bam_name == &bam_files.front());
	}
	// the device decoders' memory goes back before the container sorts (the cache was never released)
	if (!sw.keep_decoders) release_decoders_in_background();
}

// -F: the second pass over the files (bam_ingest.h); every file through the device path in its filtered mode (bam_device.cpp)
void BamController::write_filtered_bam_files(const std::vector<std::string> &bam_files, CellsDataContainer &container) {
	const BamSwitches sw = BamSwitches::from_environment();
	_filtered = FilteredFile();
	const bool source_output = _device_read_sources && _device_source_output;
	const char *why = nullptr;
	if (_params_from_files && !source_output) why = "read-parameter files (-r) are served by the host reader";
	else if (_gene_in_chromosome_name && !source_output) why = "gene = chromosome name is resolved by the host reader";
	else if (_tags.intronic_read_value.size() > 24 || _tags.intergenic_read_value.size() > 24 || _tags.exonic_read_value.size() > 24) why = "a read-type value is longer than 24 bytes";
	if (why) throw std::runtime_error(std::string("Filtered BAM output (-F) is written on the device BAM path only, which this configuration cannot take: ") + why);
	if (bam_files.empty()) return;
	join_release_thread();
	FilteredPass *pass = filtered_pass_open(sw, container, _filtered, _sharded_filtered_output);
	Counters second_pass;      // (the reads were counted when the container was filled)
	try {
		// did this controller fill the container?  Then file k brings what it brought then (a count guard per file: it sees files in another order)
		size_t remembered = 0;
		for (size_t n : _saved_per_file) remembered += n;
		const bool per_file = !_saved_per_file.empty() && remembered == filtered_pass_total(pass);
		for (auto const &bam_name : bam_files) {
			const uint64_t before = filtered_pass_reads(pass);
			const size_t k = size_t(&bam_name - &bam_files.front());
			FileIngest file(sw, bam_name, bam_files.size(), container, second_pass, _tags, _filled_bam, _params_from_files, _gene_in_chromosome_name, _min_barcode_phred, _genes, 1);
			file.filtered = pass;
			file.device_sources = file.source_output = source_output;
			if (source_output && _params_from_files && !_param_source->host_served && !_param_source->text.empty()) file.params = _param_source.get();
			if (!read_file_on_device(file))
				throw std::runtime_error("Filtered BAM output (-F) is written on the device BAM path only, which cannot take this file: " + (file.refusal.empty() ? std::string("unknown reason") : file.refusal) + ": " + bam_name);
			const uint64_t brought = filtered_pass_reads(pass) - before;
			if (per_file && (k >= _saved_per_file.size() || brought != _saved_per_file[k]))
				filtered_pass_other_files(pass, bam_name + " brings " + std::to_string(brought) + " accepted reads, file " + std::to_string(k + 1) + " of the call that filled the container brought " +
				                                (k < _saved_per_file.size() ? std::to_string(_saved_per_file[k]) : std::string("none")));
		}
	} catch (...) {
		filtered_pass_close(pass, false);
		if (!sw.keep_decoders) release_decoders_in_background();
		throw;
	}
	filtered_pass_close(pass, true);
	if (!sw.keep_decoders) release_decoders_in_background();
}

}  // namespace BamProcessing
}  // namespace Estimation
