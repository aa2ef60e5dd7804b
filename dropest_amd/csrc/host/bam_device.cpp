// bam_device.cpp -- the device path of BamController::parse_bam_files (bam_ingest.h; include/dropest_bgzf.h; DROPEST_BAM_DEVICE=1 or
// BamController::set_device_decode).
// The decoder behind that header: csrc/bam_decoder.h, bam_decoder_dict.h, bam_decoder_upload.h, bam_decoder_window.h, bam_decoder_fetch.h and bam_decoder_tag.h, compiled as parts of
// csrc/bgzf_api.hip; the block table it takes from this file's walks is bgzf::BlockTable (bgzf_blocks.h).
// The blocks are inflated on the GPU (csrc/k_inflate.h: a wave per block), the chain of records is found and every record's tags
// are walked there (csrc/k_bamparse.h: a lane per record); 39 bytes per record come back instead of the ~300 of the record.  The
// dictionaries stay here: the workers turn gene hashes and reference ids into indices, and the records that bring something NEW
// (a gene name, a chromosome, a string with N) are fetched as bytes and go through RecordParser + intern_new in file order,
// exactly like the Needs of BulkWindow.  Windows grow from 1 MB of compressed bytes (the first ones meet most gene names).
// Every block's CRC-32 is checked on the device (the wave that inflated it reads it back).  Falls back to the host reader (returns false before anything was added) when
// the configuration needs what the kernels do not do: -r parameter files and gene = chromosome name unless BamController::set_device_read_sources
// is on.  With it, -r is a table on the device (ParamSource::table_on; csrc/k_readparams.h) that every record's name is looked up in and that
// serves each row once, to the first record of the stream that asks -- the decoder says which row each record was served, and the strings of the
// few records the host must see are spelled from the row's line; -P is a table reference -> gene index (gene_of_reference_to_device).
// Behind BamController::set_device_source_output the two outputs below are written under -r and -P too: the tag kernels read the served row's
// strings from the table and the reference's name from a table of names (tagging_to_decoder), and the -F pass serves the rows afresh on claims of
// its own (filtered_pass_replay .. filtered_pass_close).
// Tagged BAM output (-b: parse_bam_files(files, true, container)) is made here and only here: every window's accepted records are edited on the device
// (csrc/k_bamtag.h) before the window goes into the container, compressed there and written to `<input stem>.tagged.bam` (open_tagged, tag_window,
// close_tagged); a file this path refuses is then an error that names the reason (FileIngest::refusal), not a file for the host reader.
// Filtered BAM output (-F: BamController::write_filtered_bam_files) is this path's second mode (FileIngest::filtered): the files are decoded again,
// nothing goes into the container, every window's accepted records are edited by the tag kernels' filtered mode under the container's per-read
// decisions (dropest_bam_decoder_filter_window; the decisions stay on the device) and ONE compressor stream writes the one output of the call
// (FilteredPass, open_filtered, filter_window, close_filtered).  Over a sharded or split container (BamController::set_sharded_filtered_output; off:
// refused) the decisions are the shards': FilteredPass holds every shard's range of the stream and its three device arrays, filter_window cuts
// [at, at + n_accepted) at the ranges' boundaries and hands the pieces to dropest_bam_decoder_filter_window_segments, each file's decoder sits on
// the GPU and stream of the shard that holds the file's first read, and the compressor follows the decoder from one stream to the next.
// A sharded container is fed the same way: ONE decoder, on the GPU of the shard the file's first read goes to and on that shard's stream, for the
// whole file (the record cut off at a window's end waits inside it); the container cuts every window at its quota boundaries and appends the
// pieces to the shards' resident reads, device to device.
#include "bam_parse.h"
#include "../../../include/dropest_bgzf.h"
#include "../../../include/dropest_annotation.h"
#include "../../../include/dropest_deflate.h"
#include "../../../include/dropest_amd.h"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>

#include <atomic>
#include <memory>

namespace Estimation {
namespace BamProcessing {

namespace {
std::mutex &decoder_cache_mutex() { static std::mutex m; return m; }
std::unordered_map<int, dropest_bam_decoder *> &decoder_cache() { static auto *c = new std::unordered_map<int, dropest_bam_decoder *>(); return *c; }   // (never destroyed: the HIP runtime may be gone by then)
// The decoders of the files just read go back on a helper thread (several GB of device buffers and up to 512 MB of pinned staging: ~40 ms of
// hipFree / hipHostFree that the container's passes need not wait for).  Joined before the next file list, by release_device_decoders(), and
// at exit before the HIP runtime goes down (std::atexit handlers run in reverse order of registration, and the runtime registered first).
std::thread *&release_thread() { static std::thread *t = nullptr; return t; }
}  // namespace

void join_release_thread() {
	std::thread *t = nullptr;
	{ std::lock_guard<std::mutex> lk(decoder_cache_mutex()); t = release_thread(); release_thread() = nullptr; }
	if (t) { if (t->joinable()) t->join(); delete t; }
}
void release_decoders_in_background() {
	join_release_thread();
	std::lock_guard<std::mutex> lk(decoder_cache_mutex());
	if (decoder_cache().empty()) return;
	std::vector<dropest_bam_decoder *> gone;
	for (auto &kv : decoder_cache()) gone.push_back(kv.second);
	decoder_cache().clear();
	static const bool at_exit = (std::atexit(join_release_thread), true);
	(void)at_exit;
	release_thread() = new std::thread([gone] { for (dropest_bam_decoder *d : gone) dropest_bam_decoder_destroy(d); });
}

void BamController::release_device_decoders() {
	join_release_thread();
	std::lock_guard<std::mutex> lk(decoder_cache_mutex());
	for (auto &kv : decoder_cache()) dropest_bam_decoder_destroy(kv.second);
	decoder_cache().clear();
}

// -r: the controller's rows as a table on `device` (made on first use; one table, on one GPU: the claims that make a row serve once live with it)
dropest_read_params *ParamSource::table_on(int device) {
	if (table) return device == table_device ? table : nullptr;
	dropest_read_params *t = nullptr;
	if (dropest_read_params_create(device, 0, &t)) return nullptr;
	std::vector<uint64_t> off;
	for (size_t f = 0; f + 1 < file_lines.size(); ++f) {      // a call per file: a file's last line ends with the file
		const size_t l0 = size_t(file_lines[f]), l1 = size_t(file_lines[f + 1]);
		if (l0 == l1) continue;
		const uint64_t begin = line_be[2 * l0], end = line_be[2 * l1 - 1];
		off.resize(l1 - l0);
		for (size_t k = l0; k < l1; ++k) off[k - l0] = line_be[2 * k] - begin;
		if (dropest_read_params_add_text(t, text.data() + begin, end - begin, off.data(), l1 - l0, min_barcode_phred)) { dropest_read_params_destroy(t); return nullptr; }
	}
	if (dropest_read_params_build(t)) { dropest_read_params_destroy(t); return nullptr; }
	table = t; table_device = device;
	return table;
}
ParamSource::~ParamSource() { if (table) dropest_read_params_destroy(table); }

std::vector<uint8_t> consumed_read_params(ParamSource &src) {
	std::vector<uint8_t> consumed;
	if (!src.table) return consumed;
	std::vector<uint64_t> claims(src.lines());
	if (dropest_read_params_claims_to_host(src.table, 0, claims.size(), claims.data())) throw std::runtime_error(std::string("read parameters: ") + dropest_bgzf_last_error());
	consumed.resize(claims.size());
	for (size_t k = 0; k < claims.size(); ++k) consumed[k] = claims[k] != ~uint64_t(0);
	return consumed;
}

// -F: what the files of one write_filtered_bam_files call share (bam_parse.h)
struct FilteredPass {
	const BamSwitches &sw;
	CellsDataContainer &container;
	BamController::FilteredFile &report;
	const uint8_t *d_verdict = nullptr; const uint32_t *d_cell = nullptr; const uint64_t *d_umi = nullptr;      // dropest_read_corrections: device arrays of the context
	const uint64_t *d_cell_codes = nullptr;                                                                     // dropest_cell_barcodes_device
	uint64_t n_reads = 0, n_cells = 0, at = 0, written = 0;      // at: accepted records of the files so far = the next window's first decision
	uint64_t counts[5] = {0, 0, 0, 0, 0};
	std::vector<uint32_t> side_off; std::vector<uint8_t> side_pool;      // the container's side strings as the decoder takes them
	// The second shape, a sharded or split container (BamController::set_sharded_filtered_output): no array holds every read's decision --
	// shard k holds those of reads [first, first + n) of the stream, the range it reports itself (dropest_shard_read_corrections after ONE
	// dropest_shard_group_read_corrections over all shards), on its GPU; `column` plays the part of `cell`: it indexes the columns that
	// dropest_shard_filtered_barcodes_device names (the same list on every shard; each file's decoder takes the copy of the shard it sits with).
	struct Piece { dropest_shard *shard; int device; void *stream; uint64_t first, n; const uint8_t *verdict; const uint32_t *column; const uint64_t *umi; };
	std::vector<Piece> pieces;
	size_t cur = 0;                  // the shard the current file's decoder sits with: the one that holds the file's first read
	std::string name;
	ParamSource *replay = nullptr;   // -r: the table's claims are the pass's own (filtered_pass_replay) until end_replay puts the ingest's back
	uint64_t ingest_ordinal = 0;     // ... and the ordinal the ingest had come to
	std::FILE *f = nullptr;
	dropest_deflate_stream *z = nullptr;
	int z_device = -1; void *z_stream = nullptr;      // where the compressor runs: the decoder's GPU and stream
	uint64_t z_in = 0, z_out = 0, z_batches = 0;      // what the compressors that are through took and gave
	double z_ms = 0;
	size_t windows = 0;
	double decode_ms = 0, tag_ms = 0, decisions_ms = 0;
	FilteredPass(const BamSwitches &sw, CellsDataContainer &container, BamController::FilteredFile &report) : sw(sw), container(container), report(report) {}
	~FilteredPass() { (void)end_replay(); if (z) dropest_deflate_stream_destroy(z); if (f) std::fclose(f); }
	bool end_replay() {
		if (!replay) return true;
		ParamSource *const src = replay;
		replay = nullptr;
		src->ordinal = ingest_ordinal;
		return dropest_read_params_replay_end(src->table) == 0;
	}
	static int write(const uint8_t *bytes, uint64_t len, void *user) { return std::fwrite(bytes, 1, size_t(len), static_cast<FilteredPass *>(user)->f) == size_t(len) ? 0 : 1; }
	[[noreturn]] void other_files(const std::string &what) const {
		throw std::runtime_error("Filtered BAM output (-F): " + what + ": these are not the files the container was filled from (the same files, in the same order)");
	}
	// the compressor's leftover goes out (flags: DROPEST_DEFLATE_EOF behind the last one), its account is kept and it goes
	void retire_compressor(int flags) {
		if (dropest_deflate_stream_finish(z, flags)) throw std::runtime_error(std::string(dropest_deflate_last_error()) + ": " + name);
		uint64_t in = 0, out = 0, batches = 0;
		double ms = 0;
		(void)dropest_deflate_stream_stats(z, &ms, &in, &out, &batches);
		z_in += in; z_out += out; z_batches += batches; z_ms += ms;
		dropest_deflate_stream_destroy(z); z = nullptr;
	}
	// sharded: the shard whose range holds read `ordinal` (past the last read, or no reads at all: the last shard that has any, else the first)
	size_t shard_of(uint64_t ordinal) const {
		size_t last = 0;
		for (size_t k = 0; k < pieces.size(); ++k) {
			if (!pieces[k].n) continue;
			if (ordinal >= pieces[k].first && ordinal - pieces[k].first < pieces[k].n) return k;
			last = k;
		}
		return last;
	}
};

// -F over the shards: every shard's decisions and the range it holds, the summed counts
static void shards_decisions(FilteredPass &p, CellsDataContainer &container) {
	const std::vector<dropest_shard *> &shards = container.shards();
	auto refuse = [] { throw std::runtime_error(std::string("Filtered BAM output (-F): ") + dropest_last_error()); };      // (the shards' own words)
	if (dropest_shard_group_read_corrections(shards.data(), int32_t(shards.size())) != DROPEST_OK) refuse();
	uint64_t base = 0;
	for (size_t k = 0; k < shards.size(); ++k) {
		FilteredPass::Piece q{shards[k], container.shard_device(k), dropest_stream(dropest_shard_ctx(shards[k])), 0, 0, nullptr, nullptr, nullptr};
		if (dropest_shard_read_corrections(q.shard, &q.n, &q.first, &q.verdict, &q.column, &q.umi) != DROPEST_OK) refuse();
		// (the ranges ascend with the rank and leave no gap: a window is cut where they meet)
		if (q.n && q.first != base) throw std::runtime_error("Filtered BAM output (-F): internal: shard " + std::to_string(k) + " holds the reads from " + std::to_string(q.first) + " on, the shards before it end at " + std::to_string(base));
		if (!q.n) q.first = base;
		base += q.n;
		p.pieces.push_back(q);
	}
	p.n_reads = base;
	if (dropest_shard_group_read_correction_counts(shards.data(), int32_t(shards.size()), p.counts) != DROPEST_OK) refuse();
	const uint64_t *codes = nullptr;
	if (dropest_shard_filtered_barcodes_device(shards[0], &p.n_cells, &codes) != DROPEST_OK) refuse();      // (n_cells: the columns; every file asks its own shard for the array)
}

FilteredPass *filtered_pass_open(const BamSwitches &sw, CellsDataContainer &container, BamController::FilteredFile &report, bool sharded_output) {
	// (a sharded or split container has no one context that holds every read: without the switch a shard's context says so in the read
	// corrections' own words)
	dropest_ctx *const ctx = container.sharded() ? dropest_shard_ctx(container.shard0()) : container.handle();
	std::unique_ptr<FilteredPass> p(new FilteredPass(sw, container, report));
	const auto t_open = clk::now();
	struct Note { double &ms; clk::time_point t; ~Note() { ms = since(t); } } note{p->decisions_ms, t_open};
	if (container.sharded() && sharded_output) shards_decisions(*p, container);
	else if (!ctx || dropest_read_corrections(ctx, &p->n_reads, &p->d_verdict, &p->d_cell, &p->d_umi) != DROPEST_OK ||
	    dropest_cell_barcodes_device(ctx, &p->n_cells, &p->d_cell_codes) != DROPEST_OK || dropest_read_correction_counts(ctx, p->counts) != DROPEST_OK)
		throw std::runtime_error(std::string("Filtered BAM output (-F): ") + (ctx ? dropest_last_error() : "the container holds no reads"));
	if (p->n_cells > 0xFFFFFFFFull) throw std::runtime_error("Filtered BAM output (-F): more than 2^32 cells");
	const std::vector<std::string> &side = container.side_strings();
	p->side_off.push_back(0);
	for (const std::string &s : side) { p->side_pool.insert(p->side_pool.end(), s.begin(), s.end()); p->side_off.push_back(uint32_t(p->side_pool.size())); }
	if (p->side_pool.size() > 0xFFFFFFF0ull) throw std::runtime_error("Filtered BAM output (-F): the side strings pass 4 GB");
	p->side_pool.push_back(0);
	return p.release();
}

void filtered_pass_replay(FilteredPass *pass, ParamSource &params) {
	if (pass->replay) return;
	if (dropest_read_params_replay_begin(params.table)) throw std::runtime_error(std::string("Filtered BAM output (-F): read parameters: ") + dropest_bgzf_last_error());
	pass->replay = &params; pass->ingest_ordinal = params.ordinal;
	params.ordinal = 0;
}

uint64_t filtered_pass_reads(const FilteredPass *pass) { return pass->at; }
uint64_t filtered_pass_total(const FilteredPass *pass) { return pass->n_reads; }
void filtered_pass_other_files(const FilteredPass *pass, const std::string &what) { pass->other_files(what); }

void filtered_pass_close(FilteredPass *pass, bool ok) {
	std::unique_ptr<FilteredPass> p(pass);
	BamController::FilteredFile &r = p->report;
	r = BamController::FilteredFile();
	auto drop = [&] {      // no half-written file, no half-written claim
		if (p->z) { dropest_deflate_stream_destroy(p->z); p->z = nullptr; }
		if (p->f) { std::fclose(p->f); p->f = nullptr; std::remove(p->name.c_str()); }
	};
	const bool claims_back = p->end_replay();      // (first thing, and whichever way the pass ended: the ingest's claims are the table's again)
	if (!ok) { drop(); return; }
	try {
		if (!claims_back) throw std::runtime_error(std::string("Filtered BAM output (-F): read parameters: ") + dropest_bgzf_last_error());
		if (p->at != p->n_reads) p->other_files("the files hold " + std::to_string(p->at) + " accepted reads, the container " + std::to_string(p->n_reads));
		if (p->written != p->counts[0]) throw std::runtime_error("internal: " + std::to_string(p->written) + " reads were written to the filtered BAM file, the container's decisions write " + std::to_string(p->counts[0]));
		if (!p->z) throw std::runtime_error("internal: no filtered BAM file was opened");
		p->retire_compressor(DROPEST_DEFLATE_EOF);
		const uint64_t in = p->z_in, out = p->z_out, batches = p->z_batches;
		const double deflate_ms = p->z_ms;
		const bool closed = std::fclose(p->f) == 0;
		p->f = nullptr;
		if (!closed) { std::remove(p->name.c_str()); throw std::runtime_error("Can't write filtered BAM file: " + p->name); }
		r.name = p->name; r.windows = p->windows; r.total_reads = size_t(p->at); r.written = size_t(p->written);
		r.wrong_genes = size_t(p->counts[3]); r.wrong_umis = size_t(p->counts[4]);
		r.inflated_bytes = size_t(in); r.compressed_bytes = size_t(out); r.batches = size_t(batches);
		r.decode_ms = p->decode_ms; r.tag_ms = p->tag_ms; r.deflate_ms = deflate_ms; r.decisions_ms = p->decisions_ms;
	} catch (...) { drop(); throw; }
}

namespace {

int host_inflate(const uint8_t *in, uint32_t in_len, uint8_t *out_bytes, uint32_t out_len, void *) {
	RawBlock b; b.cdata = in; b.clen = in_len; b.isize = out_len; b.crc = le32(in + in_len);
	try { inflate_block(b, out_bytes); } catch (...) { return 1; }
	return 0;
}

// (d) How large the windows of one file are: pure arithmetic over the file's size, its first blocks and the switches.
struct WindowPlan {
	size_t window_max = 0, window_blocks = 0, block_cap = 0, stage_cap = 0;
	size_t inflated_seen = 0, compressed_seen = 0;      // over the first 64 blocks behind the header: how far this file inflates
	size_t avg_block = size_t(1) << 14;
	uint32_t n_pieces = 0;
};
WindowPlan plan_windows(const BamSwitches &sw, const uint8_t *p, size_t n, size_t c0, size_t wave_slots) {
	WindowPlan w;
	// windows: a machine's worth of blocks (one wave per block) in a file of a few hundred MB, two in a long one (measured on 0.4 and 1.6 GB:
	// NOTES_r05 §11) -- the pinned staging buffers of larger windows cost more to allocate than their fuller kernels give back
	const bool long_file = n > (size_t(1) << 30);
	w.window_max = (sw.has_window_mb ? sw.window_mb : size_t(long_file ? 80 : 48)) << 20;
	// (DROPEST_BAM_WINDOW_BLOCKS: blocks per window instead of the device's wave slots, twice that in a long file)
	w.window_blocks = sw.has_window_blocks ? sw.window_blocks : std::max<size_t>(1024, wave_slots) * (long_file ? 2 : 1);
	if (!sw.has_window_mb) {
		// ... of blocks, not of bytes: a file that deflates 3 x (real bases and qualities) has blocks of ~20 KB where the 10 x synthetic ones have 6 KB,
		// and a window of 48 MB of them would fill a third of the wave slots -- each window takes the time of ONE block however many it holds.
		// The blocks behind the header say how large they are; up to 128 / 256 MB of staging (9.5 ms of pinning per 48 MB: NOTES_r05 section 13).
		// (the laxest walk: two magic bytes, and a BC subfield may end beyond XLEN)
		size_t at = c0, n_seen = 0, bytes_seen = 0;
		while (n_seen < 64 && at + 18 <= n && p[at] == 31 && p[at + 1] == 139) {
			const size_t bsize = bgzf::parse_header(p + at, n - at).bsize_cut;
			if (!bsize || at + bsize > n) break;
			w.inflated_seen += le32(p + at + bsize - 4);
			at += bsize; bytes_seen += bsize; ++n_seen;
		}
		w.compressed_seen = bytes_seen;
		if (n_seen >= 8) {
			const size_t want = w.window_blocks * (bytes_seen / n_seen + 1);
			w.window_max = std::min(std::max(w.window_max, want), size_t(sw.has_window_blocks ? 512 : long_file ? 256 : 128) << 20);
			w.window_max = std::min(w.window_max, std::max<size_t>(n - c0, size_t(1) << 20));      // (no more than the file)
		}
	}
	w.stage_cap = w.window_max + (size_t(1) << 17);
	w.block_cap = sw.has_window_mb ? size_t(-1) : w.window_blocks;   // (one wave per block: a full machine's worth per window)
	w.avg_block = w.compressed_seen >= 64 ? std::max<size_t>(w.compressed_seen / 64, 64) : size_t(1) << 14;
	// (the copy out of the page cache runs at ~4-5 GB/s per thread; a piece being sent, one being filled, per reader)
	w.n_pieces = 2 * sw.readers;
	return w;
}

struct Staged { const uint8_t *p = nullptr; size_t used = 0; bool final = false; std::string error; };

// One file through the device.  Lives for the file; the members are destroyed in reverse order: the window reader is waited for first, the
// annotation goes, the decoder's lent stream is given back and the decoder cached or destroyed, the file unmapped last.
class DeviceFileReader {
	FileIngest &file;
	const BamSwitches &sw;
	CellsDataContainer &container;
	const RecordParser &parser;
	const CellsDataContainer::IngestTarget target;
	const clk::time_point t_enter;
	clk::time_point t_file;
	struct Map {
		const BamSwitches &sw;
		const uint8_t *p = nullptr; size_t n = 0; int fd = -1;
		~Map() {
			const auto t = clk::now();
			if (p) munmap(const_cast<uint8_t *>(p), n);
			if (fd >= 0) close(fd);
			sw.trace("[bam] device path: file unmapped %.1f ms\n", since(t));
		}
	} map;
	struct Keep {    // back into the cache when the file went through, destroyed when it did not (whatever state an exception left)
		const BamSwitches &sw;
		dropest_bam_decoder *d = nullptr; int device = 0; bool ok = false;
		~Keep() {
			if (!d) return;
			const auto t_k = clk::now();
			(void)dropest_bam_decoder_use_stream(d, nullptr);      // (the container's stream is the container's)
			sw.trace("[bam] device path: the lent stream given back (and waited for) %.1f ms\n", since(t_k));
			if (!ok) { dropest_bam_decoder_destroy(d); return; }
			std::lock_guard<std::mutex> lk(decoder_cache_mutex());
			auto &slot = decoder_cache()[device];
			if (slot) dropest_bam_decoder_destroy(slot);
			slot = d;
		}
	} keep_dec;
	dropest_bam_decoder *dec = nullptr;
	// -g: the annotation's flat tables on the device (annotation_api.hip); the decoder asks it about the two ends of every alignment
	struct FreeAnn { dropest_annotation *a = nullptr; ~FreeAnn() { if (a) dropest_annotation_destroy(a); } } ann;
	Tools::GeneAnnotation::RefGenesContainer::Flat flat;
	std::vector<uint64_t> ann_gene_hash;
	std::vector<int32_t> id_of_ann_gene;
	size_t c0 = 0; uint32_t u0 = 0;      // where the records begin: the block's file offset, the bytes of the header inside it
	WindowPlan plan;
	std::vector<uint32_t> idx_all, offsets, p_pos, p_gene, p_aux; std::vector<uint64_t> need_off, p_cb, p_umi; std::vector<uint8_t> need_bytes;
	std::vector<uint64_t> dict_hash; std::vector<uint32_t> dict_id; std::vector<int32_t> dict_chr;
	std::vector<uint32_t> name_off; std::vector<uint8_t> name_pool;
	std::vector<int32_t> gene_of_ref;      // -P: every reference's name in the gene dictionary (-1: not yet, -2: the name is empty)
	std::vector<uint32_t> served;          // -r: the table row each asked record was served
	double dev_ms[4] = {0, 0, 0, 0}, host_ms[3] = {0, 0, 0};
	double ms_header = 0, ms_create = 0, ms_setup = 0, ms_wait_read = 0, ms_window_calls = 0;
	size_t window_bytes = 0, n_windows = 0, repaired = 0, refused = 0, n_needs = 0, est_reads = 0;
	bool first = true, dict_dirty = true;
	int which = 0;
	// the window reader's (a helper thread at a time): where the next window begins, the staging memory, the block tables
	size_t file_at = 0;
	uint8_t *stage_p[2] = {nullptr, nullptr};
	uint8_t *piece_p[16] = {};
	bgzf::Blocks blocks_of[2];
	std::atomic<size_t> stretched_windows{0};
	std::future<Staged> next;
	struct Drain { std::future<Staged> &f; ~Drain() { if (f.valid()) f.wait(); } };   // (an exception must not leave the reader running on freed buffers)
	// -b (bam_ingest.h: parse_bam_files(files, true, container)): the decoder writes every window's accepted records again with their tags edited
	// (dropest_bam_decoder_tag_window), a compressor stream on the decoder's stream collects them and hands BGZF blocks to the file in order.
	// Declared behind the decoder: it goes first, while the stream it was lent is still the decoder's.
	struct TaggedOut {
		std::FILE *f = nullptr;
		dropest_deflate_stream *z = nullptr;
		~TaggedOut() { if (z) dropest_deflate_stream_destroy(z); if (f) std::fclose(f); }
		static int write(const uint8_t *bytes, uint64_t len, void *user) { return std::fwrite(bytes, 1, size_t(len), static_cast<TaggedOut *>(user)->f) == size_t(len) ? 0 : 1; }
	} tagged;
	std::vector<uint8_t> header_bytes;      // magic, text, references: the tagged file begins with them, byte for byte
	void tagging_to_decoder();
	void open_tagged();
	void open_filtered();
	void filter_window(const dropest_bam_window &w);
	void close_filtered();
	void tag_window(const dropest_bam_window &w);
	void patch_host_decided(const dropest_bam_window &w);
	std::unordered_map<std::string, uint32_t> ann_gene_index;      // -g: the annotation's gene names -> its gene indices
	void close_tagged();

	[[noreturn]] void fail() const { throw std::runtime_error(std::string(dropest_bgzf_last_error()) + ": " + file.bam_name); }

	bool open_file();
	void read_header();
	bool lease_decoder();
	bool annotation_to_device();
	void staging();
	Staged read_window(int which, size_t want);
	Staged read_window_in_pieces(int which, size_t want, size_t ask);
	Staged read_whole_window(int which, size_t want, size_t ask);
	void read_next() { const int k = which; const size_t want = window_bytes; next = std::async(std::launch::async, [this, k, want] { return read_window(k, want); }); }
	// the ramp goes on and the buffers change places; the window after `stg` is read meanwhile
	void next_window_after(bool last) { window_bytes = std::min(window_bytes * sw.ramp_factor, plan.window_max); which ^= 1; if (!last) read_next(); }
	Staged wait_for_window(std::future<Staged> &f) {
		const auto t_wait = clk::now();
		Staged stg = f.get();
		ms_wait_read += since(t_wait);
		if (!stg.error.empty()) throw std::runtime_error(stg.error + ": " + file.bam_name);
		return stg;
	}
	void dictionaries_to_device();
	void sources_to_decoder();
	void gene_of_reference_to_device();
	bool serve_row(uint32_t row, Parsed &pr) const;
	void take_window(const dropest_bam_window &w, size_t used, clk::time_point t_call);
	void records_through_host(const dropest_bam_window &w, size_t n);
	void resolve_new(const dropest_bam_window &w);
	void windows_one_by_one();
	void windows_pipelined();
public:
	DeviceFileReader(FileIngest &file, CellsDataContainer::IngestTarget target, clk::time_point t_enter)
		: file(file), sw(file.sw), container(file.container), parser(file.parser), target(target), t_enter(t_enter), map{file.sw}, keep_dec{file.sw} {}
	bool read();
};

// (a) the file mapped; false: the host reader says what is wrong with it
bool DeviceFileReader::open_file() {
	map.fd = open(file.bam_name.c_str(), O_RDONLY);
	if (map.fd < 0) return false;
	struct stat sb;
	if (fstat(map.fd, &sb) || sb.st_size <= 0) return false;
	map.n = size_t(sb.st_size);
	void *mp = mmap(nullptr, map.n, PROT_READ, MAP_PRIVATE, map.fd, 0);
	if (mp == MAP_FAILED) return false;
	map.p = static_cast<const uint8_t *>(mp);
	// (the mapping is read at every block's header only, a cache line per ~20 KB: without this every fault maps its 16 neighbours too, and
	// half a million page-table entries of a 683 MB file took 38 ms to unmap)
	(void)madvise(mp, map.n, MADV_RANDOM);
	return true;
}

// (a) where the records begin: magic, l_text, text, n_ref, (l_name, name, l_ref) x n_ref -- blocks inflated here until that much is seen
void DeviceFileReader::read_header() {
	const std::string &bam_name = file.bam_name;
	std::vector<std::string> &refs = file.refs;
	size_t at = 0;
	std::vector<uint8_t> hdr;
	std::vector<std::pair<size_t, size_t>> starts;   // (file offset of the block, inflated bytes before it)
	auto have = [&](size_t nbytes) {
		while (hdr.size() < nbytes) {
			RawBlock b;
			const size_t before = at;
			if (!read_block(map.p, map.n, at, b, bam_name)) throw std::runtime_error("Truncated BAM header: " + bam_name);
			starts.emplace_back(before, hdr.size());
			hdr.resize(hdr.size() + b.isize);
			inflate_block(b, hdr.data() + hdr.size() - b.isize);
		}
	};
	have(12);
	if (std::memcmp(hdr.data(), "BAM\1", 4) != 0) throw std::runtime_error("Can't open BAM file: " + bam_name);
	size_t h = 8 + size_t(le32(hdr.data() + 4));
	have(h + 4);
	const uint32_t n_ref = le32(hdr.data() + h);
	h += 4;
	refs.clear();
	for (uint32_t r = 0; r < n_ref; ++r) {
		have(h + 4);
		const size_t ln = le32(hdr.data() + h);
		have(h + 4 + ln + 4);
		refs.emplace_back(reinterpret_cast<const char *>(hdr.data() + h + 4), ln ? ln - 1 : 0);
		h += 4 + ln + 4;
	}
	if (!file.filtered) container.set_reference_names(refs);      // (-F changes nothing in the container)
	if (file.tagged || (file.filtered && !file.filtered->f)) header_bytes.assign(hdr.begin(), hdr.begin() + h);
	c0 = at; u0 = 0;                                // the header ends with a block: the records open the next one
	for (size_t k = starts.size(); k-- > 0;)
		if (starts[k].second <= h && h < (k + 1 < starts.size() ? starts[k + 1].second : hdr.size())) { c0 = starts[k].first; u0 = uint32_t(h - starts[k].second); break; }
}

// (b) One decoder per device is kept between the files of one parse_bam_files call (streams, device buffers of ~15 x the staging size --
// 2 to 7 GB for windows of 128 to 256 MB -- and 2 x 32 to 2 x 256 MB of pinned staging: ~30 ms to set up, ~40 ms to give back); after the
// last file they are given back on a helper thread (release_decoders_in_background) unless DROPEST_BAM_KEEP_DECODERS=1 keeps them
// for the next call of a long-lived process.
bool DeviceFileReader::lease_decoder() {
	const BamTags &tags = parser.tags;
	dropest_bam_parse_cfg cfg{};
	for (int k = 0; k < 6; ++k) cfg.tag[k] = parser.wanted_tags[k];
	cfg.filled_bam = parser.filled_bam ? 1 : 0; cfg.min_phred = parser.min_barcode_phred; cfg.has_read_type = tags.read_type.empty() ? 0 : 1;
	cfg.n_refs = int32_t(file.refs.size());
	cfg.intronic_len = uint32_t(tags.intronic_read_value.size()); cfg.intergenic_len = uint32_t(tags.intergenic_read_value.size());
	std::memcpy(cfg.intronic, tags.intronic_read_value.data(), cfg.intronic_len);
	std::memcpy(cfg.intergenic, tags.intergenic_read_value.data(), cfg.intergenic_len);
	dropest_bam_decoder *d = nullptr;
	{
		std::lock_guard<std::mutex> lk(decoder_cache_mutex());
		auto it = decoder_cache().find(target.device);
		if (it != decoder_cache().end()) { d = it->second; decoder_cache().erase(it); }
	}
	if (d && dropest_bam_decoder_reset(d, &cfg)) { dropest_bam_decoder_destroy(d); d = nullptr; }
	if (!d && dropest_bam_decoder_create(target.device, &cfg, &d)) return false;       // (no GPU for this: the host reader does it)
	// its kernels on the container's stream (a sharded one: that shard's) for this file: that one exists and has run kernels; one of the decoder's own is ~16 ms to make
	if (target.stream && dropest_bam_decoder_use_stream(d, target.stream)) { dropest_bam_decoder_destroy(d); return false; }
	dec = keep_dec.d = d; keep_dec.device = target.device;
	return true;
}

// (c) -g: the annotation's tables; false: positions beyond 32 bits, or no room for them (the host reader does it)
bool DeviceFileReader::annotation_to_device() {
	const std::vector<std::string> &refs = file.refs;
	if (parser.genes.is_empty() || parser.gene_in_chromosome_name) return true;      // (-P comes before -g: the annotation is not asked)
	try { flat = parser.genes.flatten(); } catch (const std::exception &) { return false; }   // (positions beyond 32 bits: the host reader does it)
	dropest_flat_annotation fa{};
	fa.n_chr = uint32_t(flat.chr_names.size()); fa.n_seg = uint32_t(flat.seg_start.size()); fa.n_tr = uint32_t(flat.tr_gene.size()); fa.n_genes = uint32_t(flat.gene_names.size());
	fa.use_introns_from_gtf = flat.use_introns_from_gtf ? 1 : 0;
	fa.chr_seg_begin = flat.chr_seg_begin.data(); fa.seg_start = flat.seg_start.data(); fa.seg_end = flat.seg_end.data(); fa.seg_tr_begin = flat.seg_tr_begin.data();
	fa.seg_tr = flat.seg_tr.data(); fa.tr_gene = flat.tr_gene.data(); fa.tr_exon_begin = flat.tr_exon_begin.data(); fa.tr_intron_begin = flat.tr_intron_begin.data();
	fa.exon_start = flat.exon_start.data(); fa.exon_end = flat.exon_end.data(); fa.intron_start = flat.intron_start.data(); fa.intron_end = flat.intron_end.data();
	if (dropest_annotation_create(target.device, &fa, &ann.a)) return false;
	std::unordered_map<std::string, int32_t> chr_index;
	for (size_t k = 0; k < flat.chr_names.size(); ++k) chr_index.emplace(flat.chr_names[k], int32_t(k));
	std::vector<int32_t> ann_chr_of_ref(refs.size(), -1);
	for (size_t r = 0; r < refs.size(); ++r) { auto it = chr_index.find(refs[r]); if (it != chr_index.end()) ann_chr_of_ref[r] = it->second; }
	if (dropest_bam_decoder_set_annotation(dec, ann.a, ann_chr_of_ref.data(), uint32_t(refs.size()))) fail();
	ann_gene_hash.resize(flat.gene_names.size());
	for (size_t g = 0; g < flat.gene_names.size(); ++g) ann_gene_hash[g] = CellsDataContainer::hash_name(flat.gene_names[g]);
	id_of_ann_gene.assign(flat.gene_names.size(), -1);
	return true;
}

// (c) -b and -F: the output tag names and read-type values (BamTags.cpp:7-24; an out-value is the configured in-value, else EXONIC / INTRONIC /
// INTERGENIC), under -g the annotation's gene names
void DeviceFileReader::tagging_to_decoder() {
	const BamTags &t = parser.tags;
	dropest_bam_tag_cfg tc{};
	const std::string *names[5] = {&t.gene, &t.cell_barcode_raw, &t.umi_raw, &t.cell_barcode_quality, &t.umi_quality};
	for (int k = 0; k < 5; ++k) tc.out_tag[k] = RecordParser::tag16(*names[k]);
	tc.type_tag = RecordParser::tag16(t.read_type);
	const std::string values[3] = {t.exonic_read_value.empty() ? "EXONIC" : t.exonic_read_value, t.intronic_read_value.empty() ? "INTRONIC" : t.intronic_read_value,
	                               t.intergenic_read_value.empty() ? "INTERGENIC" : t.intergenic_read_value};
	for (int k = 0; k < 3; ++k) { tc.type_len[k] = uint32_t(values[k].size()); std::memcpy(tc.type_val[k], values[k].data(), std::min<size_t>(values[k].size(), 24)); }
	std::vector<uint32_t> off; std::vector<uint8_t> pool;
	if (ann.a) {
		off.push_back(0);
		for (const std::string &g : flat.gene_names) { pool.insert(pool.end(), g.begin(), g.end()); off.push_back(uint32_t(pool.size())); ann_gene_index.emplace(g, uint32_t(ann_gene_index.size())); }
		pool.push_back(0);
		tc.gene_name_off = off.data(); tc.gene_name_pool = pool.data(); tc.n_gene_names = uint32_t(flat.gene_names.size());
	}
	if (dropest_bam_decoder_set_tagging(dec, &tc)) fail();
	if (parser.gene_in_chromosome_name) {      // -P: the gene the kernels write is the reference's name
		std::vector<uint32_t> r_off(1, 0); std::vector<uint8_t> r_pool;
		for (const std::string &r : file.refs) { r_pool.insert(r_pool.end(), r.begin(), r.end()); r_off.push_back(uint32_t(r_pool.size())); }
		r_pool.push_back(0);
		if (r_pool.size() > 0xFFFFFFF0ull || dropest_bam_decoder_set_reference_names(dec, r_off.data(), r_pool.data(), uint32_t(file.refs.size()))) fail();
	}
}

// (c) -b: `<input stem>.tagged.bam` in the current directory (BamProcessor::get_result_bam_name, BamProcessorAbstract::update_bam strips the
// directory); the header's bytes go in first
void DeviceFileReader::open_tagged() {
	tagging_to_decoder();
	std::string name = file.bam_name.substr(0, file.bam_name.find_last_of('.')) + ".tagged.bam";
	const size_t slash = name.find_last_of("\\/");
	if (slash != std::string::npos) name = name.substr(slash + 1);
	file.tagged->name = name;
	tagged.f = std::fopen(name.c_str(), "wb");
	if (!tagged.f) throw std::runtime_error("Can't write tagged BAM file: " + name);
	if (dropest_deflate_stream_create(target.device, dropest_bam_decoder_stream(dec), sw.tagged_batch, TaggedOut::write, &tagged, &tagged.z) ||
	    dropest_deflate_stream_put(tagged.z, header_bytes.data(), header_bytes.size(), 0))
		throw std::runtime_error(std::string(dropest_deflate_last_error()) + ": " + name);
}

// (c) -F: the six tags of -b, then the two corrected ones, their values' tables (every cell's barcode code: the context's device array; the
// container's side strings) to this file's decoder.  The FIRST file of the call opens the one output, `<its stem>.filtered.bam` in the current
// directory, with its header's bytes (FilteringBamProcessor::update_bam, :103-110: _is_bam_open); the compressor runs on the container's stream,
// which every file's decoder is lent.
void DeviceFileReader::open_filtered() {
	FilteredPass &P = *file.filtered;
	tagging_to_decoder();
	dropest_bam_filter_cfg fc{};
	fc.out_tag[0] = RecordParser::tag16(parser.tags.cell_barcode); fc.out_tag[1] = RecordParser::tag16(parser.tags.umi);
	fc.on_device = 1; fc.cell_barcode = P.d_cell_codes; fc.n_cells = uint32_t(P.n_cells);
	if (!P.pieces.empty()) {      // sharded: the columns' barcodes, the copy on this decoder's GPU
		uint64_t n_columns = 0;
		if (dropest_shard_filtered_barcodes_device(P.pieces[P.cur].shard, &n_columns, &fc.cell_barcode) != DROPEST_OK) throw std::runtime_error(std::string("Filtered BAM output (-F): ") + dropest_last_error());
		if (n_columns != P.n_cells) throw std::runtime_error("Filtered BAM output (-F): internal: the shards name different numbers of columns");
	}
	fc.n_side = uint32_t(P.side_off.size() - 1); fc.side_off = P.side_off.data(); fc.side_pool = P.side_pool.data();
	if (dropest_bam_decoder_set_filtering(dec, &fc)) fail();
	// The compressor runs where the decoder does.  One context lends every file's decoder the same stream, and one compressor serves the call;
	// a file of a sharded run whose first read lives with another shard brings another stream (another GPU, even): the compressor's leftover
	// then goes out as a short block and a new one follows the decoder, so that the bytes need no ordering between two streams.
	void *const st = dropest_bam_decoder_stream(dec);
	if (P.z && (P.z_device != target.device || P.z_stream != st)) P.retire_compressor(0);
	const bool first_file = !P.f;
	if (first_file) {
		std::string name = file.bam_name.substr(0, file.bam_name.find_last_of('.')) + ".filtered.bam";
		const size_t slash = name.find_last_of("\\/");
		if (slash != std::string::npos) name = name.substr(slash + 1);
		P.name = name;
		P.f = std::fopen(name.c_str(), "wb");
		if (!P.f) throw std::runtime_error("Can't write filtered BAM file: " + name);
	}
	if (!P.z) {
		if (dropest_deflate_stream_create(target.device, st, sw.tagged_batch, FilteredPass::write, &P, &P.z)) throw std::runtime_error(std::string(dropest_deflate_last_error()) + ": " + P.name);
		P.z_device = target.device; P.z_stream = st;
	}
	if (first_file && dropest_deflate_stream_put(P.z, header_bytes.data(), header_bytes.size(), 0)) throw std::runtime_error(std::string(dropest_deflate_last_error()) + ": " + P.name);
}

// (g) -F: the window the decoder holds under the decisions of its accepted records -- entries [at, at + n_accepted) of the container's, where they are
void DeviceFileReader::filter_window(const dropest_bam_window &w) {
	FilteredPass &P = *file.filtered;
	const uint64_t n = w.n_accepted;
	if (n > P.n_reads - P.at) P.other_files("a window of " + file.bam_name + " brings the accepted reads to " + std::to_string(P.at + n) + ", the container holds " + std::to_string(P.n_reads));
	const uint8_t *d_out = nullptr;
	uint64_t len = 0, written = 0;
	// sharded: [at, at + n) cut at the boundaries of the shards' ranges -- every shard whose range meets or touches the window gives one segment
	// (an empty one where it only touches, or holds no reads)
	std::vector<dropest_bam_decision_segment> segs;
	for (const FilteredPass::Piece &q : P.pieces) {
		const uint64_t lo = std::max(P.at, q.first), hi = std::min(P.at + n, q.first + q.n);
		if (lo > hi) continue;
		const uint64_t skip = lo - q.first;
		segs.push_back(dropest_bam_decision_segment{hi - lo, q.verdict + skip, q.column + skip, q.umi + skip, int32_t(q.device)});
	}
	auto filter = [&] {
		return P.pieces.empty() ? dropest_bam_decoder_filter_window(dec, P.d_verdict + P.at, P.d_cell + P.at, P.d_umi + P.at, n, 1, &d_out, &len, &written)
		                        : dropest_bam_decoder_filter_window_segments(dec, segs.data(), uint32_t(segs.size()), &d_out, &len, &written);
	};
	int rc = filter();
	if (rc == 2) { patch_host_decided(w); rc = filter(); }
	if (rc) fail();
	if (len && dropest_deflate_stream_put(P.z, d_out, len, 1)) throw std::runtime_error(std::string(dropest_deflate_last_error()) + ": " + P.name);
	P.at += n; P.written += written; ++P.windows;
	P.decode_ms += w.ms_copy + w.ms_inflate + w.ms_boundaries + w.ms_parse;
}

// (h) -F: this file's share of the tag kernels' time; the decoder may be kept for a call that writes nothing
void DeviceFileReader::close_filtered() {
	double ms = 0;
	(void)dropest_bam_decoder_tag_stats(dec, &ms, nullptr, nullptr);
	file.filtered->tag_ms += ms;
	(void)dropest_bam_decoder_set_tagging(dec, nullptr);
}

// (g) -b: the window the decoder holds, tagged, to the compressor (on the decoder's stream: the bytes are copied before the next window overwrites them)
void DeviceFileReader::tag_window(const dropest_bam_window &w) {
	const uint8_t *d_out = nullptr;
	uint64_t len = 0, written = 0;
	int rc = dropest_bam_decoder_tag_window(dec, &d_out, &len, &written);
	if (rc == 2) { patch_host_decided(w); rc = dropest_bam_decoder_tag_window(dec, &d_out, &len, &written); }
	if (rc) fail();
	if (len && dropest_deflate_stream_put(tagged.z, d_out, len, 1)) throw std::runtime_error(std::string(dropest_deflate_last_error()) + ": " + file.tagged->name);
	++file.tagged->windows; file.tagged->records += size_t(written);
}

// (g) -b with -g: reads at loci with more transcripts at an end point than the annotation kernel holds come back among the window's need records with
// no verdict; the host's annotation decides them (as resolve_new does for the container), and the tag kernels are given its gene and mark
void DeviceFileReader::patch_host_decided(const dropest_bam_window &w) {
	const size_t m = w.n_need;
	size_t bytes = 0;
	for (size_t k = 0; k < m; ++k) bytes += w.need_size[k];
	need_bytes.resize(bytes + 16); need_off.resize(m);
	if (dropest_bam_decoder_fetch_records(dec, w.need_rec, uint32_t(m), need_bytes.data(), need_bytes.size(), need_off.data())) fail();
	std::vector<uint32_t> rec, gene, mark;
	Parsed tmp;
	for (size_t k = 0; k < m; ++k) {
		parser.parse(need_bytes.data() + need_off[k], tmp);
		if (tmp.status != Parsed::OK) throw std::runtime_error("internal: the device and the host read a BAM record differently: " + file.bam_name);
		const auto it = tmp.r.gene.empty() ? ann_gene_index.end() : ann_gene_index.find(std::string(tmp.r.gene));
		rec.push_back(w.need_rec[k]); gene.push_back(it == ann_gene_index.end() ? 0xFFFFFFFFu : it->second); mark.push_back(tmp.r.mark);
	}
	if (dropest_bam_decoder_patch_annotation(dec, rec.data(), gene.data(), mark.data(), uint32_t(m))) fail();
}

// (h) -b: what is left over, the end-of-file block, and the account of what was written
void DeviceFileReader::close_tagged() {
	BamController::TaggedFile &t = *file.tagged;
	if (dropest_deflate_stream_finish(tagged.z, DROPEST_DEFLATE_EOF)) throw std::runtime_error(std::string(dropest_deflate_last_error()) + ": " + t.name);
	uint64_t in = 0, out = 0, batches = 0, tag_in = 0, tag_out = 0;
	(void)dropest_deflate_stream_stats(tagged.z, &t.deflate_ms, &in, &out, &batches);
	(void)dropest_bam_decoder_tag_stats(dec, &t.tag_ms, &tag_in, &tag_out);
	t.inflated_bytes = size_t(in); t.compressed_bytes = size_t(out); t.batches = size_t(batches); t.tag_bytes_in = size_t(tag_in); t.tag_bytes_out = size_t(tag_out);
	dropest_deflate_stream_destroy(tagged.z); tagged.z = nullptr;
	const bool ok = std::fclose(tagged.f) == 0;
	tagged.f = nullptr;
	if (!ok) throw std::runtime_error("Can't write tagged BAM file: " + t.name);
	(void)dropest_bam_decoder_set_tagging(dec, nullptr);      // (the decoder may be kept for a call that writes none)
}

// The compressed bytes reach the device in pieces: helper threads (up to eight for a long window) read the next window from the file into
// pinned pieces of 2 MB (pread: page cache -> pinned memory) and sends each on its way (dropest_bam_decoder_upload_piece) while the device
// and this thread work on the window before.  The window itself is the mapped file's bytes: the block table is made from them, the host
// fall-back for a refused block reads them.  (Rounds 4-6a read whole windows into two pinned buffers of the window's size: 2 x 128 MB were
// 35-65 ms to allocate, a fifth to a third of a 16 M read file's time -- DROPEST_BAM_WHOLE_WINDOW_STAGING=1 takes that road.)
void DeviceFileReader::staging() {
	const size_t stage_cap = plan.stage_cap;
	if (sw.in_pieces) {
		for (int k = 0; k < 2; ++k)      // (first: the upload stream is made beside the pinned allocation, and a device allocation would wait for it)
			if (dropest_bam_decoder_reserve(dec, k, stage_cap, plan.compressed_seen ? uint64_t(double(stage_cap) * double(plan.inflated_seen) / double(plan.compressed_seen) * 1.25) : 0)) fail();
		sw.trace("[bam] device path: the device buffers of two windows of %zu MB %.1f ms\n", stage_cap >> 20, since(t_file));
		if (dropest_bam_decoder_pieces(dec, plan.n_pieces, sw.piece_bytes, piece_p)) fail();
		sw.trace("[bam] device path: ... and %u pinned pieces of %zu MB %.1f ms\n", plan.n_pieces, sw.piece_bytes >> 20, since(t_file));
	} else
		for (int k = 0; k < 2; ++k)      // (pinning 2 x 80 MB and reserving a window's device buffers: 35-50 ms; side by side on two threads they take as long)
			if (dropest_bam_decoder_staging(dec, k, stage_cap, &stage_p[k])) fail();
}

// (e) the next window of the file into staging buffer `which`: up to `want` bytes of whole blocks.  Runs on a helper thread, one at a time.
Staged DeviceFileReader::read_window(int which, size_t want) {
	const size_t ask = std::min(std::min(want + (size_t(1) << 16) + 64, plan.stage_cap), map.n - file_at);
	return sw.in_pieces ? read_window_in_pieces(which, want, ask) : read_whole_window(which, want, ask);
}

// the window's bytes to the device piece by piece (helper threads: everything up to `want` needs no block boundary), its extent and
// block table from the file meanwhile (this thread), the last blocks' bytes beyond `want` at the end
Staged DeviceFileReader::read_window_in_pieces(int which, size_t want, size_t ask) {
	Staged st;
	st.p = map.p + file_at;
	bgzf::Blocks &B = blocks_of[which];
	const size_t PIECE = sw.piece_bytes, at = file_at;
	const int fd = map.fd;
	const auto t_rw = clk::now();
	struct SayRw { const BamSwitches &sw; clk::time_point t; size_t &used; ~SayRw() { sw.trace_reader("[bam] reader: a window of %.1f MB read and sent in %.2f ms\n", double(used) / 1048576.0, since(t)); } } say_rw{sw, t_rw, st.used};
	std::atomic<bool> failed{dropest_bam_decoder_upload_begin(dec, which) != 0};
	const size_t covered = std::min(want, ask);
	const size_t n_pieces = (covered + PIECE - 1) / PIECE;
	const uint32_t n_readers = uint32_t(std::min<size_t>(sw.readers, n_pieces));
	const bool trace_rw = sw.trace_reader_on && file_at == c0;
	auto lap_rw = [trace_rw, t_rw](const char *what) { if (trace_rw) std::fprintf(stderr, "[bam] reader, first window: %s at %.2f ms\n", what, since(t_rw)); };
	lap_rw("upload_begin done");
	dropest_bam_decoder *const d = dec;
	uint8_t *const *const pieces = piece_p;
	auto send = [d, pieces, fd, at, which, &failed, lap_rw](uint32_t slot, size_t from, size_t len) {
		if (dropest_bam_decoder_piece_wait(d, slot)) { failed = true; return; }
		lap_rw("piece_wait done");
		size_t g = 0;
		while (g < len) {
			const ssize_t got = pread(fd, pieces[slot] + g, len - g, off_t(at + from + g));
			if (got <= 0) { failed = true; return; }
			g += size_t(got);
		}
		lap_rw("pread done");
		if (dropest_bam_decoder_upload_piece(d, which, slot, from, len)) failed = true;
		lap_rw("upload_piece done");
	};
	auto reader = [&send, &failed, n_pieces, n_readers, PIECE, covered](uint32_t r) {
		for (size_t k = r, turn = 0; k < n_pieces && !failed.load(std::memory_order_relaxed); k += n_readers, ++turn)
			send(2u * r + uint32_t(turn & 1u), k * PIECE, std::min(PIECE, covered - k * PIECE));
	};
	std::vector<std::future<void>> helpers;
	for (uint32_t r = 0; r < n_readers; ++r) helpers.push_back(std::async(std::launch::async, reader, r));
	bgzf::FileWalk walk;
	walk.fd = fd; walk.file_at = at; walk.block_cap = plan.block_cap; walk.avg_block = plan.avg_block;
	walk.least_bytes = sw.stretch_bytes; walk.least_blocks = sw.stretch_blocks; walk.one_walker = sw.one_walker;
	bool stretched = false;
	const size_t o = walk.whole_blocks_of_file(ask, want, B, st.error, &stretched);
	if (stretched) ++stretched_windows;
	lap_rw("block walk done");
	for (auto &f : helpers) f.get();
	lap_rw("helpers joined");
	if (!st.error.empty()) return st;
	for (size_t from = covered; from < o && !failed.load(); from += PIECE) send(0, from, std::min(PIECE, o - from));      // (at most 64 KB)
	st.used = o; file_at += o; st.final = file_at >= map.n;
	// (a piece that could not be read or sent: nothing is declared, and the window call copies the mapped bytes itself)
	const dropest_bgzf_blocks table{uint64_t(B.in_off.size()), B.in_off.data(), B.in_len.data(), B.out_len.data(), B.crc.data()};
	if (!failed.load()) (void)dropest_bam_decoder_upload_done(dec, which, st.p, o, &table);
	lap_rw("upload_done done");
	return st;
}

// the window read whole into pinned buffer `which` (DROPEST_BAM_WHOLE_WINDOW_STAGING, DROPEST_BAM_NO_UPLOAD_AHEAD)
Staged DeviceFileReader::read_whole_window(int which, size_t want, size_t ask) {
	Staged st;
	uint8_t *const buf = stage_p[which];
	st.p = buf;
	const int fd = map.fd;
	const size_t at = file_at;
	// (the copy out of the page cache runs at ~4-5 GB/s per thread: a long window is read in four pieces side by side, so that the reader
	// stays ahead of the device -- which takes ~11 ms per 64 MB window)
	auto read_piece = [buf, fd, at](size_t from, size_t len) -> long {
		size_t g = 0;
		while (g < len) {
			const ssize_t r = pread(fd, buf + from + g, len - g, off_t(at + from + g));
			if (r < 0) return -1;
			if (r == 0) break;
			g += size_t(r);
		}
		return long(g);
	};
	size_t got = 0;
	const size_t n_pieces = ask > (size_t(8) << 20) ? 4 : 1, piece = (ask / n_pieces + 4095) & ~size_t(4095);
	std::vector<std::future<long>> rest;
	for (size_t k = 1; k < n_pieces; ++k) if (k * piece < ask) rest.push_back(std::async(std::launch::async, read_piece, k * piece, std::min(piece, ask - k * piece)));
	const long g0 = read_piece(0, std::min(piece, ask));
	bool whole = g0 == long(std::min(piece, ask)), failed = g0 < 0;
	if (g0 > 0) got = size_t(g0);
	for (size_t k = 0; k < rest.size(); ++k) {
		const long g = rest[k].get();
		if (g < 0) failed = true;
		else if (whole) { got += size_t(g); whole = size_t(g) == std::min(piece, ask - (k + 1) * piece); }
	}
	if (failed) { st.error = "Can't read BAM file"; return st; }
	const size_t o = bgzf::whole_blocks(buf, got, want, plan.block_cap, st.error);
	if (!st.error.empty()) return st;
	st.used = o; file_at += o; st.final = file_at >= map.n;
	if (sw.upload_ahead) (void)dropest_bam_decoder_upload(dec, which, o);   // on its way while the window before it is in the kernels (if this fails, the window call copies)
	return st;
}

// (f) the dictionaries as they stand (other files, earlier windows, add_record calls) go to the device
void DeviceFileReader::dictionaries_to_device() {
	const auto t_phase = clk::now();
	if (dict_dirty) {
		container.dictionary_snapshot(dict_hash, dict_id, dict_chr);
		if (file.filtered) dict_chr.assign(file.refs.size(), 0);      // (-F looks at no chromosome: every reference counts as met, so that none makes a need record)
		if (dropest_bam_decoder_set_dictionaries(dec, dict_hash.data(), dict_id.data(), uint32_t(dict_hash.size()), dict_chr.data(), uint32_t(dict_chr.size()))) fail();
		{   // ... and the genes' names: a hash the device finds is confirmed byte by byte (two names with one FNV-1a value must not share an index)
			const auto &names = container.gene_indexer().values();
			name_off.resize(names.size() + 1);
			size_t bytes = 0;
			for (size_t g = 0; g < names.size(); ++g) { name_off[g] = uint32_t(bytes); bytes += names[g].size(); }
			name_off[names.size()] = uint32_t(bytes);
			name_pool.resize(bytes + 1);
			for (size_t g = 0; g < names.size(); ++g) std::memcpy(name_pool.data() + name_off[g], names[g].data(), names[g].size());
			if (bytes > 0xFFFFFFF0ull || dropest_bam_decoder_set_gene_names(dec, name_off.data(), name_pool.data(), uint32_t(names.size()))) fail();
		}
		if (ann.a) {   // the annotation's genes that the dictionary holds by now
			for (size_t g = 0; g < flat.gene_names.size(); ++g)
				if (id_of_ann_gene[g] < 0) id_of_ann_gene[g] = int32_t(container.lookup_gene(ann_gene_hash[g], flat.gene_names[g]));
			if (dropest_bam_decoder_set_annotation_genes(dec, id_of_ann_gene.data(), uint32_t(id_of_ann_gene.size()))) fail();
		}
		if (parser.gene_in_chromosome_name) gene_of_reference_to_device();
		dict_dirty = false;
	}
	host_ms[0] += since(t_phase);
}

// (c) -r: the controller's table, with the stream ordinal the file's first record claims with
void DeviceFileReader::sources_to_decoder() {
	if (file.params && dropest_bam_decoder_set_read_params(dec, file.params->table, file.params->ordinal)) fail();
}

// (f) -P: the references' names as the gene dictionary holds them by now
void DeviceFileReader::gene_of_reference_to_device() {
	const std::vector<std::string> &refs = file.refs;
	gene_of_ref.resize(refs.size());
	for (size_t r = 0; r < refs.size(); ++r) gene_of_ref[r] = refs[r].empty() ? -2 : int32_t(container.lookup_gene(CellsDataContainer::hash_name(refs[r]), refs[r]));
	if (!refs.empty() && dropest_bam_decoder_set_gene_of_reference(dec, gene_of_ref.data(), uint32_t(refs.size()))) fail();
}

// (g) -r: what BamController::serve_read_params does with the map's entry, with the row the DEVICE served this record (RP: 0xFFFFFFFF = none):
// no second look-up here.  false: the record is not to be looked at any further (it is counted under pr.status)
bool DeviceFileReader::serve_row(uint32_t row, Parsed &pr) const {
	if (pr.status == Parsed::SKIP || pr.status == Parsed::CANT_PARSE_NO_COUNT) return false;
	ParamSource::Row r;
	if (row == 0xFFFFFFFFu || row >= file.params->lines() || !file.params->row(row, r)) { pr.status = Parsed::CANT_PARSE; return false; }
	if (!r.pass) { pr.status = Parsed::LOW_QUALITY; return false; }
	if (pr.status != Parsed::OK) return false;
	pr.r.cb = r.cb; pr.r.umi = r.umi; pr.r.umi_quality = r.umi_quality; pr.r.umi_quality_length = uint32_t(r.umi_quality.size());
	if (!CellsDataContainer::pack_code(pr.r.cb, pr.r.cb_code)) pr.r.cb_code = 0;
	if (!CellsDataContainer::pack_code(pr.r.umi, pr.r.umi_code)) pr.r.umi_code = 0;
	return true;
}

// (g) UMI quality strings the container cannot take in bulk (it keeps them on the host): the records of this window come back as bytes and
// take the host reader's bulk path over them (BulkWindow: one quality row per read while the strings have one length), or, where that
// refuses, go record by record
void DeviceFileReader::records_through_host(const dropest_bam_window &w, size_t n) {
	idx_all.resize(n); need_off.resize(n);
	for (size_t i = 0; i < n; ++i) idx_all[i] = uint32_t(i);
	need_bytes.resize(size_t(w.window_bytes) + 16);
	if (dropest_bam_decoder_fetch_records(dec, idx_all.data(), uint32_t(n), need_bytes.data(), need_bytes.size(), need_off.data())) fail();
	offsets.resize(n);
	for (size_t i = 0; i < n; ++i) offsets[i] = uint32_t(need_off[i]);
	dict_dirty = true;
	// (-r: record by record, as the host reader goes under -r; every record with the row the device served it)
	if (!file.params && w.window_bytes < (uint64_t(1) << 32) && !sw.record_by_record && container.bulk_ingest_possible_at_all() && file.bulk.ingest(need_bytes.data(), offsets, n)) return;
	if (file.params) { served.resize(n); if (dropest_bam_decoder_param_rows(dec, nullptr, uint32_t(n), served.data())) fail(); }
	Parsed tmp;
	for (size_t i = 0; i < n; ++i) {
		parser.parse(need_bytes.data() + need_off[i], tmp);
		if (file.params) serve_row(served[i], tmp);
		if (count_status(file.counters, tmp.status)) container.add_record(tmp.r);
	}
}

// (g) what the dictionaries have not seen, in file order: the records that bring it come back as bytes, their columns are patched on the device
void DeviceFileReader::resolve_new(const dropest_bam_window &w) {
	const size_t m = w.n_need;
	n_needs += m;
	size_t bytes = 0;
	for (size_t k = 0; k < m; ++k) bytes += w.need_size[k];
	need_bytes.resize(bytes + 16); need_off.resize(m);
	p_pos.resize(m); p_cb.resize(m); p_umi.resize(m); p_gene.resize(m); p_aux.resize(m);
	if (dropest_bam_decoder_fetch_records(dec, w.need_rec, uint32_t(m), need_bytes.data(), need_bytes.size(), need_off.data())) fail();
	if (file.params) { served.resize(m); if (dropest_bam_decoder_param_rows(dec, w.need_rec, uint32_t(m), served.data())) fail(); }
	Parsed tmp;
	for (size_t k = 0; k < m; ++k) {
		parser.parse(need_bytes.data() + need_off[k], tmp);
		if (file.params) serve_row(served[k], tmp);      // (-r: barcode, UMI and quality of the row the device served; -P: the parser names the reference itself)
		if (tmp.status != Parsed::OK) throw std::runtime_error("internal: the device and the host read a BAM record differently: " + file.bam_name);
		const CellsDataContainer::ParsedRead &r = tmp.r;
		const bool has_gene = !r.gene.empty();
		const bool touches = !has_gene || (r.mark & (UMI::Mark::HAS_EXONS | UMI::Mark::HAS_INTRONS));
		// (a gene and a chromosome are entered whether the dictionaries know them or not: they then answer with what they hold)
		const uint8_t what = uint8_t((r.cb_code ? 0 : NEED_CB) | (has_gene && !r.umi_code ? NEED_UMI : 0) | (has_gene ? NEED_GENE : 0) | (touches ? NEED_CHR : 0));
		p_pos[k] = w.need_pos[k];
		p_cb[k] = r.cb_code; p_umi[k] = has_gene ? r.umi_code : 1; p_gene[k] = DROPEST_NO_GENE; p_aux[k] = uint32_t(r.mark) << 16;
		intern_new(container, NewParts{what, r.ref_id, r.cb, r.umi, r.gene, r.gene_hash}, p_cb[k], p_umi[k], p_gene[k], p_aux[k]);
	}
	if (dropest_bam_decoder_patch(dec, p_pos.data(), p_cb.data(), p_umi.data(), p_gene.data(), p_aux.data(), uint32_t(m))) fail();
	dict_dirty = true;
}

// (g) one decoded window into the container and the counters
void DeviceFileReader::take_window(const dropest_bam_window &w, size_t used, clk::time_point t_call) {
	ms_window_calls += since(t_call);
	if (file.params) file.params->ordinal += w.n_records;      // (the next file's first record claims above every record of this one)
	if (file.filtered) { first = false; ++n_windows; filter_window(w); return; }      // the second pass: nothing goes into the container
	if (file.tagged) tag_window(w);      // first thing: whichever way the window then goes into the container, its accepted records are written
	if (first) {
		est_reads = size_t(double(w.n_records) * double(map.n - c0) / double(std::max<size_t>(used, 1)) * double(file.n_files) * 1.05);
		const auto t_e = clk::now();
		container.expect_reads(est_reads);
		sw.trace("[bam] device path: the container told to expect %zu reads %.1f ms\n", est_reads, since(t_e));
	}
	first = false;
	++n_windows; repaired += w.guesses_repaired; refused += w.refused_blocks;
	dev_ms[0] += w.ms_copy; dev_ms[1] += w.ms_inflate; dev_ms[2] += w.ms_boundaries; dev_ms[3] += w.ms_parse;
	sw.trace_reader("[bam] window %zu: %.1f MB, %u blocks, %llu records: copy in %.2f, inflate %.2f, chain %.2f, fields %.2f ms; the call %.2f ms\n", n_windows, double(used) / 1048576.0, w.n_blocks, (unsigned long long)w.n_records, w.ms_copy, w.ms_inflate, w.ms_boundaries, w.ms_parse, since(t_call));
	const size_t n = size_t(w.n_records);
	if (!n) return;
	auto t_phase = clk::now();
	// UMI quality strings: one length over the gene-bearing reads of the window (and the container's so far) -> the device hands over one row
	// per accepted read beside the columns; anything else -> the window's records come back as bytes
	const bool has_q = w.any_gene && w.quality_len_max > 0;
	const uint32_t q_len = w.quality_len_max;
	const bool q_bulk = has_q && w.quality_len_min == w.quality_len_max && container.bulk_ingest_possible_with_quality(q_len, true);
	if ((has_q ? !q_bulk : !container.bulk_ingest_possible(true)) || (file.tagged && !container.bulk_ingest_possible_at_all(true))) {
		records_through_host(w, n);
		host_ms[1] += since(t_phase);
		return;
	}
	if (w.n_need) resolve_new(w);
	host_ms[1] += since(t_phase); t_phase = clk::now();
	bool any_gene = w.any_gene != 0;
	for (size_t k = 0; k < size_t(w.n_need) && !any_gene; ++k) any_gene = p_gene[k] != DROPEST_NO_GENE;
	if (q_bulk) {
		container.reserve_quality_rows(est_reads, q_len);
		const uint8_t *rows = nullptr;
		if (dropest_bam_decoder_quality_rows(dec, q_len, &rows)) fail();
		container.add_records_packed_device(w.d_cb, w.d_umi, w.d_gene, w.d_aux, size_t(w.n_accepted), any_gene, rows, q_len, target.device, target.stream);
	} else
		container.add_records_packed_device(w.d_cb, w.d_umi, w.d_gene, w.d_aux, size_t(w.n_accepted), any_gene, target.device, target.stream);
	host_ms[2] += since(t_phase);
	BamController::Counters &c = file.counters;
	c.cant_parse += size_t(w.counts[DROPEST_BAM_CANT_PARSE_NO_COUNT] + w.counts[DROPEST_BAM_CANT_PARSE]);
	c.low_quality += size_t(w.counts[DROPEST_BAM_LOW_QUALITY]);
	c.saved += size_t(w.counts[DROPEST_BAM_OK]);
	c.total_reads += size_t(w.counts[DROPEST_BAM_OK] + w.counts[DROPEST_BAM_CANT_PARSE] + w.counts[DROPEST_BAM_LOW_QUALITY]);
}

// (h) the default order: window k is through the device and the container before window k + 1 (read meanwhile) is given to the device
void DeviceFileReader::windows_one_by_one() {
	for (;;) {
		const Staged stg = wait_for_window(next);
		next_window_after(stg.final);
		Drain drain{next};
		dictionaries_to_device();
		dropest_bam_window w{};
		const auto t_call = clk::now();
		if (dropest_bam_decoder_window(dec, stg.p, stg.used, first ? u0 : 0u, stg.final ? 1 : 0, host_inflate, nullptr, &w)) fail();
		take_window(w, stg.used, t_call);
		if (stg.final) break;
	}
}

// (h) Round 6, DROPEST_BAM_PIPELINE=1 (off by default): the inflate of window k + 1 is given to the device BEFORE this thread waits for window k
// (dropest_bam_decoder_window_inflate / _chain).  A window's inflate lasts as long as its slowest block (7-11 ms on a file that deflates
// 3 x) and one window after the other leaves wave slots empty -- 86 ms of inflate in situ for a kernel that needs 42
// (profiles/r06a_bam_3x_file_device_trace.txt) -- but the next window's blocks then hold every slot while this window's small kernels
// and copies want some: inside the window calls 109-121 -> 81-95 ms, the dictionaries' copies 1 -> 31 ms, two more streams to create
// (8 ms each): ingest 195 -> 233 ms on the same box.  Kept as an order the library supports and the suite runs; not the default.
void DeviceFileReader::windows_pipelined() {
	Staged stg = wait_for_window(next), stg_ahead;
	int slot_cur = 0, slot_ahead = 0;
	next_window_after(stg.final);
	if (dropest_bam_decoder_window_inflate(dec, stg.p, stg.used, &slot_cur)) { if (next.valid()) next.wait(); fail(); }
	for (;;) {
		const bool final = stg.final;
		Drain drain{next};
		if (!final) {      // the window after this one: read by now (its buffer is the other one), its blocks to the device
			stg_ahead = wait_for_window(next);
			const auto t_a = clk::now();
			if (dropest_bam_decoder_window_inflate(dec, stg_ahead.p, stg_ahead.used, &slot_ahead)) fail();
			ms_window_calls += since(t_a);
		}
		dictionaries_to_device();
		dropest_bam_window w{};
		const auto t_call = clk::now();
		if (dropest_bam_decoder_window_chain(dec, slot_cur, first ? u0 : 0u, final ? 1 : 0, host_inflate, nullptr)) fail();
		// this window's compressed bytes are done with: the reader may fill their buffer with the window after the next
		if (!final && !stg_ahead.final) next_window_after(false);
		if (dropest_bam_decoder_window_finish(dec, slot_cur, &w)) fail();
		take_window(w, stg.used, t_call);
		if (final) break;
		stg = std::move(stg_ahead); slot_cur = slot_ahead;
	}
}

bool DeviceFileReader::read() {
	if (!open_file()) { file.refusal = "the file cannot be opened or mapped"; return false; }
	read_header();
	ms_header = since(t_enter);
	if (!lease_decoder()) { file.refusal = std::string("no GPU decoder (") + dropest_bgzf_last_error() + ")"; return false; }
	ms_create = since(t_enter) - ms_header;
	if (!annotation_to_device()) { file.refusal = "the gene annotation cannot be held on the device"; return false; }
	sources_to_decoder();
	if (file.tagged) open_tagged();
	if (file.filtered) open_filtered();
	t_file = clk::now();
	// (1 MB first: the file's genes and chromosomes are mostly met there, and every one of them is a record the host parses -- a first window of
	// 4 / 8 / 16 MB: 65 -> 76 / 79 / 87 ms on the 3.2 x file; then x 8: 1, 8, 64 MB ... measured against x 4 and x 16 with the round's final decoder:
	// 3.2 x file 65-70 -> 59-67 ms, 10.8 x file 85-87 -> 73-75)
	window_bytes = sw.ramp_first << 20;
	plan = plan_windows(sw, map.p, map.n, c0, dropest_bam_decoder_wave_slots(dec));
	staging();
	ms_setup = since(t_file);
	file_at = c0;
	read_next();
	if (sw.pipeline) windows_pipelined(); else windows_one_by_one();
	if (file.tagged) close_tagged();
	if (file.filtered) close_filtered();
	if (file.params) (void)dropest_bam_decoder_set_read_params(dec, nullptr, 0);      // (the decoder may be kept longer than the controller's table lives)
	sw.trace("[bam] device path: %zu windows, %.1f ms behind the header; copy in %.1f ms, inflate %.1f ms (%zu blocks left to the host), record chain %.1f ms (%zu guesses "
	         "repaired), fields + dense columns %.1f ms; host: dictionaries to the device %.1f ms, %zu records with something new %.1f ms, container %.1f ms\n",
	         n_windows, since(t_file), dev_ms[0], dev_ms[1], refused, dev_ms[2], repaired, dev_ms[3], host_ms[0], n_needs, host_ms[1], host_ms[2]);
	sw.trace("[bam] device path: file mapped and header read %.1f ms, decoder created %.1f ms, annotation + the rest before the windows %.1f ms\n", ms_header, ms_create, std::chrono::duration<double, std::milli>(t_file - t_enter).count() - ms_header - ms_create);
	sw.trace("[bam] device path: pinned staging buffers %.1f ms, waiting for the file reader %.1f ms, inside the window calls %.1f ms\n", ms_setup, ms_wait_read, ms_window_calls);
	keep_dec.ok = true;
	sw.trace("[bam] device path: %.1f ms from the file's name to its last window (block tables from four stretches: %zu windows)\n", since(t_enter), stretched_windows.load());
	return true;
}

}  // namespace

bool read_file_on_device(FileIngest &file) {
	const RecordParser &parser = file.parser;
	const bool output = (file.tagged || file.filtered) && !file.source_output;      // (-b and -F under -r or -P: only behind BamController::set_device_source_output)
	if (parser.params_from_files && (!file.params || output)) { file.refusal = "read-parameter files (-r) are served by the host reader"; return false; }
	if (parser.gene_in_chromosome_name && (!file.device_sources || output)) { file.refusal = "gene = chromosome name is resolved by the host reader"; return false; }
	// (-b stays here whatever the container takes: a window it cannot take in bulk goes through records_through_host, record by record if need be)
	if (!file.tagged && !file.filtered && !file.container.bulk_ingest_possible_at_all(true)) { file.refusal = "the container no longer takes reads in bulk"; return false; }
	CellsDataContainer::IngestTarget target = file.container.next_read_target();
	if (file.filtered && !file.filtered->pieces.empty()) {      // -F over shards: the decoder sits with the shard that holds the file's first read, on its stream, as ingest does
		FilteredPass &P = *file.filtered;
		P.cur = P.shard_of(P.at);
		target.device = P.pieces[P.cur].device; target.stream = P.pieces[P.cur].stream;
	}
	const auto t_enter = clk::now();
	if (parser.tags.intronic_read_value.size() > 24 || parser.tags.intergenic_read_value.size() > 24) { file.refusal = "a read-type value is longer than 24 bytes"; return false; }
	// -r: the table on the GPU this file's decoder will sit on (a container over several GPUs may want another one than the table's: the claims
	// would have to be carried over -- the host reader takes the file instead)
	if (file.params && !file.params->table_on(target.device)) { file.refusal = "the read-parameter table cannot be held on this file's GPU"; return false; }
	if (file.params && file.filtered) filtered_pass_replay(file.filtered, *file.params);      // (before the pass's first file claims anything)
	DeviceFileReader reader(file, target, t_enter);
	return reader.read();
}

}  // namespace BamProcessing
}  // namespace Estimation
