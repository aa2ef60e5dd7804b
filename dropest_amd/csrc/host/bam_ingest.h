// bam_ingest.h -- BAM records -> CellsDataContainer::add_record, without BamTools.
//
// Mirrors the part of Estimation::BamProcessing that feeds the container:
//   BamController::parse_bam_file / process_alignment  (Estimation/BamProcessing/BamController.cpp:70-172)
//   FilledBamParamsParser::get_read_params (-f: CB / UB tags, FilledBamParamsParser.cpp:12-40)
//   ReadParamsParser::get_read_params (read name "id!CB#UMI", ReadParamsParser.cpp:20-33)
//   ReadParamsParser::get_gene / parse_read_type (gene tag + optional read-type tag, :36-90)
//   BamTags defaults (BamTags.cpp:7-24), Tools::ReadParameters quality check (Tools/ReadParameters.cpp:118-136)
//   ReadParamsParser::get_gene_from_reference (-g: gene annotation from a GTF / BED file, gene_annotation.h)
//   ReadMapParamsParser::get_read_params (-r: droptag's read-parameter files "name cb umi cb_quality umi_quality", gzip;
//     ReadMapParamsParser.cpp:22-48, :50-108; every name serves once)
//   FilteringBamProcessor::write_alignment / update_bam (-F: FilteringBamProcessor.cpp:61-110) through BamController::write_filtered_bam_files
// Tagged BAM output (-b: parse_bam_files(files, true, container)) and filtered BAM output (-F: write_filtered_bam_files) are written on the device
// path only.
//
// The container format: BGZF (gzip members with a 'BC' extra field, SAMv1 §4.1) holding the BAM stream (§4.2).
// Blocks are inflated by a pool of host threads, records are parsed in stream order by the caller's thread (the
// order of add_record calls defines cell, gene and UMI ids).  Host-only code; zlib.
#pragma once

#include <cstdint>
#include <memory>
#include <string>
#include <unordered_map>
#include <string_view>
#include <vector>

#include "facade.h"
#include "gene_annotation.h"

namespace Estimation {
namespace BamProcessing {

struct Parsed;       // bam_parse.h: one record as the controller's parser read it
struct FileIngest;   // bam_parse.h: what the readers of one file share

struct BamTags {   // BamTags.cpp:7-24 (defaults of the XML config)
	std::string cell_barcode = "CB", cell_barcode_raw = "CR", umi = "UB", umi_raw = "UR", gene = "GX";
	std::string cell_barcode_quality = "CQ", umi_quality = "UQ";
	std::string read_type, intronic_read_value, intergenic_read_value, exonic_read_value;
};

// One decoded alignment (the fields the path looks at)
struct BamRecord {
	int32_t ref_id = -1;
	int32_t position = -1;           // 0-based leftmost coordinate
	int32_t end_position = -1;       // BamAlignment::GetEndPosition(): position + reference bases consumed by the CIGAR (M, D, N, =, X)
	uint16_t flag = 0;
	std::string name;
	std::string_view name_view;      // set by parse_record (points into the window)
	const uint8_t *tags = nullptr;   // aux data, valid until the next record is read
	size_t tags_size = 0;
	bool is_mapped() const { return !(flag & 0x4); }
	bool is_primary() const { return !(flag & 0x100); }
	// Z / A / H tags as text (BamAlignment::GetTag(tag, std::string&)); false if absent or numeric
	bool get_string_tag(const std::string &tag, std::string &value, char *type = nullptr) const;
	bool get_string_tag(const std::string &tag, std::string_view &value, char *type = nullptr) const;   // view into `tags`
	// several tags in ONE walk over the aux data (the walk is most of a record's parse time when six tags are asked for one by
	// one): wanted[k] = the two tag letters packed as lo | hi << 8, 0 = not asked; same answers as get_string_tag per tag
	void get_string_tags(const uint16_t *wanted, int n_wanted, std::string_view *values, bool *found) const;
};

class BamReader {
	struct Impl;
	Impl *impl;
public:
	explicit BamReader(const std::string &path, unsigned threads = 0);   // throws std::runtime_error("Can't open BAM file: ...")
	~BamReader();
	BamReader(const BamReader &) = delete;
	BamReader &operator=(const BamReader &) = delete;
	const std::vector<std::string> &reference_names() const;
	const std::string &header_text() const;
	double file_over_first_batch() const;                                // file bytes / bytes the first decompressed batch covered (>= 1)
	bool next(BamRecord &rec);                                           // false at end of file
	// A run of whole records (as many as the decompressed window holds), valid until the next call of next / next_window;
	// offsets[i] = start of record i (its block_size field) relative to data
	bool next_window(const uint8_t *&data, std::vector<uint32_t> &offsets);
	static void parse_record(const uint8_t *at, BamRecord &rec);         // name is NOT copied: see name_view
};

class BamController {
public:
	struct Counters {
		size_t total_reads = 0, cant_parse = 0, low_quality = 0, saved = 0;
		double wait_ms = 0, parse_ms = 0, add_ms = 0;   // waiting for decompressed data / parallel record parsing / add_record (serial)
	};
	// -b: one `<input stem>.tagged.bam` that parse_bam_files(files, true, container) wrote
	struct TaggedFile {
		std::string name;
		size_t windows = 0, records = 0, inflated_bytes = 0, compressed_bytes = 0, batches = 0;
		double tag_ms = 0, deflate_ms = 0;              // the tag kernels (plan, scan, emit) and the compressor's launches, by device events
		size_t tag_bytes_in = 0, tag_bytes_out = 0;     // inflated bytes of the windows the tag kernels looked at, bytes they wrote
	};
	// -F: the one `<first input's stem>.filtered.bam` that write_filtered_bam_files wrote
	struct FilteredFile {
		std::string name;
		size_t windows = 0, total_reads = 0, written = 0;   // windows decoded; accepted alignments that reached write_alignment; those it wrote
		size_t wrong_genes = 0, wrong_umis = 0;              // FilteringBamProcessor::trace_state's numbers (dropest_read_correction_counts [3], [4])
		size_t inflated_bytes = 0, compressed_bytes = 0, batches = 0;
		double decode_ms = 0, tag_ms = 0, deflate_ms = 0;    // the decoder's kernels and copies, the tag kernels, the compressor's launches: by device events
		double decisions_ms = 0;                             // host time of the read corrections (one context's, or all shards'), paid once before the first file
	};
private:
	BamTags _tags;
	struct ReadParams { std::string cb, umi, umi_quality; bool pass_quality; };
	std::unordered_map<std::string, ReadParams> _read_params;     // -r: read name -> parameters (erased when served); built when the host reader first takes a file
	bool _params_from_files = false;
	std::shared_ptr<struct ParamSource> _param_source;            // -r: the files' inflated text and, on the device path, its table (bam_parse.h)
	bool _read_params_mapped = false;
	bool _device_read_sources = false, _device_source_output = false;
	void load_read_params(const std::string &filenames);
	void map_read_params();
	void serve_read_params(Parsed &pr);
	void add_record_by_record(FileIngest &file, const uint8_t *data, const std::vector<uint32_t> &offsets, std::vector<Parsed> &parsed);
	void read_file_on_host(FileIngest &file, bool first_file);
	bool _filled_bam, _gene_in_chromosome_name;
	int _min_barcode_phred;
	unsigned _threads;
	bool _device_decode = false;
	bool _sharded_filtered_output = false;
	Counters _counters;
	std::vector<TaggedFile> _tagged;
	FilteredFile _filtered;
	std::vector<size_t> _saved_per_file;             // accepted reads of every file of the last parse_bam_files call, for write_filtered_bam_files' guard
	Tools::GeneAnnotation::RefGenesContainer _genes;   // -g: empty unless a GTF / BED file was given
public:
	// gtf_path: GTF / BED annotation (-g), "" = genes come from the BAM's gene tag; read_param_filenames must be empty (not built)
	BamController(const BamTags &tags, bool filled_bam, const std::string &read_param_filenames, const std::string &gtf_path,
	              bool gene_in_chromosome_name, int min_barcode_phred, unsigned threads = 0);
	// BamController::parse_bam_files with a BamProcessor: every accepted read reaches container.add_record in file order
	void parse_bam_files(const std::vector<std::string> &bam_files, CellsDataContainer &container);
	// The reference's signature.  print_result_bams (-b): every accepted alignment of every file is also written, in file order, to
	// `<input stem>.tagged.bam` in the current directory (BamProcessor::get_result_bam_name, BamProcessorAbstract::update_bam), with its gene, raw
	// barcode ("CR"), raw UMI ("UR"), quality strings and read type as Z tags (BamProcessorAbstract::save_alignment; DESIGN.md section 7 has the
	// rule).  The records are edited on the device (csrc/k_bamtag.h) and compressed there (include/dropest_deflate.h), so the device reader is used
	// whether or not DROPEST_BAM_DEVICE is set, and what it refuses -- -r parameter files and gene = chromosome name (unless
	// set_device_source_output is on), a read-type value over 24 bytes, no GPU -- throws std::runtime_error naming the reason: the host reader
	// does not write BAM.  false: the call above.
	void parse_bam_files(const std::vector<std::string> &bam_files, bool print_result_bams, CellsDataContainer &container);
	const std::vector<TaggedFile> &tagged_files() const { return _tagged; }   // of the last parse_bam_files call
	// BamController::write_filtered_bam_files (BamController.cpp:38-48; -F), after container.merge_and_filter(): the same files are read again, and
	// every accepted alignment that FilteringBamProcessor::write_alignment writes -- the container's verdict for it is "written"
	// (dropest_read_corrections, include/dropest_amd.h) -- goes out with the edits of -b and, behind them, the target cell's barcode
	// (BamTags::cell_barcode) and the corrected UMI (BamTags::umi) as Z tags (DESIGN.md section 7 has the rule).  As in the reference
	// (FilteringBamProcessor::update_bam, :103-110: only the first input opens a writer) there is ONE output, `<first input's stem>.filtered.bam`
	// in the current directory, with the first file's header, and the written records of ALL inputs follow in order.  The records are decoded,
	// edited and compressed on the device and nothing is added to the container; read i of the container is the i-th record the files'
	// readers accept, so the files must be the ones the container was filled from, in that order: a window that would pass the container's
	// read count, or a final count that differs from it, throws std::runtime_error saying so; and when this controller filled the container
	// (its last parse_bam_files call accepted exactly the container's reads) every file must bring the reads it brought then.  Device path only, like -b: -r parameter files
	// and gene = chromosome name (unless set_device_source_output is on), a read-type value over 24 bytes, no GPU throw naming the reason; a sharded or split container (unless
	// set_sharded_filtered_output is on) and UMI-dictionary mode throw with the read corrections' own message.
	void write_filtered_bam_files(const std::vector<std::string> &bam_files, CellsDataContainer &container);
	// -F over a sharded or split container (off by default: write_filtered_bam_files then refuses such a container as before).  On: the shards
	// compute their reads' decisions (dropest_shard_group_read_corrections), every window is filtered under the pieces of them that the shards'
	// resident ranges cut out of it (dropest_bam_decoder_filter_window_segments), each file's decoder sits on the GPU and stream of the shard that
	// holds the file's first read, and the one output is what one context would have written.  What the shards' read corrections refuse
	// (UMI-dictionary mode, a molecule key wider than 64 bits, ...) throws in their words.  DESIGN.md section 7.
	void set_sharded_filtered_output(bool on) { _sharded_filtered_output = on; }
	const FilteredFile &filtered_file() const { return _filtered; }           // of the last write_filtered_bam_files call (empty when it threw)
	// BGZF inflate, record chain and tag walk on the container's GPU (include/dropest_bgzf.h) where the configuration allows it: tags or read
	// names as the source of barcode / UMI, the gene tag or a -g annotation (annotation_api.hip) as the source of the gene; with -r or gene =
	// chromosome name only behind set_device_read_sources (otherwise the host reader runs).  A sharded container is fed by one decoder on the GPU of the shard the file's first read goes to.
	// CRC-32 and ISIZE of every block are checked there too.  DROPEST_BAM_DEVICE=1 in the environment does the same.
	void set_device_decode(bool on) { _device_decode = on; }
	// The device BAM path also takes files under -r (read-parameter files) and -P (gene = chromosome name) for INGEST (off by default: such files
	// go to the host reader, as before).  -r: the files' rows become a table on the container's GPU (include/dropest_bgzf.h:
	// dropest_read_params_*), probed by every record's name there, each row serving the first record of the stream that asks, as the host
	// reader's map does; -P: the reference's name is the gene, a constant per record.  The answer is the host reader's.  Tagged and filtered
	// output (-b, -F) under -r or -P stay refused unless set_device_source_output is on as well.  A file the device path cannot take after all (no GPU, a container over several
	// GPUs whose next read lives on another GPU than the table) goes to the host reader with the rows the device served taken out of its map;
	// from then on the host reader serves every later file.  DESIGN.md section 7.
	void set_device_read_sources(bool on) { _device_read_sources = on; }
	// Tagged and filtered output (-b, -F) under -r and -P, on the device path (off by default: both are refused with the texts they always had; on,
	// together with set_device_read_sources).  -r: the raw barcode, the raw UMI and the UMI quality tag of a written record are the fields of the
	// row the record was served, as they stand in the line; NO barcode quality tag is written (ReadParametersEfficient::parameters answers "" for
	// it) and an entry of that name stays in the record.  -P: the gene tag is the reference's name and the read is exonic; an empty name writes
	// neither tag.  -F serves the rows afresh from the first file on, as the reference's new parser does, on claims of its own: the ingest's
	// claims are what they were when the call returns or throws.  Still refused, with the reason: a table that cannot be held on the file's GPU,
	// parameter files the host reader has served from, and what the read corrections refuse (UMI-dictionary mode).  DESIGN.md section 7.
	void set_device_source_output(bool on) { _device_source_output = on; }
	// the device path keeps one decoder per GPU (streams, 2-7 GB of device buffers, up to 512 MB of pinned staging) between the files of one
	// parse_bam_files call; they are given back on a helper thread when the call ends (DROPEST_BAM_KEEP_DECODERS=1: kept for the next call).
	// This waits for that thread and frees whatever is still cached.
	static void release_device_decoders();
	const Counters &counters() const { return _counters; }
};

}  // namespace BamProcessing
}  // namespace Estimation
