// bam_decoder.h -- the device BAM decoder of include/dropest_bgzf.h (dropest_bam_decoder_*): its state, grouped by what it is for; the helpers
// every group of calls shares; the life cycle and the buffer sizing.  Included by bgzf_api.hip alone, behind its error plumbing and the
// inflate scratch pool; the calls are in bam_decoder_dict.h, _upload.h, _window.h, _fetch.h and _tag.h.
#pragma once

// ---- helpers --------------------------------------------------------------------------------------------------------------------------------
// a stretch of host time, for the ms_* figures of a window and the [bam] traces
struct BamLap {
	using clk = std::chrono::steady_clock;
	clk::time_point t0 = clk::now();
	double ms() const { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }
	double next() { const double v = ms(); t0 = clk::now(); return v; }      // ... and the next stretch begins
};

// Small arrays between pinned host memory and the device by a kernel's own loads and stores, any number of them in one launch, one element of
// each per lane.  Not by copies: a hipMemcpyAsync of ~50 KB took 4-8 ms whenever the runtime's staging had to grow (five of them out of pageable
// vectors per window; three the first time a process made them), and a copy to the host queues behind the next window's 80 MB on their way
// in (dropest_bam_decoder_upload): the chain took 0.75 instead of 0.25 ms per window.
template <class T> struct BamFromHost { const T *h; T *__restrict__ d; __device__ void move(uint32_t k) const { d[k] = h[k]; } };
template <class T> struct BamToHost { const T *__restrict__ d; T *h; __device__ void move(uint32_t k) const { h[k] = d[k]; } };
template <class T> BamFromHost<T> from_host(const T *h, T *d) { return {h, d}; }
template <class T> BamToHost<T> to_host(const T *d, T *h) { return {d, h}; }
template <class... P> __global__ __launch_bounds__(256) void bam_copy_kernel(uint32_t n, P... pair) {
	const uint32_t k = blockIdx.x * 256 + threadIdx.x;
	if (k < n) (pair.move(k), ...);
}
template <class... P> static void bam_copy(hipStream_t st, uint32_t n, P... pair) {
	if (!n) return;      // (a grid of no workgroup is a launch error)
	hipLaunchKernelGGL((bam_copy_kernel<P...>), dim3((n + 255) / 256), dim3(256), 0, st, n, pair...);
	HIP_CHECK(hipGetLastError());
}

// src[0 .. n) into a pinned buffer (`what`, for the error) at byte `at` rounded up to `align`; `at` moves behind it.  No room is an error: the
// caller sizes the buffer first -- growing it here would move what was put before.  Arrays put in falling order of their elements' size need
// no padding.
template <class T, class B> static T *pinned_put(PinnedBuf<B> &buf, size_t &at, const T *src, size_t n, const char *what, size_t align = alignof(T)) {
	const size_t from = (at + align - 1) & ~(align - 1), bytes = n * sizeof(T);
	if (from + bytes > buf.n * sizeof(B)) throw InvalidError(std::string("internal: ") + what + " is too small");
	T *const to = reinterpret_cast<T *>(reinterpret_cast<uint8_t *>(buf.p) + from);
	std::memcpy(to, src, bytes);
	at = from + bytes;
	return to;
}

// ---- the state ------------------------------------------------------------------------------------------------------------------------------
// What the first half of a window produces (copy in, inflate, the chain of records) and the second half (fields, dense columns) consumes.  Two of
// them: the caller may run the first half of window k + 1 on another thread while the second half of window k and its own work go on.
struct BamFront {
	hipStream_t stream = nullptr;
	DevBuf<uint8_t> d_in, d_out;
	DevBuf<uint64_t> d_in_off, d_out_off, seg_start, seg_exit;
	DevBuf<uint32_t> d_in_len, d_out_len, d_status, d_crc, seg_count, seg_base, d_bad, d_list;
	PinnedBuf<uint64_t> h_seg_start, h_seg_exit;
	PinnedBuf<uint32_t> h_count, h_block_status, h_base;
	PinnedBuf<uint64_t> h_tab;      // the window's block table on its way to the device: in_off | out_off | in_len, out_len, crc (28 bytes a block)
	bgzf::BlockTable tab;
	uint64_t data_len = 0, tail_start = 0, n_rec = 0;
	uint32_t n_segs = 0, n_blocks = 0, refused = 0, repaired = 0;
	double ms_copy = 0, ms_inflate = 0, ms_boundaries = 0;
	bool begun = false;
	// the window's data stand at d_out + base_off: [the record the window before cut off | the inflated blocks].  The blocks are inflated to
	// d_out + reserve BEFORE the window before has said how long its cut-off record is (dropest_bam_decoder_window_inflate: the inflate of window
	// k + 1 runs beside the chain / parse / host work of window k); the record is put in front of them afterwards (.._window_chain).
	uint64_t base_off = 0, reserve = 0, total = 0, comp_len = 0;
	const uint8_t *comp = nullptr;
	bool inflating = false;
	uint8_t *data() { return d_out.p + base_off; }
	// room for n blocks / n segments (the device's arrays with `margin` more, so that the next, slightly larger window does not grow them again)
	void size_blocks(size_t n, size_t margin) {
		const size_t c = n + margin;
		d_in_off.ensure(c); d_out_off.ensure(c); d_in_len.ensure(c); d_out_len.ensure(c); d_status.ensure(c); d_crc.ensure(c);
		h_block_status.ensure(n);
		h_tab.ensure(n * 4 + 8);      // (words of 8 bytes: 2 n for the offsets, 1.5 n for the three 32-bit arrays)
	}
	void size_segments(size_t n, size_t margin) {
		const size_t c = n + margin;
		seg_start.ensure(c); seg_exit.ensure(c); seg_count.ensure(c); seg_base.ensure(c); d_bad.ensure(2); d_list.ensure(1);
		h_seg_start.ensure(n); h_seg_exit.ensure(n); h_count.ensure(n); h_base.ensure(c);
	}
};

// The host's dictionaries on the device (BamDict): gene-name hashes -> indices, reference -> chromosome, with -g the annotation's two tables
struct BamDictionaries {
	DevBuf<unsigned long long> g_keys;
	DevBuf<uint32_t> g_vals, g_name_off;      // g_name_*: the dictionary's gene names by index (dropest_bam_decoder_set_gene_names), 0 names: hashes alone
	DevBuf<uint8_t> g_name_pool;
	DevBuf<int32_t> d_chr, d_ann_chr, d_ann_id;
	PinnedBuf<uint8_t> h_dict;                // the tables on their way to the device (bam_to_device)
	dropest_annotation *annotation = nullptr;   // -g: not owned
	uint32_t g_mask = 0, n_gene_names = 0, n_ann_genes = 0;
	unsigned long long hash_mask = ~0ull;
	bool fresh = true;                        // the empty dictionaries' memsets have not been queued yet (they wait for the decoder's stream)
	void reset(int n_refs) { annotation = nullptr; n_ann_genes = 0; n_gene_names = 0; d_chr.ensure(size_t(std::max(1, n_refs))); }
	BamDict args() const {
		return BamDict{g_keys.p, g_vals.p, g_mask, d_chr.p, annotation ? d_ann_chr.p : nullptr, annotation ? d_ann_id.p : nullptr,
		               n_gene_names ? g_name_off.p : nullptr, g_name_pool.p, n_gene_names, hash_mask};
	}
};

// A window's records one by one: where each begins, its fields (BamRecordOut), the tiles' counts, the window's counters
struct BamRecords {
	DevBuf<uint64_t> off;
	DevBuf<unsigned long long> cb, umi, qoff;
	DevBuf<uint32_t> gene, aux, uql, tile_ok, tile_need, d_totals;
	DevBuf<uint8_t> status, need;
	DevBuf<BamWindowCounts> d_wc;
	PinnedBuf<uint32_t> h_result;             // a window's counters, totals and flag (13 words)
};
// -g: what the annotation query takes and answers, per record
struct BamAnnotated {
	DevBuf<int32_t> chr, mark;
	DevBuf<uint32_t> pos, end, gene;
};
// The accepted records made dense (BamDense), and the list of those the host must see
struct BamDenseColumns {
	DevBuf<unsigned long long> cb, umi, qoff;
	DevBuf<uint32_t> gene, aux, need_rec, need_pos, need_size;
	DevBuf<uint8_t> qual;
	PinnedBuf<uint32_t> h_need_rec, h_need_pos, h_need_size;
	PinnedBuf<uint8_t> h_qual;
	BamDense args() const { return BamDense{cb.p, umi.p, gene.p, aux.p, need_rec.p, need_pos.p, need_size.p, qoff.p}; }
};
// Pinned staging of fetch_records and the two patch calls: the kernels read and write it themselves
struct BamGather {
	PinnedBuf<uint32_t> h_idx, h_size;
	PinnedBuf<uint64_t> h_off, h_patch;
	PinnedBuf<uint8_t> h_bytes;
};

// The compressed bytes of a window on their way to the device ahead of the window call (dropest_bam_decoder_upload), out of a staging buffer or
// out of pinned pieces (dropest_bam_decoder_pieces): the bytes go piece by piece, so that the pinned memory (0.15-0.4 ms per MB to allocate) does
// not grow with the window.
struct BamUpload {
	hipStream_t stream = nullptr;      // the device's null stream (see dropest_bam_decoder::stream)
	PinnedBuf<uint8_t> h_stage[2];
	PinnedBuf<uint8_t> piece_mem;      // one allocation (each has a fixed cost of a few ms), cut into the pieces
	uint32_t n_pieces = 0;
	uint64_t piece_bytes = 0;
	std::vector<hipEvent_t> piece_done;
	bool begun[2] = {false, false};
	std::atomic<const uint8_t *> host[2] = {{nullptr}, {nullptr}};   // the host bytes that in[w] holds (or will, once done[w] has passed)
	hipEvent_t done[2] = {nullptr, nullptr};
	DevBuf<uint8_t> in[2];
	uint64_t len[2] = {0, 0};
	std::atomic<bool> ready[2] = {{false}, {false}};   // written by the reader thread (publish_upload), read by the window call: release / acquire around len / blocks
	// ... and their block table, made by the same caller (a walk from header to header is one cache miss per block: ~2 ms per 64 MB window)
	bgzf::BlockTable blocks[2];
	void reset() { for (int w = 0; w < 2; ++w) { ready[w].store(false, std::memory_order_relaxed); host[w].store(nullptr, std::memory_order_relaxed); } }
};

// -b and -F (dropest_bam_decoder_set_tagging / _tag_window, _set_filtering / _filter_window; k_bamtag.h): the output configuration, the
// annotation's gene names under -g, the sizes and offsets of the last window's output records and the output itself
struct BamTagging {
	bool on = false, has_names = false;
	BamTagCfg cfg{};
	DevBuf<uint32_t> name_off, size, tile_written, flags;
	DevBuf<uint8_t> name_pool, out;
	DevBuf<unsigned long long> tile_bytes;
	DevBuf<uint64_t> off;
	PinnedBuf<unsigned long long> h_tag;    // all bytes, records written, flags: stored by the scan kernel
	uint32_t n_names = 0;
	uint64_t len = 0;                       // bytes of the last tagged window in `out`
	hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};      // around plan + scan, around emit
	bool pending = false;                   // the last emit's flag and time have not been looked at yet (tag_collect, after a wait that is made anyway)
	double ms = 0;                          // plan + scan + emit by device events, since the decoder was created or reset
	uint64_t bytes_in = 0, bytes_out = 0;
	// -F (dropest_bam_decoder_set_filtering / _filter_window): the two corrected tags' names, every cell's barcode code (the caller's device array,
	// or `codes`, a copy of its host array), the side strings of escaped codes, each record's rank among the accepted ones, and a window's
	// decisions when they come from host arrays (through h_fix, pinned).  _filter_window_segments: the segment table (through h_seg, pinned, to
	// `seg`); umi / cell / verdict are then the staging of segments whose arrays live on another GPU (or of all, under the test switch)
	struct Filtering {
		bool on = false;
		uint32_t out_tag[2] = {0, 0}, n_cells = 0, n_side = 0;
		const uint64_t *cell_barcode = nullptr;
		DevBuf<uint64_t> codes, umi;
		DevBuf<uint32_t> side_off, rank, tile_ok, total, cell;
		DevBuf<uint8_t> side_pool, verdict;
		DevBuf<BamTagSeg> seg;
		PinnedBuf<uint64_t> h_fix;
		PinnedBuf<BamTagSeg> h_seg;
	} filt;
	void reset() { on = false; has_names = false; pending = false; len = 0; ms = 0; bytes_in = bytes_out = 0; filt.on = false; }      // (the names were the annotation's)
};

// The two sources beside a record's own tags and name (k_bamparse.h: BamSources): the caller's read-parameter table (-r; not owned) with the
// stream ordinal of the next window's first record, and the reference -> gene table of -P.  A reset drops both, as it drops the annotation.
// ref_off / ref_pool: the references' names for the tag kernels under -P (dropest_bam_decoder_set_reference_names); a reset drops them too.
struct BamSourceState {
	dropest_read_params *table = nullptr;
	uint64_t first_ordinal = 0, seen = 0;      // seen: records of the windows finished since the table was given
	bool ref_gene = false;
	DevBuf<uint32_t> rp_row;
	DevBuf<int32_t> gene_of_ref;
	PinnedBuf<uint32_t> h_rp_row;
	DevBuf<uint32_t> ref_off;
	DevBuf<uint8_t> ref_pool;
	uint32_t n_ref_names = 0;
	bool has_ref_names = false;
	void reset() { table = nullptr; first_ordinal = seen = 0; ref_gene = false; has_ref_names = false; n_ref_names = 0; }
	int bits() const { return (table ? BAM_SRC_PARAMS : 0) | (ref_gene ? BAM_SRC_REF_GENE : 0); }
};

// Where the file's windows stand: the record the last chain cut off, the fronts' turns, what the last finished window holds
struct BamProgress {
	uint64_t tail_len = 0, last_n_rec = 0, last_n_ok = 0;
	int next_front = 0, last_front = 0;
};

struct dropest_bam_decoder {
	int device = 0;
	// Two streams: `stream` for the kernels and the small copies, `up.stream` for the compressed bytes on their way in under the kernels of the
	// window before.  A stream is 8-20 ms to create (and its first dispatch as much again), and every other HIP call of the process waits
	// meanwhile -- measured three ways in round 6 (created up front: 16 ms; on a helper thread beside the pinned allocation: the allocation runs,
	// hipMalloc and the reader's first copies wait, nothing gained; NOTES_r06 section 7).  So the decoder creates none unless it has to:
	// `stream` is LENT by the caller for a file (dropest_bam_decoder_use_stream: the container's own, which exists and has run kernels; a
	// decoder that is lent none makes one when first needed), and the uploads take the device's null stream, which the non-blocking streams
	// do not wait for.
	hipStream_t stream = nullptr;
	hipStream_t own_stream = nullptr;      // `stream` is this one, or the caller's
	std::mutex ready_mutex;
	BamParseCfg cfg{};
	BamFront front[2];
	BamProgress at;
	DevBuf<uint8_t> d_tail;                // at.tail_len bytes: the record the last chain cut off
	bool traced_first = false;
	bool halves_in_sequence = false;       // dropest_bam_decoder_window is running: its first half uses `stream`
	BamDictionaries dict;
	BamRecords rec;
	BamAnnotated ann;
	BamDenseColumns dense;
	BamGather gather;
	BamUpload up;
	BamTagging tag;
	BamSourceState src;

	BamFront &last() { return front[at.last_front]; }
	// room for n records in tiles of BAM_FIN_TILE (`tiles` of them); the annotation's columns when there is one
	void size_records(size_t n, size_t tiles) {
		rec.off.ensure(n); rec.cb.ensure(n); rec.umi.ensure(n); rec.gene.ensure(n); rec.aux.ensure(n); rec.uql.ensure(n); rec.qoff.ensure(n); rec.status.ensure(n); rec.need.ensure(n);
		dense.cb.ensure(n); dense.umi.ensure(n); dense.gene.ensure(n); dense.aux.ensure(n); dense.qoff.ensure(n); dense.need_rec.ensure(n); dense.need_pos.ensure(n); dense.need_size.ensure(n);
		rec.tile_ok.ensure(tiles); rec.tile_need.ensure(tiles); rec.d_totals.ensure(2); rec.d_wc.ensure(1);
		if (dict.annotation) { ann.chr.ensure(n); ann.pos.ensure(n); ann.end.ensure(n); ann.gene.ensure(n); ann.mark.ensure(n); }
		if (src.table) src.rp_row.ensure(n);
	}
	BamRecordOut record_out() const { return BamRecordOut{rec.cb.p, rec.umi.p, rec.gene.p, rec.aux.p, rec.uql.p, rec.qoff.p, rec.status.p, rec.need.p, ann.chr.p, ann.pos.p, ann.end.p}; }
};

// empty dictionaries: every gene and chromosome is new
static void queue_empty_dictionaries(dropest_bam_decoder *d) {
	HIP_CHECK(hipMemsetAsync(d->dict.g_vals.p, 0, size_t(d->dict.g_mask + 1) * 4, d->stream));
	HIP_CHECK(hipMemsetAsync(d->dict.d_chr.p, 0xFF, d->dict.d_chr.n * 4, d->stream));
}

// The decoder's stream exists from here on (a decoder that was lent none makes its own now)
static void bam_ready(dropest_bam_decoder *d) {
	std::lock_guard<std::mutex> lk(d->ready_mutex);
	if (!d->stream) {
		if (!d->own_stream) HIP_CHECK(hipStreamCreateWithFlags(&d->own_stream, hipStreamNonBlocking));
		d->stream = d->own_stream;
	}
	if (d->dict.fresh) { queue_empty_dictionaries(d); d->dict.fresh = false; }
}

static void check_cfg(const dropest_bam_parse_cfg *cfg) {
	if (cfg->intronic_len > 24 || cfg->intergenic_len > 24) throw InvalidError("read-type values longer than 24 characters");
	if (cfg->n_refs < 0) throw InvalidError("negative number of references");
}

// ---- life cycle -----------------------------------------------------------------------------------------------------------------------------
extern "C" int dropest_bam_decoder_create(int device, const dropest_bam_parse_cfg *cfg, dropest_bam_decoder **out) {
	return bgzf_guarded([&] {
		if (!cfg || !out) throw InvalidError("null argument");
		int n_dev = 0;
		if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) throw DeviceError("no such GPU: the BAM decoder has no CPU implementation");
		HIP_CHECK(hipSetDevice(device));
		static_assert(sizeof(dropest_bam_parse_cfg) == sizeof(BamParseCfg), "the C struct and the kernels' struct are one layout");
		check_cfg(cfg);
		auto *d = new dropest_bam_decoder();
		d->device = device;
		std::memcpy(&d->cfg, cfg, sizeof(BamParseCfg));
		if (const char *e = getenv("DROPEST_BAM_TEST_GENE_HASH_BITS")) { const int b = atoi(e); if (b > 0 && b < 64) d->dict.hash_mask = (1ull << b) - 1ull; }   // (tests: names that collide)
		try {
			const bool trace = getenv("DROPEST_BAM_TRACE") != nullptr;
			BamLap t;
			auto lap = [&](const char *what) { if (trace) std::fprintf(stderr, "[bam] decoder: %s %.1f ms\n", what, t.next()); };
			// (room for 32 000 genes and their names from the start: growing these tables between two windows is a hipFree, a hipMalloc and a pinned
			// reallocation -- ~10 ms of "dictionaries to the device" in the window that first knows a few thousand genes)
			BamDictionaries &D = d->dict;
			D.g_mask = 1023; D.g_keys.alloc(size_t(1) << 16); D.g_vals.alloc(size_t(1) << 16); D.d_chr.alloc(size_t(std::max(1, cfg->n_refs)));
			D.g_name_off.ensure(size_t(1) << 15); D.g_name_pool.ensure(size_t(1) << 20); D.h_dict.ensure(size_t(2) << 20);
			lap("dictionary buffers");
			for (hipEvent_t &e : d->up.done) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
			lap("events");
		} catch (...) { delete d; throw; }
		*out = d;
	});
}

// A decoder taken up again for another file (its buffers, streams and pinned memory stay): the parse configuration of that file, empty
// dictionaries, no annotation, no tagging, no record carried over.
extern "C" int dropest_bam_decoder_reset(dropest_bam_decoder *d, const dropest_bam_parse_cfg *cfg) {
	return bgzf_guarded([&] {
		if (!d || !cfg) throw InvalidError("null argument");
		check_cfg(cfg);
		HIP_CHECK(hipSetDevice(d->device));
		bam_ready(d);
		HIP_CHECK(hipStreamSynchronize(d->stream));
		for (BamFront &f : d->front) { if (f.stream) HIP_CHECK(hipStreamSynchronize(f.stream)); f.begun = false; f.inflating = false; }
		HIP_CHECK(hipStreamSynchronize(d->up.stream));
		std::memcpy(&d->cfg, cfg, sizeof(BamParseCfg));
		d->up.reset(); d->at = BamProgress{}; d->tag.reset(); d->src.reset(); d->dict.reset(cfg->n_refs);
		queue_empty_dictionaries(d);
		HIP_CHECK(hipStreamSynchronize(d->stream));
	});
}

// BGZF blocks the device inflates at once (a wave each, INF_WAVES_PER_EU per SIMD): a window of that many blocks takes as long as one of fewer
extern "C" uint32_t dropest_bam_decoder_wave_slots(const dropest_bam_decoder *d) {
	if (!d) return 0;
	hipDeviceProp_t prop{};
	if (hipGetDeviceProperties(&prop, d->device) != hipSuccess) return 0;
	return uint32_t(prop.multiProcessorCount) * 4u * uint32_t(INF_WAVES_PER_EU);
}

// The decoder's kernels and small copies run on `stream` (a hipStream_t of the decoder's device) from now on -- the caller's own, which exists and
// has run kernels, instead of one the decoder would have to create (~16 ms with its first dispatch).  NULL: back to a stream of the decoder's own
// (made when first needed); call that before the lent stream goes away.  Not while a window is in flight.
extern "C" int dropest_bam_decoder_use_stream(dropest_bam_decoder *d, void *stream) {
	return bgzf_guarded([&] {
		if (!d) throw InvalidError("null argument");
		HIP_CHECK(hipSetDevice(d->device));
		std::lock_guard<std::mutex> lk(d->ready_mutex);
		if (getenv("DROPEST_BAM_TRACE_SYNC")) {      // (development: which stream still has work when a file is done)
			BamLap t;
			(void)hipStreamSynchronize(d->up.stream);
			std::fprintf(stderr, "[bam] use_stream: the upload stream waited for %.1f ms\n", t.next());
			if (d->stream) (void)hipStreamSynchronize(d->stream);
			std::fprintf(stderr, "[bam] use_stream: the kernels' stream waited for %.1f ms\n", t.ms());
		}
		if (d->stream) HIP_CHECK(hipStreamSynchronize(d->stream));
		if (d->stream && d->stream != hipStream_t(stream)) bgzf_release_inflate_scratch(d->device, d->stream);      // (a stream let go of keeps no scratch of the decoder's)
		d->stream = stream ? hipStream_t(stream) : d->own_stream;      // (null: bam_ready makes the decoder's own)
	});
}

extern "C" void *dropest_bam_decoder_stream(dropest_bam_decoder *d) {
	if (!d || hipSetDevice(d->device) != hipSuccess) return nullptr;
	try { bam_ready(d); } catch (...) { return nullptr; }
	return d->stream;
}

extern "C" void dropest_bam_decoder_destroy(dropest_bam_decoder *d) {
	if (!d) return;
	(void)hipSetDevice(d->device);
	(void)hipStreamSynchronize(d->up.stream);
	for (hipEvent_t e : d->up.done) if (e) (void)hipEventDestroy(e);
	for (hipEvent_t e : d->up.piece_done) if (e) (void)hipEventDestroy(e);
	for (hipEvent_t e : d->tag.ev) if (e) (void)hipEventDestroy(e);
	// the inflate scratch of every stream the decoder inflated on (a lent one it still holds, its own, its fronts')
	if (d->stream && d->stream != d->own_stream) bgzf_release_inflate_scratch(d->device, d->stream);
	if (d->own_stream) bgzf_release_inflate_scratch(d->device, d->own_stream);
	for (BamFront &f : d->front) if (f.stream) bgzf_release_inflate_scratch(d->device, f.stream);
	if (d->own_stream) { (void)hipStreamSynchronize(d->own_stream); (void)hipStreamDestroy(d->own_stream); }
	for (BamFront &f : d->front) if (f.stream) { (void)hipStreamSynchronize(f.stream); (void)hipStreamDestroy(f.stream); }
	delete d;
}

// ---- buffer sizing --------------------------------------------------------------------------------------------------------------------------
// Room on the device for windows of `bytes` compressed bytes in front `which`, up front (a BAM inflates ~4-12 x, a record is >= ~120 bytes), so that
// the first windows do not grow every buffer step by step (each growth is a free + an allocation that wait for the device)
static void bam_reserve(dropest_bam_decoder *d, int which, uint64_t bytes, uint64_t out_hint = 0) {
	BamFront &F = d->front[which];
	// (14 x when the caller does not know better: 2 x 1.8 GB for windows of 128 MB, 1-2 ms on most boxes and 130 ms on some)
	const uint64_t out_bytes = out_hint ? out_hint + out_hint / 8 + (uint64_t(1) << 20) : bytes * 14, n_rec = out_bytes / 120;
	F.d_in.ensure(bytes + 8); F.d_out.ensure(out_bytes);
	d->up.in[which].ensure(bytes + 8);
	F.size_blocks(bytes / 2048 + 1024, 0);
	F.size_segments(out_bytes / BAM_SEG + 16, 0);
	if (which == 0) d->size_records(n_rec, n_rec / BAM_FIN_TILE + 2);
}
