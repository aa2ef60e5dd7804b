// bam_decoder_tag.h -- -b and -F: the accepted records of the LAST finished window with their tags edited; under -F only those the container's
// decision writes, with the corrected barcode and UMI behind the other tags (k_bamtag.h; the state: BamTagging, bam_decoder.h).  The decisions come
// as one array (_filter_window: one context's) or in segments (_filter_window_segments: the shards' of a sharded run, one table entry each)
#pragma once

extern "C" int dropest_bam_decoder_set_tagging(dropest_bam_decoder *d, const dropest_bam_tag_cfg *cfg) {
	return bgzf_guarded([&] {
		if (!d) throw InvalidError("null argument");
		BamTagging &T = d->tag;
		T.on = false; T.has_names = false; T.len = 0; T.filt.on = false;      // (-F is configured behind -b: its names are checked against these)
		if (!cfg) return;
		static_assert(sizeof(BamTagCfg) == 12 + 12 + 72, "the C struct's first members and the kernels' struct are one layout");
		for (int k = 0; k < 3; ++k) if (cfg->type_len[k] > 24) throw InvalidError("read-type values longer than 24 characters");
		if (!cfg->out_tag[1] || !cfg->out_tag[2]) throw InvalidError("the raw barcode and raw UMI tags need two-letter names");
		if (cfg->n_gene_names && (!cfg->gene_name_off || !cfg->gene_name_pool)) throw InvalidError("null argument");
		HIP_CHECK(hipSetDevice(d->device));
		bam_ready(d);
		HIP_CHECK(hipStreamSynchronize(d->stream));
		for (int k = 0; k < 5; ++k) T.cfg.out_tag[k] = cfg->out_tag[k];
		T.cfg.type_tag = cfg->type_tag;
		for (int k = 0; k < 3; ++k) { T.cfg.type_len[k] = cfg->type_len[k]; std::memcpy(T.cfg.type_val[k], cfg->type_val[k], 24); }
		if (cfg->n_gene_names) {
			const uint32_t n = cfg->n_gene_names, bytes = cfg->gene_name_off[n];
			for (uint32_t g = 0; g < n; ++g) if (cfg->gene_name_off[g] > cfg->gene_name_off[g + 1]) throw InvalidError("the gene names' offsets must not decrease");
			T.name_off.ensure(size_t(n) + 1); T.name_pool.ensure(size_t(bytes) + 16);
			d->dict.h_dict.ensure((size_t(n) + 1) * 4 + size_t(bytes) + 128);
			size_t at = 0;
			bam_to_device(d, T.name_off.p, cfg->gene_name_off, (size_t(n) + 1) * 4, at);
			if (bytes) bam_to_device(d, T.name_pool.p, cfg->gene_name_pool, bytes, at);
			HIP_CHECK(hipStreamSynchronize(d->stream));
			T.n_names = n; T.has_names = true;
		}
		T.on = true;
	});
}

// After a wait on the decoder's stream: the last emit's size flag and its time by the device's events
static void tag_collect(dropest_bam_decoder *d) {
	BamTagging &T = d->tag;
	if (!T.pending) return;
	T.pending = false;
	float ms = 0;
	HIP_CHECK(hipEventElapsedTime(&ms, T.ev[2], T.ev[3]));
	T.ms += ms;
	if (uint32_t(T.h_tag.p[3]) & BAMTAG_FLAG_SIZE) throw DeviceError("internal: a tagged record did not have the size that was planned for it");
}

// -g: the host's answer for records whose gene the annotation query left to it, before the window is tagged (again)
extern "C" int dropest_bam_decoder_patch_annotation(dropest_bam_decoder *d, const uint32_t *rec, const uint32_t *ann_gene, const uint32_t *mark, uint32_t n) {
	return bgzf_guarded([&] {
		if (!d || (n && (!rec || !ann_gene || !mark))) throw InvalidError("null argument");
		if (!d->dict.annotation) throw InvalidError("no annotation was given to this decoder");
		if (!n) return;
		for (uint32_t k = 0; k < n; ++k) if (rec[k] >= d->at.last_n_rec) throw RangeError("record index outside the window");
		HIP_CHECK(hipSetDevice(d->device));
		bam_ready(d);
		HIP_CHECK(hipStreamSynchronize(d->stream));
		PinnedBuf<uint64_t> &P = d->gather.h_patch;
		P.ensure(size_t(n) * 2 + 8);      // words of 8 bytes: rec | gene | mark, 4 bytes each
		size_t at = 0;
		const char *const what = "the patches' staging";
		const uint32_t *const q_rec = pinned_put(P, at, rec, n, what), *const q_gene = pinned_put(P, at, ann_gene, n, what), *const q_mark = pinned_put(P, at, mark, n, what);
		hipLaunchKernelGGL(bam_tag_patch_annotation_kernel, dim3((n + 255) / 256), dim3(256), 0, d->stream, q_rec, q_gene, q_mark, n, d->ann.gene.p, d->ann.mark.p, d->rec.aux.p);
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipStreamSynchronize(d->stream));
	});
}

// -P: the gene the kernels write is the reference's name, which only the caller has
static void tag_check_sources(const dropest_bam_decoder *d) {
	if (d->src.ref_gene && !d->src.has_ref_names) throw InvalidError("under gene = chromosome name the tag kernels need the references' names (dropest_bam_decoder_set_reference_names)");
}

// the last window's records as the tag kernels read them
static BamTagIn tag_in(dropest_bam_decoder *d) {
	const bool ann = d->dict.annotation != nullptr && !d->src.ref_gene;      // (-P comes before -g: the parse asked no annotation)
	return BamTagIn{d->last().data(), d->rec.off.p, d->rec.status.p, d->rec.aux.p, uint32_t(d->at.last_n_rec), ann ? d->ann.gene.p : nullptr, ann ? d->ann.mark.p : nullptr};
}

// each record's output size, the tiles' sums and every record's place; the wait for the one total that sizes the output (in h_tag)
// (filt: -F -- every record's rank among the accepted ones first, the sizes by the decisions; segs: the decisions stand in segments)
// (ts: -r / -P -- the kernels with the sources)
static void tag_plan(dropest_bam_decoder *d, hipStream_t st, const BamTagIn &in, const BamTagNames &names, uint32_t grid, uint32_t tiles, const BamTagFilt *filt, const BamTagSegments *segs,
                     const BamTagSrc *ts) {
	BamTagging &T = d->tag;
	const uint32_t n_rec = in.n_rec;
	HIP_CHECK(hipMemsetAsync(T.flags.p, 0, 4, st));
	HIP_CHECK(hipEventRecord(T.ev[0], st));
	if (filt) {
		hipLaunchKernelGGL(bam_tag_rank_tile_kernel, dim3(tiles), dim3(256), 0, st, in.status, n_rec, T.filt.tile_ok.p);
		hipLaunchKernelGGL(bam_tag_rank_scan_kernel, dim3(1), dim3(1024), 0, st, T.filt.tile_ok.p, tiles, T.filt.total.p);
		hipLaunchKernelGGL(bam_tag_rank_kernel, dim3(tiles), dim3(256), 0, st, in.status, n_rec, T.filt.tile_ok.p, T.filt.rank.p);
		if (ts && segs) hipLaunchKernelGGL((bam_tag_sources_plan_kernel<true, BamTagSegments>), dim3(grid), dim3(BAMTAG_T), 0, st, in, d->cfg, T.cfg, names, *filt, T.size.p, T.flags.p, *segs, *ts);
		else if (ts) hipLaunchKernelGGL((bam_tag_sources_plan_kernel<true, BamTagOneArray>), dim3(grid), dim3(BAMTAG_T), 0, st, in, d->cfg, T.cfg, names, *filt, T.size.p, T.flags.p, BamTagOneArray{}, *ts);
		else if (segs) hipLaunchKernelGGL(bam_tag_filter_plan_kernel<BamTagSegments>, dim3(grid), dim3(BAMTAG_T), 0, st, in, d->cfg, T.cfg, names, *filt, T.size.p, T.flags.p, *segs);
		else hipLaunchKernelGGL(bam_tag_filter_plan_kernel<BamTagOneArray>, dim3(grid), dim3(BAMTAG_T), 0, st, in, d->cfg, T.cfg, names, *filt, T.size.p, T.flags.p, BamTagOneArray{});
	} else if (ts)
		hipLaunchKernelGGL((bam_tag_sources_plan_kernel<false, BamTagOneArray>), dim3(grid), dim3(BAMTAG_T), 0, st, in, d->cfg, T.cfg, names, BamTagFilt{}, T.size.p, T.flags.p, BamTagOneArray{}, *ts);
	else
		hipLaunchKernelGGL(bam_tag_plan_kernel, dim3(grid), dim3(BAMTAG_T), 0, st, in, d->cfg, T.cfg, names, T.size.p, T.flags.p);
	hipLaunchKernelGGL(bam_tag_tile_sum_kernel, dim3(tiles), dim3(256), 0, st, T.size.p, n_rec, T.tile_bytes.p, T.tile_written.p);
	hipLaunchKernelGGL(bam_tag_tile_scan_kernel, dim3(1), dim3(1024), 0, st, T.tile_bytes.p, T.tile_written.p, tiles, T.flags.p, T.h_tag.p);
	hipLaunchKernelGGL(bam_tag_offsets_kernel, dim3(tiles), dim3(256), 0, st, T.size.p, n_rec, T.tile_bytes.p, T.off.p);
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipEventRecord(T.ev[1], st));
	HIP_CHECK(hipStreamSynchronize(st));      // the one total that sizes the output: the only wait of the call
	tag_collect(d);                           // (the window before: its emit is through as well)
	float ms_plan = 0;
	HIP_CHECK(hipEventElapsedTime(&ms_plan, T.ev[0], T.ev[1]));
	T.ms += ms_plan;
}

// What _tag_window and _filter_window share: plan, the one wait, emit.  filt: -F (its rank pointer and decisions are set by the caller); segs:
// the decisions stand in segments (_filter_window_segments: filt's own three arrays are not looked at).
static void tag_run(dropest_bam_decoder *d, const BamTagFilt *filt, const uint8_t **d_out, uint64_t *len, uint64_t *n_written, bool &undecided, const BamTagSegments *segs = nullptr) {
	BamTagging &T = d->tag;
	const uint64_t n_rec = d->at.last_n_rec;
	hipStream_t st = d->stream;
	const uint32_t tiles = uint32_t((n_rec + BAMTAG_SCAN_TILE - 1) / BAMTAG_SCAN_TILE);
	const size_t rc = size_t(n_rec) + size_t(n_rec) / 4;
	T.size.ensure(rc); T.off.ensure(rc); T.tile_bytes.ensure(tiles + tiles / 4 + 1); T.tile_written.ensure(tiles + tiles / 4 + 1); T.flags.ensure(1);
	T.h_tag.ensure(4);
	for (hipEvent_t &e : T.ev) if (!e) HIP_CHECK(hipEventCreate(&e));
	const BamTagIn in = tag_in(d);
	const BamTagNames names{in.a_gene ? T.name_off.p : nullptr, T.name_pool.p, T.n_names};
	const uint32_t grid = uint32_t((n_rec + BAMTAG_WAVES - 1) / BAMTAG_WAVES);
	// -r / -P: the served rows and the table's text, the references' names (the table is not in use by anything else: its calls' own rule)
	const BamSourceState &S = d->src;
	const dropest_read_params *const tb = S.table;
	const BamTagSrc sources{S.bits(), S.rp_row.p, tb ? tb->rows.p : nullptr, tb ? tb->text.p : nullptr, tb ? tb->n_rows : 0u, tb ? tb->text_len : 0ull,
	                        BamTagNames{S.ref_off.p, S.ref_pool.p, S.n_ref_names}};
	const BamTagSrc *const ts = sources.bits ? &sources : nullptr;
	tag_plan(d, st, in, names, grid, tiles, filt, segs, ts);
	const uint64_t total = T.h_tag.p[0], written = T.h_tag.p[1];
	if (ts && (T.h_tag.p[2] & BAMTAG_FLAG_RANGE)) throw RangeError("a record that is written names a read-parameter row, an extent of the table's text or a reference that does not exist (or its decision a cell or a side string)");
	if (T.h_tag.p[2] & BAMTAG_FLAG_RANGE) throw RangeError("the decision of a read that is written names a cell or a side string that does not exist");      // (or no segment covers it: never, the counts were checked)
	if (T.h_tag.p[2] & BAMTAG_FLAG_UNDECIDED) {
		undecided = true;
		throw UnsupportedError("the annotation query left the gene of some reads to the host: give their genes and marks with dropest_bam_decoder_patch_annotation and tag the window again");
	}
	if (!filt && written != d->at.last_n_ok) throw DeviceError("internal: the tagged records and the window's counters disagree");
	T.bytes_in += d->last().data_len;
	if (filt && !total) return;                  // (-F: no read of this window is written)
	T.out.ensure(size_t(total) + size_t(total) / 8 + 64);
	HIP_CHECK(hipEventRecord(T.ev[2], st));      // (the kernels' time: the host's wait and the allocation between them are not theirs)
	const BamTagFilt no_filt{};
	if (ts && segs) hipLaunchKernelGGL((bam_tag_sources_emit_kernel<true, BamTagSegments>), dim3(grid), dim3(BAMTAG_T), 0, st, in, d->cfg, T.cfg, names, *filt, T.size.p, T.off.p, T.out.p, total, T.flags.p, *segs, *ts);
	else if (ts && filt) hipLaunchKernelGGL((bam_tag_sources_emit_kernel<true, BamTagOneArray>), dim3(grid), dim3(BAMTAG_T), 0, st, in, d->cfg, T.cfg, names, *filt, T.size.p, T.off.p, T.out.p, total, T.flags.p, BamTagOneArray{}, *ts);
	else if (ts) hipLaunchKernelGGL((bam_tag_sources_emit_kernel<false, BamTagOneArray>), dim3(grid), dim3(BAMTAG_T), 0, st, in, d->cfg, T.cfg, names, no_filt, T.size.p, T.off.p, T.out.p, total, T.flags.p, BamTagOneArray{}, *ts);
	else if (filt && segs) hipLaunchKernelGGL(bam_tag_filter_emit_kernel<BamTagSegments>, dim3(grid), dim3(BAMTAG_T), 0, st, in, d->cfg, T.cfg, names, *filt, T.size.p, T.off.p, T.out.p, total, T.flags.p, *segs);
	else if (filt) hipLaunchKernelGGL(bam_tag_filter_emit_kernel<BamTagOneArray>, dim3(grid), dim3(BAMTAG_T), 0, st, in, d->cfg, T.cfg, names, *filt, T.size.p, T.off.p, T.out.p, total, T.flags.p, BamTagOneArray{});
	else hipLaunchKernelGGL(bam_tag_emit_kernel, dim3(grid), dim3(BAMTAG_T), 0, st, in, d->cfg, T.cfg, names, T.size.p, T.off.p, T.out.p, total, T.flags.p);
	HIP_CHECK(hipGetLastError());
	bam_copy(st, 1u, to_host(T.flags.p, reinterpret_cast<uint32_t *>(T.h_tag.p + 3)));
	HIP_CHECK(hipEventRecord(T.ev[3], st));
	T.pending = true;                         // its flag (plan and emit disagree: internal) and its time are read after the next wait on the stream
	T.bytes_out += total;
	T.len = total;
	*d_out = T.out.p; *len = total; *n_written = written;
}

extern "C" int dropest_bam_decoder_tag_window(dropest_bam_decoder *d, const uint8_t **d_out, uint64_t *len, uint64_t *n_written) {
	bool undecided = false;
	const int rc = bgzf_guarded([&] {
		if (!d || !d_out || !len || !n_written) throw InvalidError("null argument");
		*d_out = nullptr; *len = 0; *n_written = 0;
		BamTagging &T = d->tag;
		if (!T.on) throw InvalidError("tagging is not configured for this decoder (dropest_bam_decoder_set_tagging)");
		if (d->dict.annotation && !T.has_names) throw InvalidError("with an annotation the tagging configuration must bring its gene names");
		tag_check_sources(d);
		T.len = 0;
		if (!d->at.last_n_rec) return;
		HIP_CHECK(hipSetDevice(d->device));
		bam_ready(d);
		tag_run(d, nullptr, d_out, len, n_written, undecided);
	});
	return rc && undecided ? 2 : rc;
}

// ---- -F ----------------------------------------------------------------------------------------------------------------------------------------
extern "C" int dropest_bam_decoder_set_filtering(dropest_bam_decoder *d, const dropest_bam_filter_cfg *cfg) {
	return bgzf_guarded([&] {
		if (!d) throw InvalidError("null argument");
		BamTagging &T = d->tag;
		BamTagging::Filtering &F = T.filt;
		F.on = false; T.len = 0;
		if (!cfg) return;
		if (!T.on) throw InvalidError("filtering needs the tagging configuration first (dropest_bam_decoder_set_tagging): the other six tags come from there");
		if ((cfg->n_cells && !cfg->cell_barcode) || (cfg->n_side && (!cfg->side_off || !cfg->side_pool))) throw InvalidError("null argument");
		const uint32_t mine[2] = {cfg->out_tag[0], cfg->out_tag[1]};
		bool shared = mine[0] && mine[0] == mine[1];
		for (int k = 0; k < 2; ++k) {
			for (int j = 0; j < 5; ++j) shared |= mine[k] && mine[k] == T.cfg.out_tag[j];
			shared |= mine[k] && mine[k] == T.cfg.type_tag;
		}
		if (shared) throw InvalidError("two output tags share a name: the corrected barcode and UMI tags need names of their own");
		const uint32_t n_side = cfg->n_side, side_bytes = n_side ? cfg->side_off[n_side] : 0u;
		for (uint32_t k = 0; k < n_side; ++k) if (cfg->side_off[k] > cfg->side_off[k + 1]) throw InvalidError("the side strings' offsets must not decrease");
		HIP_CHECK(hipSetDevice(d->device));
		bam_ready(d);
		HIP_CHECK(hipStreamSynchronize(d->stream));
		const size_t code_bytes = cfg->on_device ? 0 : size_t(cfg->n_cells) * 8;
		d->dict.h_dict.ensure(code_bytes + (size_t(n_side) + 1) * 4 + size_t(side_bytes) + 256);
		size_t at = 0;
		F.cell_barcode = cfg->cell_barcode;
		if (!cfg->on_device) {
			F.codes.ensure(size_t(cfg->n_cells) + 1);
			bam_to_device(d, F.codes.p, cfg->cell_barcode, code_bytes, at);
			F.cell_barcode = F.codes.p;
		}
		F.side_off.ensure(size_t(n_side) + 1); F.side_pool.ensure(size_t(side_bytes) + 16);
		if (n_side) bam_to_device(d, F.side_off.p, cfg->side_off, (size_t(n_side) + 1) * 4, at);
		if (side_bytes) bam_to_device(d, F.side_pool.p, cfg->side_pool, side_bytes, at);
		HIP_CHECK(hipStreamSynchronize(d->stream));
		F.out_tag[0] = mine[0]; F.out_tag[1] = mine[1]; F.n_cells = cfg->n_cells; F.n_side = n_side;
		F.on = true;
	});
}

extern "C" int dropest_bam_decoder_filter_window(dropest_bam_decoder *d, const uint8_t *verdict, const uint32_t *cell, const uint64_t *umi, uint64_t n, int on_device,
                                                 const uint8_t **d_out, uint64_t *len, uint64_t *n_written) {
	bool undecided = false;
	const int rc = bgzf_guarded([&] {
		if (!d || !d_out || !len || !n_written || (n && (!verdict || !cell || !umi))) throw InvalidError("null argument");
		*d_out = nullptr; *len = 0; *n_written = 0;
		BamTagging &T = d->tag;
		BamTagging::Filtering &F = T.filt;
		if (!T.on) throw InvalidError("tagging is not configured for this decoder (dropest_bam_decoder_set_tagging)");
		if (!F.on) throw InvalidError("filtering is not configured for this decoder (dropest_bam_decoder_set_filtering)");
		if (d->dict.annotation && !T.has_names) throw InvalidError("with an annotation the tagging configuration must bring its gene names");
		tag_check_sources(d);
		T.len = 0;
		if (n != d->at.last_n_ok) throw InvalidError(std::to_string(n) + " decisions for a window of " + std::to_string(d->at.last_n_ok) + " accepted records");
		const uint64_t n_rec = d->at.last_n_rec;
		if (!n_rec) return;
		HIP_CHECK(hipSetDevice(d->device));
		bam_ready(d);
		const uint32_t tiles = uint32_t((n_rec + BAMTAG_SCAN_TILE - 1) / BAMTAG_SCAN_TILE);
		F.rank.ensure(size_t(n_rec) + size_t(n_rec) / 4); F.tile_ok.ensure(tiles + tiles / 4 + 1); F.total.ensure(1);
		BamTagFilt f{};
		f.rank = F.rank.p; f.verdict = verdict; f.cell = cell; f.umi = umi; f.n = uint32_t(n);
		if (!on_device && n) {      // host arrays: through pinned staging, moved by a kernel's own loads (from_host)
			const size_t m = size_t(n);
			F.umi.ensure(m + m / 4); F.cell.ensure(m + m / 4); F.verdict.ensure(m + m / 4);
			HIP_CHECK(hipStreamSynchronize(d->stream));      // (a call before this one that failed half-way may still be reading the staging)
			F.h_fix.ensure(m + m / 2 + m / 8 + 8);      // words of 8 bytes: UMI | cell | verdict
			size_t at = 0;
			const char *const what = "the decisions' staging";
			const uint64_t *const q_umi = pinned_put(F.h_fix, at, umi, m, what);
			const uint32_t *const q_cell = pinned_put(F.h_fix, at, cell, m, what);
			const uint8_t *const q_verdict = pinned_put(F.h_fix, at, verdict, m, what);
			bam_copy(d->stream, uint32_t(m), from_host(q_umi, F.umi.p), from_host(q_cell, F.cell.p), from_host(q_verdict, F.verdict.p));
			f.verdict = F.verdict.p; f.cell = F.cell.p; f.umi = F.umi.p;      // (tag_run waits for the stream before it returns: the staging is free again)
		}
		f.cell_barcode = F.cell_barcode; f.n_cells = F.n_cells;
		f.side_off = F.side_off.p; f.side_pool = F.side_pool.p; f.n_side = F.n_side;
		f.out_tag[0] = F.out_tag[0]; f.out_tag[1] = F.out_tag[1];
		tag_run(d, &f, d_out, len, n_written, undecided);
	});
	return rc && undecided ? 2 : rc;
}

// The decisions in segments (a sharded run: one segment per shard whose resident range meets the window).  Segments of the decoder's GPU are read
// where they are; those of another GPU are copied into the decoder's staging first (hipMemcpyPeerAsync on the decoder's stream: the arrays are
// finished when the caller has them -- dropest_shard_read_corrections waits for the owning shard's stream before it returns -- so the copy is
// ordered behind that stream by the caller's own wait).  That copy has never run: no machine with two GPUs was there.
// DROPEST_BAM_TEST_STAGE_SEGMENTS=1 (tests) sends every segment through the staging, so that all but the hop between two devices runs on one GPU.
extern "C" int dropest_bam_decoder_filter_window_segments(dropest_bam_decoder *d, const dropest_bam_decision_segment *seg, uint32_t n_seg, const uint8_t **d_out, uint64_t *len,
                                                          uint64_t *n_written) {
	bool undecided = false;
	const int rc = bgzf_guarded([&] {
		if (!d || !d_out || !len || !n_written || (n_seg && !seg)) throw InvalidError("null argument");
		*d_out = nullptr; *len = 0; *n_written = 0;
		BamTagging &T = d->tag;
		BamTagging::Filtering &F = T.filt;
		if (!T.on) throw InvalidError("tagging is not configured for this decoder (dropest_bam_decoder_set_tagging)");
		if (!F.on) throw InvalidError("filtering is not configured for this decoder (dropest_bam_decoder_set_filtering)");
		if (d->dict.annotation && !T.has_names) throw InvalidError("with an annotation the tagging configuration must bring its gene names");
		tag_check_sources(d);
		T.len = 0;
		uint64_t n = 0;
		bool wraps = false;
		for (uint32_t s = 0; s < n_seg; ++s) { wraps |= seg[s].count > ~0ull - n; n += seg[s].count; }
		if (wraps || n != d->at.last_n_ok) throw InvalidError(std::to_string(n) + " decisions for a window of " + std::to_string(d->at.last_n_ok) + " accepted records");
		for (uint32_t s = 0; s < n_seg; ++s) if (seg[s].count && (!seg[s].verdict || !seg[s].cell || !seg[s].umi)) throw InvalidError("null argument");
		const uint64_t n_rec = d->at.last_n_rec;
		if (!n_rec) return;
		HIP_CHECK(hipSetDevice(d->device));
		bam_ready(d);
		const uint32_t tiles = uint32_t((n_rec + BAMTAG_SCAN_TILE - 1) / BAMTAG_SCAN_TILE);
		F.rank.ensure(size_t(n_rec) + size_t(n_rec) / 4); F.tile_ok.ensure(tiles + tiles / 4 + 1); F.total.ensure(1);
		const char *const sw = getenv("DROPEST_BAM_TEST_STAGE_SEGMENTS");
		const bool stage_all = sw && sw[0] == '1';
		bool staged = false;
		for (uint32_t s = 0; s < n_seg; ++s) staged |= seg[s].count && (stage_all || seg[s].device != d->device);
		HIP_CHECK(hipStreamSynchronize(d->stream));      // (a call before this one that failed half-way may still be reading the table's staging)
		if (staged) { const size_t m = size_t(n); F.umi.ensure(m + m / 4); F.cell.ensure(m + m / 4); F.verdict.ensure(m + m / 4); }
		F.h_seg.ensure(size_t(n_seg) + 1); F.seg.ensure(size_t(n_seg) + size_t(n_seg) / 4 + 1);
		uint32_t first = 0;
		for (uint32_t s = 0; s < n_seg; ++s) {
			const dropest_bam_decision_segment &g = seg[s];
			const uint32_t count = uint32_t(g.count);      // (<= the window's records, which a 32-bit rank numbers)
			BamTagSeg e{first, count, g.verdict, g.cell, g.umi};
			if (count && (stage_all || g.device != d->device)) {
				const void *const src[3] = {g.verdict, g.cell, g.umi};
				void *const dst[3] = {F.verdict.p + first, F.cell.p + first, F.umi.p + first};
				const size_t width[3] = {1, 4, 8};
				for (int k = 0; k < 3; ++k) {
					if (g.device != d->device) HIP_CHECK(hipMemcpyPeerAsync(dst[k], d->device, src[k], g.device, size_t(count) * width[k], d->stream));
					else HIP_CHECK(hipMemcpyAsync(dst[k], src[k], size_t(count) * width[k], hipMemcpyDeviceToDevice, d->stream));
				}
				e.verdict = F.verdict.p + first; e.cell = F.cell.p + first; e.umi = F.umi.p + first;
			}
			F.h_seg.p[s] = e;
			first += count;
		}
		bam_copy(d->stream, n_seg, from_host(static_cast<const BamTagSeg *>(F.h_seg.p), F.seg.p));
		BamTagFilt f{};
		f.rank = F.rank.p; f.n = uint32_t(n);
		f.cell_barcode = F.cell_barcode; f.n_cells = F.n_cells;
		f.side_off = F.side_off.p; f.side_pool = F.side_pool.p; f.n_side = F.n_side;
		f.out_tag[0] = F.out_tag[0]; f.out_tag[1] = F.out_tag[1];
		const BamTagSegments segs{F.seg.p, n_seg};
		tag_run(d, &f, d_out, len, n_written, undecided, &segs);      // (waits for the stream before it returns: the table's staging is free again)
	});
	return rc && undecided ? 2 : rc;
}

extern "C" int dropest_bam_decoder_tagged_to_host(dropest_bam_decoder *d, uint8_t *dst, uint64_t cap) {
	return bgzf_guarded([&] {
		if (!d || (d->tag.len && !dst)) throw InvalidError("null argument");
		if (d->tag.len > cap) throw InvalidError("destination too small: " + std::to_string(d->tag.len) + " bytes needed");
		if (!d->tag.len) return;
		HIP_CHECK(hipSetDevice(d->device));
		bam_ready(d);
		HIP_CHECK(hipMemcpyAsync(dst, d->tag.out.p, d->tag.len, hipMemcpyDeviceToHost, d->stream));
		HIP_CHECK(hipStreamSynchronize(d->stream));
		tag_collect(d);
	});
}

extern "C" int dropest_bam_decoder_tag_stats(dropest_bam_decoder *d, double *kernel_ms, uint64_t *bytes_in, uint64_t *bytes_out) {
	if (!d) return 1;
	if (d->tag.pending && bgzf_guarded([&] { HIP_CHECK(hipSetDevice(d->device)); HIP_CHECK(hipStreamSynchronize(d->stream)); tag_collect(d); })) return 1;
	if (kernel_ms) *kernel_ms = d->tag.ms;
	if (bytes_in) *bytes_in = d->tag.bytes_in;
	if (bytes_out) *bytes_out = d->tag.bytes_out;
	return 0;
}
