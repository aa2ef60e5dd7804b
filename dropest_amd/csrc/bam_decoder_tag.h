// bam_decoder_tag.h -- -b: the accepted records of the LAST finished window with their tags edited (k_bamtag.h; the state: BamTagging, bam_decoder.h)
#pragma once

extern "C" int dropest_bam_decoder_set_tagging(dropest_bam_decoder *d, const dropest_bam_tag_cfg *cfg) {
	return bgzf_guarded([&] {
		if (!d) throw InvalidError("null argument");
		BamTagging &T = d->tag;
		T.on = false; T.has_names = false; T.len = 0;
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

// the last window's records as the tag kernels read them
static BamTagIn tag_in(dropest_bam_decoder *d) {
	const bool ann = d->dict.annotation != nullptr;
	return BamTagIn{d->last().data(), d->rec.off.p, d->rec.status.p, d->rec.aux.p, uint32_t(d->at.last_n_rec), ann ? d->ann.gene.p : nullptr, ann ? d->ann.mark.p : nullptr};
}

// each record's output size, the tiles' sums and every record's place; the wait for the one total that sizes the output (in h_tag)
static void tag_plan(dropest_bam_decoder *d, hipStream_t st, const BamTagIn &in, const BamTagNames &names, uint32_t grid, uint32_t tiles) {
	BamTagging &T = d->tag;
	const uint32_t n_rec = in.n_rec;
	HIP_CHECK(hipMemsetAsync(T.flags.p, 0, 4, st));
	HIP_CHECK(hipEventRecord(T.ev[0], st));
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

extern "C" int dropest_bam_decoder_tag_window(dropest_bam_decoder *d, const uint8_t **d_out, uint64_t *len, uint64_t *n_written) {
	bool undecided = false;
	const int rc = bgzf_guarded([&] {
		if (!d || !d_out || !len || !n_written) throw InvalidError("null argument");
		*d_out = nullptr; *len = 0; *n_written = 0;
		BamTagging &T = d->tag;
		if (!T.on) throw InvalidError("tagging is not configured for this decoder (dropest_bam_decoder_set_tagging)");
		if (d->dict.annotation && !T.has_names) throw InvalidError("with an annotation the tagging configuration must bring its gene names");
		T.len = 0;
		const uint64_t n_rec = d->at.last_n_rec;
		if (!n_rec) return;
		HIP_CHECK(hipSetDevice(d->device));
		bam_ready(d);
		hipStream_t st = d->stream;
		const uint32_t tiles = uint32_t((n_rec + BAMTAG_SCAN_TILE - 1) / BAMTAG_SCAN_TILE);
		const size_t rc = size_t(n_rec) + size_t(n_rec) / 4;
		T.size.ensure(rc); T.off.ensure(rc); T.tile_bytes.ensure(tiles + tiles / 4 + 1); T.tile_written.ensure(tiles + tiles / 4 + 1); T.flags.ensure(1);
		T.h_tag.ensure(4);
		for (hipEvent_t &e : T.ev) if (!e) HIP_CHECK(hipEventCreate(&e));
		const BamTagIn in = tag_in(d);
		const BamTagNames names{d->dict.annotation ? T.name_off.p : nullptr, T.name_pool.p, T.n_names};
		const uint32_t grid = uint32_t((n_rec + BAMTAG_WAVES - 1) / BAMTAG_WAVES);
		tag_plan(d, st, in, names, grid, tiles);
		const uint64_t total = T.h_tag.p[0], written = T.h_tag.p[1];
		if (T.h_tag.p[2] & BAMTAG_FLAG_UNDECIDED) {
			undecided = true;
			throw UnsupportedError("the annotation query left the gene of some reads to the host: give their genes and marks with dropest_bam_decoder_patch_annotation and tag the window again");
		}
		if (written != d->at.last_n_ok) throw DeviceError("internal: the tagged records and the window's counters disagree");
		T.out.ensure(size_t(total) + size_t(total) / 8 + 64);
		HIP_CHECK(hipEventRecord(T.ev[2], st));      // (the kernels' time: the host's wait and the allocation between them are not theirs)
		hipLaunchKernelGGL(bam_tag_emit_kernel, dim3(grid), dim3(BAMTAG_T), 0, st, in, d->cfg, T.cfg, names, T.size.p, T.off.p, T.out.p, total, T.flags.p);
		HIP_CHECK(hipGetLastError());
		bam_copy(st, 1u, to_host(T.flags.p, reinterpret_cast<uint32_t *>(T.h_tag.p + 3)));
		HIP_CHECK(hipEventRecord(T.ev[3], st));
		T.pending = true;                         // its flag (plan and emit disagree: internal) and its time are read after the next wait on the stream
		T.bytes_in += d->last().data_len; T.bytes_out += total;
		T.len = total;
		*d_out = T.out.p; *len = total; *n_written = written;
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
