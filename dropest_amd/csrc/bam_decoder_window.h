// bam_decoder_window.h -- a window of a BAM file through the decoder: inflate, the chain of records, the fields and dense columns (the three
// window calls and their two compositions).  What the caller may ask of the last finished window: bam_decoder_fetch.h.
#pragma once

// ---- first half, part A: inflate -------------------------------------------------------------------------------------------------------------
// the up-buffer that holds exactly comp[0 .. len) (dropest_bam_decoder_upload / _upload_done sent them ahead), taken; -1: none
static int take_upload(dropest_bam_decoder *dec, const uint8_t *comp, uint64_t len) {
	int up = -1;
	for (int w = 0; w < 2; ++w)
		// (the buffer first: only the slot these bytes stand in is looked at -- the reader thread may be filling the other one right now)
		if (comp && comp == dec->up.host[w].load(std::memory_order_relaxed) && dec->up.ready[w].load(std::memory_order_acquire) && len == dec->up.len[w]) { up = w; dec->up.ready[w].store(false, std::memory_order_relaxed); }
	return up;
}

// the front's block table to the device through pinned memory, in one launch
static void block_table_to_device(BamFront &F, hipStream_t st) {
	const bgzf::BlockTable &T = F.tab;
	const size_t n = T.n;
	size_t at = 0;
	const char *const what = "the block table's staging";
	const uint64_t *const t_in = pinned_put(F.h_tab, at, T.in_off.data(), n, what), *const t_out = pinned_put(F.h_tab, at, T.out_off.data(), n, what);
	const uint32_t *const t_ilen = pinned_put(F.h_tab, at, T.in_len.data(), n, what), *const t_olen = pinned_put(F.h_tab, at, T.out_len.data(), n, what), *const t_crc = pinned_put(F.h_tab, at, T.crc.data(), n, what);
	bam_copy(st, uint32_t(n), from_host(t_in, F.d_in_off.p), from_host(t_out, F.d_out_off.p), from_host(t_ilen, F.d_in_len.p), from_host(t_olen, F.d_out_len.p), from_host(t_crc, F.d_crc.p));
}

// First half of a window, part A: the block table, the tables and (unless dropest_bam_decoder_upload sent them ahead) the compressed bytes to the
// device, the inflate kernel enqueued -- and back, without waiting for any of it.  The blocks land at a fixed distance from the start of the
// front's buffer, so this may be called for window k + 1 while window k is still in its chain / fields / host work: the device then always has
// the next window's blocks to fill the wave slots that window k's finished blocks leave (a window's inflate takes as long as its slowest
// block, ~7-11 ms on a file that deflates 3 x, however few blocks are left running).  comp must stay as it is until .._window_chain returns.
constexpr uint64_t BAM_TAIL_RESERVE = uint64_t(1) << 20;
extern "C" int dropest_bam_decoder_window_inflate(dropest_bam_decoder *dec, const uint8_t *comp, uint64_t len, int *slot) {
	return bgzf_guarded([&] {
		if (!dec || !slot || (len && !comp)) throw InvalidError("null argument");
		BamFront &F = dec->front[dec->at.next_front];
		if (F.inflating) throw InvalidError("this front still holds a window whose blocks are being inflated (call .._window_chain first)");
		F.begun = false;
		*slot = dec->at.next_front;
		dec->at.next_front ^= 1;
		HIP_CHECK(hipSetDevice(dec->device));
		bam_ready(dec);
		// the first half of a window on a stream of its own, for a caller that runs it beside the second half of the window before; the two
		// halves one after the other (dropest_bam_decoder_window) share the decoder's stream
		// (Beside window k's chain / fields kernels the inflate of window k + 1 holds every wave slot of the device for 7-11 ms: whatever else is
		// launched meanwhile waits for slots.  Measured on the 3.2 x file: the chain 1.3 -> 52 ms, the dictionaries' copies 1.2 -> 31 ms; with a CU
		// mask on this stream that leaves 32 CUs alone the chain is back at 2 ms but the fields kernels run on those 32 CUs, 28 -> 49 ms, and a
		// masked stream is a blocking one: every null-stream copy waits for the inflate.  NOTES_r06 section 3.)
		if (!dec->halves_in_sequence && !F.stream) HIP_CHECK(hipStreamCreateWithFlags(&F.stream, hipStreamNonBlocking));
		hipStream_t st = dec->halves_in_sequence ? dec->stream : F.stream;
		const int up = take_upload(dec, comp, len);      // >= 0: the bytes went ahead
		if (up >= 0 && dec->up.blocks[up].ok) { F.tab.swap(dec->up.blocks[up]); dec->up.blocks[up].ok = false; }
		else if (!F.tab.fill(comp, len)) throw InvalidError(F.tab.error);
		const uint64_t n = F.tab.n, total = F.tab.total;
		if (F.tab.used != len) throw InvalidError("a window must hold whole BGZF blocks");
		if (n > 0xFFFFFFFFull) throw UnsupportedError("more than 2^32 blocks in one window");
		if (total >= (uint64_t(1) << 40)) throw UnsupportedError("window too large");
		static const uint64_t reserve_min = [] { const char *e = getenv("DROPEST_BAM_TEST_TAIL_RESERVE"); return e ? uint64_t(std::max(0ll, atoll(e))) : BAM_TAIL_RESERVE; }();
		F.reserve = (std::max(reserve_min, dec->at.tail_len) + 255u) & ~uint64_t(255);   // (the last cut-off record seen is a hint; a longer one moves the data: .._window_chain)
		BamLap t;
		F.d_out.ensure(F.reserve + total + total / 4 + 64);
		F.ms_copy = F.ms_inflate = F.ms_boundaries = 0;
		if (n) {
			const uint8_t *uploaded = nullptr;
			if (up >= 0) { uploaded = dec->up.in[up].p; HIP_CHECK(hipStreamWaitEvent(st, dec->up.done[up], 0)); }
			else F.d_in.ensure(len + len / 4 + 8);
			F.size_blocks(n, n / 4);
			if (!uploaded) HIP_CHECK(hipMemcpyAsync(F.d_in.p, comp, len, hipMemcpyHostToDevice, st));
			block_table_to_device(F, st);
			F.ms_copy = t.ms();
			// (every verdict "not inflated" until the kernel says otherwise: a block it never reaches goes to the host fall-back, not through with stale bytes)
			HIP_CHECK(hipMemsetAsync(F.d_status.p, 0xFF, size_t(n) * 4, st));
			if (dropest_bgzf_inflate_device(dec->device, st, uploaded ? uploaded : F.d_in.p, len, F.d_in_off.p, F.d_in_len.p, F.d_out_off.p, F.d_out_len.p, uint32_t(n), F.d_out.p + F.reserve, F.d_status.p, F.d_crc.p))
				throw DeviceError(g_bgzf_error);
			bam_copy(st, uint32_t(n), to_host(F.d_status.p, F.h_block_status.p));      // (the blocks' verdicts)
		}
		F.n_blocks = uint32_t(n); F.total = total; F.comp = comp; F.comp_len = len;
		F.inflating = true;
	});
}

// ---- first half, part B: the chain -----------------------------------------------------------------------------------------------------------
// the blocks the device refused, inflated by the caller's function; returns how many
static uint32_t host_inflate_refused(BamFront &F, hipStream_t st, dropest_bgzf_host_inflate inflate_fallback, void *user) {
	const bgzf::BlockTable &T = F.tab;
	uint32_t refused = 0;
	std::vector<uint8_t> tmp;
	for (uint64_t k = 0; k < F.n_blocks; ++k) {
		if (!F.h_block_status.p[k]) continue;
		++refused;
		if (!inflate_fallback) throw InvalidError("the device refused BGZF block " + std::to_string(k) + " of the window (status " + std::to_string(F.h_block_status.p[k]) + ") and no host inflate was given");
		tmp.resize(T.out_len[k] + 1);
		if (inflate_fallback(F.comp + T.in_off[k], T.in_len[k], tmp.data(), T.out_len[k], user)) throw InvalidError("damaged BGZF block (neither the device nor the host inflates it)");
		HIP_CHECK(hipMemcpyAsync(F.d_out.p + F.reserve + T.out_off[k], tmp.data(), T.out_len[k], hipMemcpyHostToDevice, st));
		HIP_CHECK(hipStreamSynchronize(st));
	}
	return refused;
}

// the cut-off record of the window before, in front of the blocks
static void place_carried_record(dropest_bam_decoder *dec, BamFront &F, hipStream_t st) {
	const uint64_t tail = dec->at.tail_len, data_len = tail + F.total;
	if (tail > F.reserve) {      // longer than the room left for it: the window moves behind it in a buffer of its own (a record beyond 1 MB: rare)
		DevBuf<uint8_t> moved;
		moved.alloc(data_len + data_len / 4 + 64);
		if (F.total) HIP_CHECK(hipMemcpyAsync(moved.p + tail, F.d_out.p + F.reserve, F.total, hipMemcpyDeviceToDevice, st));
		HIP_CHECK(hipStreamSynchronize(st));
		F.d_out = std::move(moved);
		F.reserve = tail;
	}
	F.base_off = F.reserve - tail;
	if (tail) HIP_CHECK(hipMemcpyAsync(F.data(), dec->d_tail.p, tail, hipMemcpyDeviceToDevice, st));
}

// The chain of records through the window's n_segs segments, the first at `expect`: guesses per segment, walks, the host's check (a guess that
// is not on the chain is put right and its segment walked again).  Returns where the first record begins that the window does not hold whole;
// F.h_base / F.n_rec / F.repaired: the records in front of each segment, all of them, the guesses put right.
static uint64_t find_chain(dropest_bam_decoder *dec, BamFront &F, hipStream_t st, uint64_t data_len, uint32_t n_segs, uint64_t expect) {
	uint8_t *const data = F.data();
	uint64_t n_rec = 0;
	F.n_rec = 0; F.repaired = 0;
	if (!n_segs) return expect;
	F.size_segments(n_segs, n_segs / 4);
	HIP_CHECK(hipMemsetAsync(F.d_bad.p, 0, 8, st));
	HIP_CHECK(hipMemcpyAsync(F.seg_start.p, &expect, 8, hipMemcpyHostToDevice, st));
	if (n_segs > 1) hipLaunchKernelGGL(bam_seg_guess_kernel, dim3((n_segs - 1 + 3) / 4), dim3(256), 0, st, data, data_len, dec->cfg.n_refs, n_segs, F.seg_start.p);
	if (getenv("DROPEST_BAM_TEST_SPOIL_GUESSES")) hipLaunchKernelGGL(bam_spoil_guesses_kernel, dim3((n_segs + 255) / 256), dim3(256), 0, st, F.seg_start.p, n_segs);
	hipLaunchKernelGGL(bam_seg_walk_kernel, dim3((n_segs + 255) / 256), dim3(256), 0, st, data, data_len, (const uint32_t *)nullptr, n_segs, F.seg_start.p,
	                   F.seg_count.p, F.seg_exit.p, (const uint32_t *)nullptr, (uint64_t *)nullptr, F.d_bad.p + 1);
	// (a walk from a guess that is not on the chain reads anything as a length: what these walks flag is not looked at -- the walk that
	// writes the record offsets, from the checked starts, is the one whose flag counts: dropest_bam_decoder_window_finish)
	bam_copy(st, n_segs, to_host(F.seg_start.p, F.h_seg_start.p), to_host(F.seg_exit.p, F.h_seg_exit.p), to_host(F.seg_count.p, F.h_count.p));
	HIP_CHECK(hipStreamSynchronize(st));
	for (uint32_t k = 0; k < n_segs; ++k) {
		const uint64_t seg_end = uint64_t(k + 1) * BAM_SEG;
		const uint64_t want = expect < seg_end ? expect : BAM_NONE;      // no record starts in this segment: the chain is already past it
		if (F.h_seg_start.p[k] != want) {                                  // the guess was not on the chain: walk again from the true place
			if (k) ++F.repaired;
			F.h_seg_start.p[k] = want;
			HIP_CHECK(hipMemcpyAsync(F.seg_start.p + k, &F.h_seg_start.p[k], 8, hipMemcpyHostToDevice, st));
			HIP_CHECK(hipMemcpyAsync(F.d_list.p, &k, 4, hipMemcpyHostToDevice, st));
			hipLaunchKernelGGL(bam_seg_walk_kernel, dim3(1), dim3(256), 0, st, data, data_len, F.d_list.p, 1u, F.seg_start.p, F.seg_count.p, F.seg_exit.p,
			                   (const uint32_t *)nullptr, (uint64_t *)nullptr, F.d_bad.p + 1);
			HIP_CHECK(hipMemcpyAsync(F.h_seg_exit.p + k, F.seg_exit.p + k, 8, hipMemcpyDeviceToHost, st));
			HIP_CHECK(hipMemcpyAsync(F.h_count.p + k, F.seg_count.p + k, 4, hipMemcpyDeviceToHost, st));
			HIP_CHECK(hipStreamSynchronize(st));
		}
		F.h_base.p[k] = uint32_t(n_rec);
		n_rec += F.h_count.p[k];
		if (want != BAM_NONE) expect = F.h_seg_exit.p[k];
	}
	if (n_rec > 0xFFFFFFF0ull) throw UnsupportedError("more than 2^32 records in one window");
	F.n_rec = n_rec;
	return expect;
}

// the record the window cuts off opens the next window
static void keep_tail(dropest_bam_decoder *dec, BamFront &F, hipStream_t st, uint64_t new_tail) {
	if (new_tail) {
		dec->d_tail.ensure(new_tail + new_tail / 4 + 64);
		HIP_CHECK(hipMemcpyAsync(dec->d_tail.p, F.data() + F.tail_start, new_tail, hipMemcpyDeviceToDevice, st));
		HIP_CHECK(hipStreamSynchronize(st));
	}
	dec->at.tail_len = new_tail;
}

// First half of a window, part B: waits for the inflate of `slot`, has refused blocks inflated on the host, puts the record the window before cut
// off in front of the data, and finds the chain of records (guesses per segment, walks, the host's check).  Windows take this call in file order.
extern "C" int dropest_bam_decoder_window_chain(dropest_bam_decoder *dec, int slot, uint32_t first_skip, int final, dropest_bgzf_host_inflate inflate_fallback, void *user) {
	return bgzf_guarded([&] {
		if (!dec || slot < 0 || slot > 1) throw InvalidError("bad argument");
		BamFront &F = dec->front[slot];
		if (!F.inflating) throw InvalidError("this window's inflate was not started (or failed)");
		F.inflating = false;
		HIP_CHECK(hipSetDevice(dec->device));
		bam_ready(dec);
		// (the blocks were inflated on the front's stream, which may leave CUs alone -- see _inflate; everything from here on runs on the
		// decoder's own stream, which may use them all: it must not queue behind the next window's inflate)
		hipStream_t st_inflate = dec->halves_in_sequence ? dec->stream : F.stream;
		hipStream_t st = dec->stream;
		const uint64_t tail = dec->at.tail_len, data_len = tail + F.total;
		if (tail && first_skip) throw InvalidError("first_skip belongs to the first window");
		if (data_len >= (uint64_t(1) << 40)) throw UnsupportedError("window too large");
		BamLap t;
		HIP_CHECK(hipStreamSynchronize(st_inflate));      // the blocks are inflated (and their verdicts on the host)
		const uint32_t refused = host_inflate_refused(F, st, inflate_fallback, user);
		F.ms_inflate = t.ms();
		place_carried_record(dec, F, st);
		t = BamLap();
		const uint32_t n_segs = uint32_t((data_len + BAM_SEG - 1) / BAM_SEG);
		const uint64_t tail_start = find_chain(dec, F, st, data_len, n_segs, tail ? 0 : first_skip);
		if (tail_start > data_len) throw InvalidError("Corrupt BAM record");
		if (final && tail_start != data_len) throw InvalidError("Truncated BAM file");
		F.ms_boundaries = t.ms();
		F.data_len = data_len; F.tail_start = tail_start; F.n_segs = n_segs; F.refused = refused;
		keep_tail(dec, F, st, data_len - tail_start);
		F.begun = true;
	});
}

// The two parts one after the other (the first half of a window as rounds before 6 had it)
extern "C" int dropest_bam_decoder_window_begin(dropest_bam_decoder *dec, const uint8_t *comp, uint64_t len, uint32_t first_skip, int final,
                                                dropest_bgzf_host_inflate inflate_fallback, void *user, int *slot) {
	if (dropest_bam_decoder_window_inflate(dec, comp, len, slot)) return 1;
	const int rc = dropest_bam_decoder_window_chain(dec, *slot, first_skip, final, inflate_fallback, user);
	if (rc && dec) dec->front[*slot].inflating = false;
	return rc;
}

// ---- second half: fields and dense columns ---------------------------------------------------------------------------------------------------
// what dropest_bam_decoder_window_finish says at its steps (DROPEST_BAM_TRACE_READER=1: of the first window, 2: of every one)
struct BamFinishTrace {
	dropest_bam_decoder *d;
	uint64_t n_rec;
	BamLap t;
	void operator()(const char *what) const {
		static const int trace_laps = getenv("DROPEST_BAM_TRACE_READER") ? atoi(getenv("DROPEST_BAM_TRACE_READER")) : 0;
		if (trace_laps >= 2 || (trace_laps && !d->traced_first)) std::fprintf(stderr, "[bam] a window's fields (%llu records): %s at %.2f ms\n", (unsigned long long)n_rec, what, t.ms());
	}
};

// record offsets, the fields, the accepted records made dense; the counters, totals and flag on their way to h_result
static void queue_fields(dropest_bam_decoder *d, BamFront &F, hipStream_t st, const BamFinishTrace &lap) {
	const uint64_t n_rec = F.n_rec;
	const uint32_t tiles = uint32_t((n_rec + BAM_FIN_TILE - 1) / BAM_FIN_TILE);
	const size_t rc = size_t(n_rec) + size_t(n_rec) / 4;
	d->rec.off.ensure(rc);      // (ahead of the others: the walk that fills it runs while they grow)
	lap("rec_off ensured");
	bam_copy(st, F.n_segs, from_host(F.h_base.p, F.seg_base.p));
	lap("segment bases copy queued");
	hipLaunchKernelGGL(bam_seg_walk_kernel, dim3((F.n_segs + 255) / 256), dim3(256), 0, st, F.data(), F.data_len, (const uint32_t *)nullptr, F.n_segs, F.seg_start.p,
	                   F.seg_count.p, F.seg_exit.p, F.seg_base.p, d->rec.off.p, F.d_bad.p);
	lap("record offsets walked (queued)");
	d->size_records(rc, tiles + tiles / 4 + 1);
	HIP_CHECK(hipMemsetAsync(d->rec.d_wc.p, 0, sizeof(BamWindowCounts), st));
	lap("buffers ensured");
	const BamRecordOut ro = d->record_out();
	const BamDict dict = d->dict.args();
	const int sources = d->src.bits();
	dropest_annotation *const annotation = (sources & BAM_SRC_REF_GENE) ? nullptr : d->dict.annotation;      // (-P comes before -g)
	if (annotation) HIP_CHECK(hipMemsetAsync(d->ann.chr.p, 0xFF, size_t(n_rec) * 4, st));   // (records that are not accepted: "no such chromosome", ignored)
	const dim3 parse_grid(uint32_t((n_rec + BAM_PARSE_T - 1) / BAM_PARSE_T));
	if (!sources) hipLaunchKernelGGL(bam_parse_kernel, parse_grid, dim3(BAM_PARSE_T), 0, st, F.data(), d->rec.off.p, uint32_t(n_rec), d->cfg, dict, ro, F.d_bad.p);
	else {
		// -r: the claims of this window's records carry ordinals behind those of every window before (the parses run in file order on one stream)
		const BamSources bs{d->src.table ? d->src.table->view() : RpTable{}, d->src.first_ordinal + d->src.seen, d->src.rp_row.p, d->src.gene_of_ref.p};
		auto parse = [&](auto kernel) { hipLaunchKernelGGL(kernel, parse_grid, dim3(BAM_PARSE_T), 0, st, F.data(), d->rec.off.p, uint32_t(n_rec), d->cfg, dict, ro, F.d_bad.p, bs); };
		if (sources == BAM_SRC_PARAMS) parse(bam_parse_sources_kernel<BAM_SRC_PARAMS>);
		else if (sources == BAM_SRC_REF_GENE) parse(bam_parse_sources_kernel<BAM_SRC_REF_GENE>);
		else parse(bam_parse_sources_kernel<BAM_SRC_PARAMS | BAM_SRC_REF_GENE>);
		if (sources & BAM_SRC_PARAMS) hipLaunchKernelGGL(bam_params_settle_kernel, dim3(uint32_t((n_rec + 255) / 256)), dim3(256), 0, st, uint32_t(n_rec), bs, ro, annotation ? 1 : 0);
		d->src.seen += n_rec;
	}
	if (annotation) {
		if (dropest_annotation_query_device(annotation, st, n_rec, d->ann.chr.p, d->ann.pos.p, d->ann.end.p, d->ann.gene.p, d->ann.mark.p)) throw DeviceError(dropest_annotation_last_error());
		hipLaunchKernelGGL(bam_resolve_annotated_kernel, dim3(uint32_t((n_rec + 255) / 256)), dim3(256), 0, st, uint32_t(n_rec), dict, ro, d->ann.gene.p, d->ann.mark.p);
	}
	BamRecords &R = d->rec;
	hipLaunchKernelGGL(bam_fin_count_kernel, dim3(tiles), dim3(256), 0, st, R.status.p, R.need.p, R.uql.p, uint32_t(n_rec), R.tile_ok.p, R.tile_need.p, R.d_wc.p);
	hipLaunchKernelGGL(bam_fin_scan_kernel, dim3(1), dim3(1024), 0, st, R.tile_ok.p, R.tile_need.p, tiles, R.d_totals.p);
	hipLaunchKernelGGL(bam_fin_scatter_kernel, dim3(tiles), dim3(256), 0, st, F.data(), R.off.p, ro, uint32_t(n_rec), R.tile_ok.p, R.tile_need.p, d->dense.args());
	HIP_CHECK(hipGetLastError());
	// (into pinned words: a copy to pageable memory is staged and waits for the stream each time -- three of them per window)
	HIP_CHECK(hipMemcpyAsync(R.h_result.p, R.d_wc.p, sizeof(BamWindowCounts), hipMemcpyDeviceToHost, st));
	HIP_CHECK(hipMemcpyAsync(R.h_result.p + 10, R.d_totals.p, 8, hipMemcpyDeviceToHost, st));
	HIP_CHECK(hipMemcpyAsync(R.h_result.p + 12, F.d_bad.p, 4, hipMemcpyDeviceToHost, st));
}

// h_result after the wait, into the caller's window: the counters, what was accepted, the dense columns
static void read_results(dropest_bam_decoder *d, const BamFront &F, dropest_bam_window *out) {
	static_assert(sizeof(BamWindowCounts) == 40, "ten words");
	BamWindowCounts wc{};
	uint32_t totals[2] = {0, 0}, bad_record = 0;
	const uint32_t *const r = d->rec.h_result.p;
	if (F.n_rec) { std::memcpy(&wc, r, sizeof(wc)); totals[0] = r[10]; totals[1] = r[11]; bad_record = r[12]; }
	if (bad_record) throw InvalidError("Corrupt BAM record");      // (a block_size below the 32 bytes of a record's fixed part, met by the walk from the checked starts; fixed part + name + cigar + bases longer than the record, met by the parse)
	out->n_records = F.n_rec; out->tail_bytes = F.data_len - F.tail_start;
	for (int k = 0; k < 5; ++k) out->counts[k] = wc.status[k];
	out->n_accepted = totals[0]; out->n_need = totals[1];
	out->d_cb = reinterpret_cast<const uint64_t *>(d->dense.cb.p); out->d_umi = reinterpret_cast<const uint64_t *>(d->dense.umi.p); out->d_gene = d->dense.gene.p; out->d_aux = d->dense.aux.p;
	out->quality_seen = wc.quality; out->any_gene = wc.any_gene;
	out->quality_len_max = wc.any_gene ? wc.ql_max : 0u; out->quality_len_min = wc.any_gene ? 0xFFFFFFFFu - wc.ql_min_inv : 0u;
}

// the records the host must see, to its pinned arrays
static void need_lists_to_host(dropest_bam_decoder *d, hipStream_t st, dropest_bam_window *out, const BamFinishTrace &lap) {
	BamDenseColumns &C = d->dense;
	const uint32_t n_need = out->n_need;
	if (n_need) {
		C.h_need_rec.ensure(n_need); C.h_need_pos.ensure(n_need); C.h_need_size.ensure(n_need);
		lap("need arrays pinned");
		bam_copy(st, n_need, to_host(C.need_rec.p, C.h_need_rec.p), to_host(C.need_pos.p, C.h_need_pos.p), to_host(C.need_size.p, C.h_need_size.p));
		HIP_CHECK(hipStreamSynchronize(st));
	}
	lap("need arrays copied");
	out->need_rec = C.h_need_rec.p; out->need_pos = C.h_need_pos.p; out->need_size = C.h_need_size.p;
}

extern "C" int dropest_bam_decoder_window_finish(dropest_bam_decoder *d, int slot, dropest_bam_window *out) {
	return bgzf_guarded([&] {
		if (!d || !out || slot < 0 || slot > 1) throw InvalidError("bad argument");
		BamFront &F = d->front[slot];
		if (!F.begun) throw InvalidError("this window was not begun (or its first half failed)");
		F.begun = false;
		HIP_CHECK(hipSetDevice(d->device));
		bam_ready(d);
		hipStream_t st = d->stream;
		*out = dropest_bam_window{};
		d->at.last_n_rec = 0; d->at.last_n_ok = 0; d->at.last_front = slot;
		out->n_blocks = F.n_blocks; out->window_bytes = F.data_len; out->refused_blocks = F.refused; out->guesses_repaired = F.repaired;
		out->ms_copy = F.ms_copy; out->ms_inflate = F.ms_inflate; out->ms_boundaries = F.ms_boundaries;
		const BamFinishTrace lap{d, F.n_rec, BamLap()};
		d->rec.h_result.ensure(16);
		lap("result words pinned");
		if (F.n_rec) queue_fields(d, F, st, lap);
		lap("kernels and copies queued");
		HIP_CHECK(hipStreamSynchronize(st));
		lap("kernels done");
		read_results(d, F, out);
		need_lists_to_host(d, st, out, lap);
		d->traced_first = true;
		out->ms_parse = lap.t.ms();
		d->at.last_n_rec = F.n_rec; d->at.last_n_ok = out->n_accepted;
		if (out->n_accepted != out->counts[0]) throw DeviceError("internal: the dense columns and the counters disagree");
	});
}

extern "C" int dropest_bam_decoder_window(dropest_bam_decoder *d, const uint8_t *comp, uint64_t len, uint32_t first_skip, int final,
                                          dropest_bgzf_host_inflate inflate_fallback, void *user, dropest_bam_window *out) {
	int slot = 0;
	if (d) d->halves_in_sequence = true;
	const int rc = dropest_bam_decoder_window_begin(d, comp, len, first_skip, final, inflate_fallback, user, &slot);
	if (d) d->halves_in_sequence = false;
	if (rc) return 1;
	return dropest_bam_decoder_window_finish(d, slot, out);
}
