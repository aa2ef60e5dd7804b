// bam_decoder_upload.h -- the compressed bytes of a window on their way to the device ahead of the window call: the staging buffers, the pinned
// pieces and the upload calls (the state: BamUpload, bam_decoder.h).  These are the calls a reader thread makes beside the window calls.
#pragma once

extern "C" int dropest_bam_decoder_staging(dropest_bam_decoder *d, int which, uint64_t bytes, uint8_t **out) {
	return bgzf_guarded([&] {
		if (!d || !out || which < 0 || which > 1) throw InvalidError("bad argument");
		HIP_CHECK(hipSetDevice(d->device));
		const bool trace = getenv("DROPEST_BAM_TRACE") != nullptr;
		BamLap t;
		auto lap = [&](const char *what) { if (trace) std::fprintf(stderr, "[bam] staging %d: %s %.1f ms\n", which, what, t.next()); };
		d->up.h_stage[which].ensure(bytes);
		lap("pinned buffer");
		*out = d->up.h_stage[which].p;
		bam_reserve(d, which, bytes);
		lap("device buffers");
	});
}

// The same without the pinned buffer: for a caller that sends the compressed bytes in pieces (below)
extern "C" int dropest_bam_decoder_reserve(dropest_bam_decoder *d, int which, uint64_t bytes, uint64_t inflated_bytes) {
	return bgzf_guarded([&] {
		if (!d || which < 0 || which > 1) throw InvalidError("bad argument");
		HIP_CHECK(hipSetDevice(d->device));
		bam_reserve(d, which, bytes, inflated_bytes);
	});
}

// n pinned pieces of `bytes` each (kept by the decoder; a second call with other sizes replaces them): out[k] = piece k
extern "C" int dropest_bam_decoder_pieces(dropest_bam_decoder *d, uint32_t n, uint64_t bytes, uint8_t **out) {
	return bgzf_guarded([&] {
		if (!d || !out || !n || n > 64 || !bytes) throw InvalidError("bad argument");
		HIP_CHECK(hipSetDevice(d->device));
		BamUpload &U = d->up;
		if (U.n_pieces) HIP_CHECK(hipStreamSynchronize(U.stream));      // (copies out of the pieces there are)
		if (U.n_pieces != n) {
			for (hipEvent_t e : U.piece_done) if (e) (void)hipEventDestroy(e);
			U.piece_done.clear();
			U.n_pieces = 0;
			U.piece_done.assign(n, nullptr);
			for (hipEvent_t &e : U.piece_done) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
		}
		const uint64_t each = (bytes + 4095u) & ~uint64_t(4095);
		// (DROPEST_BAM_PINNED_COHERENT=1: the default kind of pinned memory, fine-grained, instead of memory the CPU caches)
		static const bool coherent = getenv("DROPEST_BAM_PINNED_COHERENT") != nullptr;
		U.piece_mem.ensure_exact(each * n, coherent ? hipHostMallocDefault : hipHostMallocNonCoherent);
		U.n_pieces = n; U.piece_bytes = each;
		for (uint32_t k = 0; k < n; ++k) out[k] = U.piece_mem.p + each * k;
	});
}

// Piece `piece` is free again: the copy that read it last has finished (at once when there was none)
extern "C" int dropest_bam_decoder_piece_wait(dropest_bam_decoder *d, uint32_t piece) {
	if (!d || piece >= d->up.n_pieces) return 1;
	if (hipSetDevice(d->device) != hipSuccess) return 1;
	return hipEventSynchronize(d->up.piece_done[piece]) == hipSuccess ? 0 : 1;
}

// A window's pieces are about to be sent to up-buffer `which` (one thread; the .._upload_piece calls that follow may come from several)
extern "C" int dropest_bam_decoder_upload_begin(dropest_bam_decoder *d, int which) {
	if (!d || which < 0 || which > 1 || !d->up.n_pieces) return 1;
	d->up.ready[which].store(false, std::memory_order_relaxed);
	d->up.begun[which] = true;
	return 0;
}

// The first `len` bytes of piece `piece` to up-buffer `which` at byte `dst_off`, on the upload stream; does not wait.  May be called from several
// threads (different pieces).  .._upload_done(which, host bytes, total length) then says what the buffer holds.
extern "C" int dropest_bam_decoder_upload_piece(dropest_bam_decoder *d, int which, uint32_t piece, uint64_t dst_off, uint64_t len) {
	if (!d || which < 0 || which > 1 || piece >= d->up.n_pieces || len > d->up.piece_bytes || dst_off + len + 8 > d->up.in[which].n) return 1;
	if (!len) return 0;
	if (hipSetDevice(d->device) != hipSuccess) return 1;
	BamUpload &U = d->up;
	if (!U.begun[which]) return 1;      // (.._upload_begin was not called)
	if (hipMemcpyAsync(U.in[which].p + dst_off, U.piece_mem.p + U.piece_bytes * piece, len, hipMemcpyHostToDevice, U.stream) != hipSuccess) return 1;
	return hipEventRecord(U.piece_done[piece], U.stream) == hipSuccess ? 0 : 1;
}

// Up-buffer `which` holds (will hold, once done[which] has passed) host[0 .. len): their block table -- the caller's, made while it read the file
// (`host` is then not touched at all unless a block is refused), else from the bytes, while the copy runs; a failure here is the window call's
// to report -- and the word to the window call that is then given exactly these bytes.
static void publish_upload(dropest_bam_decoder *d, int which, const uint8_t *host, uint64_t len, const dropest_bgzf_blocks *blocks = nullptr) {
	bgzf::BlockTable &b = d->up.blocks[which];
	try {
		if (blocks) b.fill(blocks->n, blocks->in_off, blocks->in_len, blocks->out_len, blocks->crc32, host, len);
		else b.fill(host, len);
	} catch (...) { b.ok = false; }
	d->up.len[which] = len;
	d->up.host[which].store(host, std::memory_order_relaxed);
	d->up.ready[which].store(true, std::memory_order_release);
}

// Every piece of a window has been given to .._upload_piece: up-buffer `which` holds (will hold, when those copies are through) host[0 .. len).
// The block table is made from `host` (which must stay readable until the window call that is given `host` and `len` has returned -- the host
// fall-back for a refused block reads it).
extern "C" int dropest_bam_decoder_upload_done(dropest_bam_decoder *d, int which, const uint8_t *host, uint64_t len, const dropest_bgzf_blocks *blocks) {
	if (!d || which < 0 || which > 1) return 1;
	d->up.ready[which].store(false, std::memory_order_relaxed);
	if (!len || !host || len + 8 > d->up.in[which].n) return 0;
	if (hipSetDevice(d->device) != hipSuccess) return 1;
	if (!d->up.begun[which] || hipEventRecord(d->up.done[which], d->up.stream) != hipSuccess) return 1;
	d->up.begun[which] = false;
	publish_upload(d, which, host, len, blocks);
	return 0;
}

// The first `len` bytes of staging buffer `which` start their way to the device now, on a stream of their own: the window call that is then given
// exactly that buffer and length waits for this copy instead of making one -- with a reader thread that calls this when its read is done, the
// copy of window k + 1 runs under the kernels of window k.  Allocates nothing; the one call of the decoder that may run beside a window call
// (from another thread).  A length the buffers were not sized for is not an error: the window call copies as before.
extern "C" int dropest_bam_decoder_upload(dropest_bam_decoder *d, int which, uint64_t len) {
	if (!d || which < 0 || which > 1) return 1;
	d->up.ready[which].store(false, std::memory_order_relaxed);
	const PinnedBuf<uint8_t> &stage = d->up.h_stage[which];
	if (!len || !stage.p || len > stage.n || len + 8 > d->up.in[which].n) return 0;
	if (hipSetDevice(d->device) != hipSuccess) return 1;
	if (hipMemcpyAsync(d->up.in[which].p, stage.p, len, hipMemcpyHostToDevice, d->up.stream) != hipSuccess) return 1;
	if (hipEventRecord(d->up.done[which], d->up.stream) != hipSuccess) return 1;
	publish_upload(d, which, stage.p, len);
	return 0;
}
