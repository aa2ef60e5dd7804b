// deflate_api.hip -- include/dropest_deflate.h: BGZF blocks written on the device (k_deflate.h).
#include "../../include/dropest_deflate.h"
#include "k_deflate.h"
#include "util.h"

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

using namespace dropest;

namespace {
thread_local std::string g_deflate_error;
template <class F> int deflate_guarded(F &&f) {
	try { f(); return 0; }
	catch (const std::exception &e) { g_deflate_error = e.what(); return 1; }
}
inline uint64_t round_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }
inline uint64_t chunks_of(uint64_t len) { return (len + DFL_CHUNK - 1) / DFL_CHUNK; }

// the scratch of one call, in one allocation: [token lists | staging | member offsets]
struct DeflateLayout {
	uint64_t n_chunks, n_members, tokens_at, staging_at, off_at, bytes;
	DeflateLayout(uint64_t len, int flags) {
		n_chunks = chunks_of(len);
		n_members = n_chunks + ((flags & DROPEST_DEFLATE_EOF) ? 1 : 0);
		tokens_at = 0;
		staging_at = round_up(n_chunks * DFL_CHUNK * 4, 256);
		off_at = staging_at + round_up(n_members * DFL_STRIDE, 256);
		bytes = off_at + round_up(n_members * 8, 256);
	}
};

void deflate_launch(hipStream_t stream, const DeflateLayout &lay, uint8_t *scratch, const uint8_t *d_in, uint64_t len, uint8_t *d_out, uint64_t out_cap,
                    uint32_t *d_member_len, uint64_t *d_totals) {
	uint8_t *staging = scratch + lay.staging_at;
	uint64_t *off = reinterpret_cast<uint64_t *>(scratch + lay.off_at);
	hipLaunchKernelGGL(bgzf_deflate_kernel, dim3(uint32_t(lay.n_members)), dim3(64), 0, stream, d_in, len, uint32_t(lay.n_chunks), staging,
	                   reinterpret_cast<uint32_t *>(scratch + lay.tokens_at), d_member_len);
	HIP_CHECK(hipGetLastError());
	hipLaunchKernelGGL(deflate_scan_kernel, dim3(1), dim3(256), 0, stream, d_member_len, uint32_t(lay.n_members), off, out_cap, d_totals);
	HIP_CHECK(hipGetLastError());
	hipLaunchKernelGGL(deflate_copy_kernel, dim3(uint32_t(lay.n_members)), dim3(256), 0, stream, staging, d_member_len, off, d_out, out_cap);
	HIP_CHECK(hipGetLastError());
}

void deflate_check(const DeflateLayout &lay, const void *d_in, uint64_t len, const void *d_out, const void *d_member_len, uint64_t member_cap, const void *d_totals) {
	if (!d_totals || (lay.n_members && (!d_out || !d_member_len)) || (len && !d_in)) throw InvalidError("null argument");
	if (lay.n_members > member_cap) throw InvalidError("member_cap too small: " + std::to_string(lay.n_members) + " members");
	if (lay.n_members > 0x7FFFFFFFull) throw UnsupportedError("more than 2^31 chunks in one call");
}
}  // namespace

extern "C" const char *dropest_deflate_last_error(void) { return g_deflate_error.c_str(); }

extern "C" uint64_t dropest_bgzf_deflate_bound(uint64_t len) { return len + chunks_of(len) * 31 + DFL_EOF_BYTES; }
extern "C" uint64_t dropest_bgzf_deflate_members(uint64_t len, int flags) { return chunks_of(len) + ((flags & DROPEST_DEFLATE_EOF) ? 1 : 0); }

extern "C" int dropest_bgzf_deflate_device(int device, void *stream, const uint8_t *d_in, uint64_t len, uint8_t *d_out, uint64_t out_cap,
                                           uint32_t *d_member_len, uint64_t member_cap, uint64_t *d_totals, int flags) {
	return deflate_guarded([&] {
		const DeflateLayout lay(len, flags);
		deflate_check(lay, d_in, len, d_out, d_member_len, member_cap, d_totals);
		HIP_CHECK(hipSetDevice(device));
		if (!lay.n_members) { HIP_CHECK(hipMemsetAsync(d_totals, 0, 24, hipStream_t(stream))); return; }
		void *scratch = nullptr;
		HIP_CHECK(hipMallocAsync(&scratch, lay.bytes, hipStream_t(stream)));
		try { deflate_launch(hipStream_t(stream), lay, static_cast<uint8_t *>(scratch), d_in, len, d_out, out_cap, d_member_len, d_totals); }
		catch (...) { (void)hipFreeAsync(scratch, hipStream_t(stream)); throw; }
		HIP_CHECK(hipFreeAsync(scratch, hipStream_t(stream)));
	});
}

extern "C" int dropest_bgzf_deflate_buffer(int device, const uint8_t *data, uint64_t len, uint8_t *out, uint64_t out_cap, uint64_t *out_len,
                                           uint64_t *n_members, double *kernel_ms, int repeats, int flags) {
	return deflate_guarded([&] {
		if (!out_len || !n_members || (len && !data)) throw InvalidError("null argument");
		int n_dev = 0;
		if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) throw DeviceError("no such GPU: BGZF blocks are deflated on the device only here");
		HIP_CHECK(hipSetDevice(device));
		const DeflateLayout lay(len, flags);
		*out_len = 0; *n_members = lay.n_members;
		if (kernel_ms) *kernel_ms = 0;
		if (!lay.n_members) return;
		if (!out && out_cap) throw InvalidError("null argument");
		constexpr uint64_t GUARD = 256;                                   // behind the capacity: must come back as it went
		const uint64_t cap = std::min<uint64_t>(out_cap, dropest_bgzf_deflate_bound(len));
		DevBuf<uint8_t> d_in, d_out, scratch;
		DevBuf<uint32_t> d_member_len;
		DevBuf<uint64_t> d_totals;
		d_in.alloc(len); d_out.alloc(cap + GUARD); scratch.alloc(lay.bytes); d_member_len.alloc(lay.n_members); d_totals.alloc(3);
		if (len) HIP_CHECK(hipMemcpy(d_in.p, data, len, hipMemcpyHostToDevice));
		HIP_CHECK(hipMemset(d_out.p, 0xA5, cap + GUARD));
		hipEvent_t e0, e1;
		HIP_CHECK(hipEventCreate(&e0)); HIP_CHECK(hipEventCreate(&e1));
		double ms_sum = 0;
		const int reps = repeats > 0 ? repeats : 1;
		for (int r = 0; r < reps; ++r) {
			HIP_CHECK(hipEventRecord(e0, nullptr));
			deflate_launch(nullptr, lay, scratch.p, d_in.p, len, d_out.p, cap, d_member_len.p, d_totals.p);
			HIP_CHECK(hipEventRecord(e1, nullptr));
			HIP_CHECK(hipEventSynchronize(e1));
			float ms = 0;
			HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
			ms_sum += ms;
		}
		(void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
		if (kernel_ms) *kernel_ms = ms_sum / reps;
		uint64_t totals[3] = {};
		uint8_t guard[GUARD];
		HIP_CHECK(hipMemcpy(totals, d_totals.p, sizeof(totals), hipMemcpyDeviceToHost));
		HIP_CHECK(hipMemcpy(guard, d_out.p + cap, GUARD, hipMemcpyDeviceToHost));
		for (uint64_t k = 0; k < GUARD; ++k) if (guard[k] != 0xA5) throw DeviceError("the device wrote beyond the output capacity");
		*out_len = totals[1];
		if (totals[2] || totals[1] > cap) throw InvalidError("output buffer too small: " + std::to_string(totals[1]) + " bytes needed");
		HIP_CHECK(hipMemcpy(out, d_out.p, totals[1], hipMemcpyDeviceToHost));
	});
}

// ---- batches through buffers that stay ---------------------------------------------------------------------------------------------
struct dropest_deflate_batch {
	int device = 0;
	uint64_t max_bytes = 0, out_cap = 0;
	hipStream_t stream = nullptr;
	PinnedBuf<uint8_t> h_in, h_out;
	PinnedBuf<uint64_t> h_totals;
	DevBuf<uint8_t> d_in, d_out, scratch;
	DevBuf<uint32_t> d_member_len;
	DevBuf<uint64_t> d_totals;
	~dropest_deflate_batch() { if (stream) { (void)hipSetDevice(device); (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); } }
};

extern "C" int dropest_deflate_batch_create(int device, uint64_t max_bytes, dropest_deflate_batch **out) {
	return deflate_guarded([&] {
		if (!out || !max_bytes) throw InvalidError("null argument");
		*out = nullptr;
		int n_dev = 0;
		if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) throw DeviceError("no such GPU: BGZF blocks are deflated on the device only here");
		HIP_CHECK(hipSetDevice(device));
		std::unique_ptr<dropest_deflate_batch> b(new dropest_deflate_batch());
		const DeflateLayout lay(max_bytes, 0);
		b->device = device; b->max_bytes = max_bytes; b->out_cap = dropest_bgzf_deflate_bound(max_bytes);
		HIP_CHECK(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
		b->h_in.ensure_exact(max_bytes, hipHostMallocDefault); b->h_out.ensure_exact(b->out_cap, hipHostMallocDefault); b->h_totals.ensure_exact(3, hipHostMallocDefault);
		b->d_in.alloc(max_bytes); b->d_out.alloc(b->out_cap); b->scratch.alloc(lay.bytes); b->d_member_len.alloc(lay.n_members); b->d_totals.alloc(3);
		*out = b.release();
	});
}

extern "C" int dropest_deflate_batch_input(dropest_deflate_batch *b, uint8_t **pinned) {
	return deflate_guarded([&] { if (!b || !pinned) throw InvalidError("null argument"); *pinned = b->h_in.p; });
}

extern "C" int dropest_deflate_batch_run(dropest_deflate_batch *b, uint64_t len, const uint8_t **out, uint64_t *out_len, uint64_t *n_members) {
	return deflate_guarded([&] {
		if (!b || !out || !out_len) throw InvalidError("null argument");
		if (len > b->max_bytes) throw InvalidError("a batch of " + std::to_string(len) + " bytes in a handle made for " + std::to_string(b->max_bytes));
		*out = b->h_out.p; *out_len = 0;
		if (n_members) *n_members = 0;
		if (!len) return;
		HIP_CHECK(hipSetDevice(b->device));
		const DeflateLayout lay(len, 0);
		HIP_CHECK(hipMemcpyAsync(b->d_in.p, b->h_in.p, len, hipMemcpyHostToDevice, b->stream));
		deflate_launch(b->stream, lay, b->scratch.p, b->d_in.p, len, b->d_out.p, b->out_cap, b->d_member_len.p, b->d_totals.p);
		HIP_CHECK(hipMemcpyAsync(b->h_totals.p, b->d_totals.p, 24, hipMemcpyDeviceToHost, b->stream));
		HIP_CHECK(hipStreamSynchronize(b->stream));
		const uint64_t total = b->h_totals.p[1];
		if (b->h_totals.p[2] || total > b->out_cap || b->h_totals.p[0] != lay.n_members) throw DeviceError("the deflate kernels reported an impossible size");
		HIP_CHECK(hipMemcpyAsync(b->h_out.p, b->d_out.p, total, hipMemcpyDeviceToHost, b->stream));
		HIP_CHECK(hipStreamSynchronize(b->stream));
		*out_len = total;
		if (n_members) *n_members = lay.n_members;
	});
}

extern "C" void dropest_deflate_batch_destroy(dropest_deflate_batch *b) { delete b; }

// ---- a stream of bytes that are on the device already (the tagged BAM output, -b) ---------------------------------------------------------
struct dropest_deflate_stream {
	int device = 0;
	hipStream_t stream = nullptr;
	uint64_t batch = 0, fill = 0, out_cap = 0;
	dropest_deflate_write write = nullptr;
	void *user = nullptr;
	DevBuf<uint8_t> d_in, d_out, scratch;
	DevBuf<uint32_t> d_member_len;
	DevBuf<uint64_t> d_totals;
	PinnedBuf<uint8_t> h_out;
	PinnedBuf<uint64_t> h_totals;
	hipEvent_t ev[2] = {nullptr, nullptr};
	double kernel_ms = 0;
	uint64_t bytes_in = 0, bytes_out = 0, n_batches = 0;
	~dropest_deflate_stream() { (void)hipSetDevice(device); (void)hipStreamSynchronize(stream); for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

namespace {
// the first `len` bytes collected so far: one launch, the members to pinned memory, then to the caller
void deflate_stream_flush(dropest_deflate_stream *s, uint64_t len, int flags) {
	const DeflateLayout lay(len, flags);
	if (!lay.n_members) return;
	// The launches of dropest_bgzf_deflate_device with a scratch buffer that is the handle's own, as dropest_deflate_batch has one.  With that
	// call's scratch from the stream-ordered pool, blocks came out damaged (sizes right, payload bits wrong, other blocks each run) whenever the
	// BAM decoder inflated its next window on another stream meanwhile (DROPEST_BAM_PIPELINE=1; measured: 9-22 of 161 blocks, none with this
	// buffer, none with a device-wide wait in front of the launch).
	deflate_check(lay, s->d_in.p, len, s->d_out.p, s->d_member_len.p, s->d_member_len.n, s->d_totals.p);
	s->scratch.ensure(lay.bytes);
	HIP_CHECK(hipEventRecord(s->ev[0], s->stream));
	deflate_launch(s->stream, lay, s->scratch.p, s->d_in.p, len, s->d_out.p, s->out_cap, s->d_member_len.p, s->d_totals.p);
	HIP_CHECK(hipEventRecord(s->ev[1], s->stream));
	HIP_CHECK(hipMemcpyAsync(s->h_totals.p, s->d_totals.p, 24, hipMemcpyDeviceToHost, s->stream));
	HIP_CHECK(hipStreamSynchronize(s->stream));
	const uint64_t total = s->h_totals.p[1];
	if (s->h_totals.p[2] || total > s->out_cap || s->h_totals.p[0] != lay.n_members) throw DeviceError("the deflate kernels reported an impossible size");
	float ms = 0;
	HIP_CHECK(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
	s->kernel_ms += ms; s->bytes_in += len; s->bytes_out += total; ++s->n_batches;
	s->h_out.ensure(total);
	HIP_CHECK(hipMemcpyAsync(s->h_out.p, s->d_out.p, total, hipMemcpyDeviceToHost, s->stream));
	HIP_CHECK(hipStreamSynchronize(s->stream));
	if (s->write(s->h_out.p, total, s->user)) throw IoError("the compressed bytes could not be written");
}
}  // namespace

extern "C" int dropest_deflate_stream_create(int device, void *stream, uint64_t batch_bytes, dropest_deflate_write write, void *user, dropest_deflate_stream **out) {
	return deflate_guarded([&] {
		if (!out || !write) throw InvalidError("null argument");
		*out = nullptr;
		int n_dev = 0;
		if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) throw DeviceError("no such GPU: BGZF blocks are deflated on the device only here");
		HIP_CHECK(hipSetDevice(device));
		std::unique_ptr<dropest_deflate_stream> s(new dropest_deflate_stream());
		// whole chunks, so that every block but a file's last is full; at most 64 MB, so that a launch's scratch (about 5 x its input) stays bounded
		const uint64_t chunks = std::max<uint64_t>(1, std::min<uint64_t>(batch_bytes ? batch_bytes : ~0ull, uint64_t(64) << 20) / DFL_CHUNK);
		s->device = device; s->stream = hipStream_t(stream); s->batch = chunks * DFL_CHUNK; s->write = write; s->user = user;
		s->out_cap = dropest_bgzf_deflate_bound(s->batch);
		s->d_in.alloc(s->batch); s->d_out.alloc(s->out_cap); s->d_member_len.alloc(chunks + 1); s->d_totals.alloc(3);
		s->h_totals.ensure_exact(3, hipHostMallocDefault);
		for (hipEvent_t &e : s->ev) HIP_CHECK(hipEventCreate(&e));
		*out = s.release();
	});
}

extern "C" int dropest_deflate_stream_put(dropest_deflate_stream *s, const uint8_t *src, uint64_t len, int on_device) {
	return deflate_guarded([&] {
		if (!s || (len && !src)) throw InvalidError("null argument");
		HIP_CHECK(hipSetDevice(s->device));
		while (len) {
			const uint64_t take = std::min(len, s->batch - s->fill);
			HIP_CHECK(hipMemcpyAsync(s->d_in.p + s->fill, src, take, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->stream));
			if (!on_device) HIP_CHECK(hipStreamSynchronize(s->stream));      // (the caller's host bytes are its own again)
			s->fill += take; src += take; len -= take;
			if (s->fill == s->batch) { s->fill = 0; deflate_stream_flush(s, s->batch, 0); }
		}
	});
}

extern "C" int dropest_deflate_stream_finish(dropest_deflate_stream *s, int flags) {
	return deflate_guarded([&] {
		if (!s) throw InvalidError("null argument");
		HIP_CHECK(hipSetDevice(s->device));
		const uint64_t rest = s->fill;
		s->fill = 0;
		if (rest) deflate_stream_flush(s, rest, flags);
		else if (flags & DROPEST_DEFLATE_EOF) {      // nothing is left over: the end-of-file block alone (SAMv1 section 4.1.2)
			static const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
			HIP_CHECK(hipStreamSynchronize(s->stream));
			if (s->write(eof, sizeof(eof), s->user)) throw IoError("the compressed bytes could not be written");
			s->bytes_out += sizeof(eof);
		}
	});
}

extern "C" int dropest_deflate_stream_stats(const dropest_deflate_stream *s, double *kernel_ms, uint64_t *bytes_in, uint64_t *bytes_out, uint64_t *n_batches) {
	if (!s) return 1;
	if (kernel_ms) *kernel_ms = s->kernel_ms;
	if (bytes_in) *bytes_in = s->bytes_in;
	if (bytes_out) *bytes_out = s->bytes_out;
	if (n_batches) *n_batches = s->n_batches;
	return 0;
}

extern "C" void dropest_deflate_stream_destroy(dropest_deflate_stream *s) { delete s; }
