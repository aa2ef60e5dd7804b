// bgzf_api.hip -- include/dropest_bgzf.h: BGZF block scan on the host, DEFLATE on the device (k_inflate.h).
#include "../../include/dropest_bgzf.h"
#include "../../include/dropest_annotation.h"
#include "k_inflate.h"
#include "k_inflate_par.h"
#include "k_bamparse.h"
#include "k_bamtag.h"
#include "util.h"
#include "host/bgzf_blocks.h"

#include <atomic>
#include <chrono>
#include <future>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

using namespace dropest;
namespace bgzf = Estimation::BamProcessing::bgzf;

namespace {
thread_local std::string g_bgzf_error;
template <class F> int bgzf_guarded(F &&f) {
	try { f(); return 0; }
	catch (const std::exception &e) { g_bgzf_error = e.what(); return 1; }
}
}  // namespace

extern "C" const char *dropest_bgzf_last_error(void) { return g_bgzf_error.c_str(); }

// The parallel inflate's scratch per (device, stream): a block counter and the waves' match lists (~0.5 GB).  Entries of a decoder's streams are
// given back when the decoder lets go of the stream (bgzf_release_inflate_scratch); the null stream's entry stays for the process.
namespace {
struct InflateScratch { DevBuf<InfpMatch> list; DevBuf<uint32_t> next; uint32_t grid = 0; };
std::mutex g_inflate_scratch_mu;
std::map<std::pair<int, void *>, std::unique_ptr<InflateScratch>> g_inflate_scratch;

// freed after the work already queued on `stream` (which may still use the scratch) is done
void bgzf_release_inflate_scratch(int device, void *stream) {
	std::unique_ptr<InflateScratch> gone;
	{
		std::lock_guard<std::mutex> lk(g_inflate_scratch_mu);
		auto it = g_inflate_scratch.find({device, stream});
		if (it == g_inflate_scratch.end()) return;
		gone = std::move(it->second);
		g_inflate_scratch.erase(it);
	}
	(void)hipStreamSynchronize(hipStream_t(stream));
}
}  // namespace

extern "C" int dropest_bgzf_scan(const uint8_t *data, uint64_t len, uint64_t cap, uint64_t *in_off, uint32_t *in_len, uint64_t *out_off,
                                 uint32_t *out_len, uint32_t *crc32, uint64_t *n_blocks, uint64_t *bytes_used, uint64_t *out_total) {
	return bgzf_guarded([&] {
		if (!data || !in_off || !in_len || !out_off || !out_len || !n_blocks) throw InvalidError("null argument");
		uint64_t used = 0, total = 0;
		const std::string error = bgzf::scan_blocks(data, len, cap, in_off, in_len, out_off, out_len, crc32, *n_blocks, used, total);
		if (!error.empty()) throw InvalidError(error);
		if (bytes_used) *bytes_used = used;
		if (out_total) *out_total = total;
	});
}

extern "C" int dropest_bgzf_inflate_device(int device, void *stream, const uint8_t *d_in, uint64_t in_total, const uint64_t *d_in_off,
                                           const uint32_t *d_in_len, const uint64_t *d_out_off, const uint32_t *d_out_len, uint32_t n_blocks,
                                           uint8_t *d_out, uint32_t *d_status, const uint32_t *d_crc32) {
	return bgzf_guarded([&] {
		if (!n_blocks) return;
		if (!d_in || !d_in_off || !d_in_len || !d_out_off || !d_out_len || !d_out || !d_status) throw InvalidError("null argument");
		if (uintptr_t(d_in) & 7u) throw InvalidError("the compressed bytes must be 8-byte aligned");
		HIP_CHECK(hipSetDevice(device));
		// DROPEST_INFLATE_PAR=0: one chain of symbols per block (k_inflate.h: 131 GB/s on a file that deflates 10.8 x, 52 on one that deflates 3.2 x like
		// a real 10x BAM); default: the lanes of a wave on different chunks of the block's symbols (k_inflate_par.h: 123 / 94 GB/s, and a block lasts
		// 0.7 ms instead of 7-11, which is what a window of the BAM path waits for)
		static const int par = [] { const char *e = getenv("DROPEST_INFLATE_PAR"); return e ? atoi(e) : 1; }();
		if (par) {
			// the lanes of a wave on different parts of a block's symbol stream (k_inflate_par.h); the waves take blocks from a counter and keep their
			// match lists in a scratch buffer of the (device, stream) they run on.  The pool's lock is held from the counter's reset to the launch: two
			// calls on one stream then enqueue (memset, kernel) pairs that the stream orders one after the other, never memset A, memset B, kernel A,
			// kernel B (kernel B would find the counter past its blocks and inflate none)
			std::lock_guard<std::mutex> lk(g_inflate_scratch_mu);
			auto &slot = g_inflate_scratch[{device, stream}];
			if (!slot) {
				slot.reset(new InflateScratch());
				hipDeviceProp_t prop{};
				HIP_CHECK(hipGetDeviceProperties(&prop, device));
				slot->grid = uint32_t(prop.multiProcessorCount) * 4u;
				slot->list.alloc(size_t(slot->grid) * INFP_WAVES * INFP_MATCH_CAP);
				slot->next.alloc(1);
			}
			InflateScratch *const sc = slot.get();
			HIP_CHECK(hipMemsetAsync(sc->next.p, 0, 4, hipStream_t(stream)));
			// (DROPEST_INFLATE_PAR_WGS_PER_CU=1..3: fewer workgroups than the CUs hold, so that kernels of other streams find wave slots and LDS beside this one)
			static const uint32_t wgs_per_cu = [] { const char *e = getenv("DROPEST_INFLATE_PAR_WGS_PER_CU"); const int v = e ? atoi(e) : 4; return uint32_t(v < 1 ? 1 : v > 4 ? 4 : v); }();
			const uint32_t grid = std::min<uint32_t>(sc->grid / 4u * wgs_per_cu, (n_blocks + INFP_WAVES - 1) / INFP_WAVES);
			hipLaunchKernelGGL(bgzf_inflate_par_kernel, dim3(grid), dim3(INFP_WAVES * 64), 0, hipStream_t(stream), d_in, in_total, d_in_off, d_in_len, d_out_off, d_out_len,
			                   n_blocks, d_out, d_status, d_crc32, sc->list.p, sc->next.p, uint32_t(getenv("DROPEST_INFLATE_PAR_DBG") ? atoi(getenv("DROPEST_INFLATE_PAR_DBG")) : 0));
			HIP_CHECK(hipGetLastError());
			return;
		}
		hipLaunchKernelGGL(bgzf_inflate_kernel, dim3((n_blocks + INF_WAVES - 1) / INF_WAVES), dim3(INF_WAVES * 64), 0, hipStream_t(stream), d_in, in_total,
		                   d_in_off, d_in_len, d_out_off, d_out_len, n_blocks, d_out, d_status, d_crc32);
		HIP_CHECK(hipGetLastError());
	});
}

#ifdef INFP_PROFILE
// (variant builds of scripts/experiments/inflate_variants only: the kernel's own account of its phases, read and cleared)
extern "C" int dropest_bgzf_inflate_profile(unsigned long long *out24) {
	if (hipMemcpyFromSymbol(out24, HIP_SYMBOL(dropest::infp_prof), 24 * sizeof(unsigned long long)) != hipSuccess) return 1;
	unsigned long long zero[24] = {};
	return hipMemcpyToSymbol(HIP_SYMBOL(dropest::infp_prof), zero, sizeof(zero)) != hipSuccess;
}
#endif

extern "C" int dropest_bgzf_inflate_buffer(int device, const uint8_t *data, uint64_t len, uint8_t *out, uint64_t out_cap, uint64_t *out_len,
                                           uint32_t *status, uint64_t status_cap, uint64_t *n_blocks, double *kernel_ms, int repeats) {
	const bool check_crc = repeats >= 0;     // (repeats < 0: |repeats| runs without the CRC-32 check -- what the check costs)
	if (repeats < 0) repeats = -repeats;
	return bgzf_guarded([&] {
		if (!data || !out_len || !n_blocks) throw InvalidError("null argument");
		int n_dev = 0;
		if (hipGetDeviceCount(&n_dev) != hipSuccess || device >= n_dev) throw DeviceError("no such GPU: BGZF blocks are inflated on the device only here");
		HIP_CHECK(hipSetDevice(device));
		bgzf::BlockTable tab;
		if (!tab.fill(data, len)) throw InvalidError(tab.error);
		const uint64_t n = tab.n, used = tab.used, total = tab.total;
		*n_blocks = n; *out_len = total;
		if (total > out_cap) throw InvalidError("output buffer too small: " + std::to_string(total) + " bytes needed");
		if (!n) return;
		if (n > 0xFFFFFFFFull) throw UnsupportedError("more than 2^32 blocks in one call");
		DevBuf<uint8_t> d_in, d_out;
		DevBuf<uint64_t> d_in_off, d_out_off;
		DevBuf<uint32_t> d_in_len, d_out_len, d_status, d_crc;
		d_in.alloc(used + 8); d_out.alloc(total + 8); d_in_off.alloc(n); d_out_off.alloc(n); d_in_len.alloc(n); d_out_len.alloc(n); d_status.alloc(n); d_crc.alloc(n);
		HIP_CHECK(hipMemcpy(d_crc.p, tab.crc.data(), n * 4, hipMemcpyHostToDevice));
		HIP_CHECK(hipMemcpy(d_in.p, data, used, hipMemcpyHostToDevice));
		HIP_CHECK(hipMemcpy(d_in_off.p, tab.in_off.data(), n * 8, hipMemcpyHostToDevice));
		HIP_CHECK(hipMemcpy(d_out_off.p, tab.out_off.data(), n * 8, hipMemcpyHostToDevice));
		HIP_CHECK(hipMemcpy(d_in_len.p, tab.in_len.data(), n * 4, hipMemcpyHostToDevice));
		HIP_CHECK(hipMemcpy(d_out_len.p, tab.out_len.data(), n * 4, hipMemcpyHostToDevice));
		HIP_CHECK(hipMemset(d_status.p, 0xFF, n * 4));
		HIP_CHECK(hipMemset(d_out.p, 0, total + 8));
		hipEvent_t e0, e1;
		HIP_CHECK(hipEventCreate(&e0)); HIP_CHECK(hipEventCreate(&e1));
		double ms_sum = 0;
		const int reps = repeats > 0 ? repeats : 1;
		for (int r = 0; r < reps; ++r) {
			HIP_CHECK(hipEventRecord(e0, nullptr));
			if (dropest_bgzf_inflate_device(device, nullptr, d_in.p, used, d_in_off.p, d_in_len.p, d_out_off.p, d_out_len.p, uint32_t(n), d_out.p, d_status.p, check_crc ? d_crc.p : nullptr))
				throw DeviceError(g_bgzf_error);
			HIP_CHECK(hipEventRecord(e1, nullptr));
			HIP_CHECK(hipEventSynchronize(e1));
			float ms = 0;
			HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
			ms_sum += ms;
		}
		(void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
		if (kernel_ms) *kernel_ms = ms_sum / reps;
		if (out) HIP_CHECK(hipMemcpy(out, d_out.p, total, hipMemcpyDeviceToHost));
		if (status) HIP_CHECK(hipMemcpy(status, d_status.p, std::min<uint64_t>(n, status_cap) * 4, hipMemcpyDeviceToHost));
	});
}

// ---- BAM records of a window, on the device ------------------------------------------------------------------------------------
// tests: wrong guesses on purpose (every third segment one byte late, every seventh none at all) -- the host's check must find the true chain anyway
__global__ __launch_bounds__(256) void bam_spoil_guesses_kernel(uint64_t *__restrict__ seg_start, uint32_t n_segs) {
	const uint32_t k = blockIdx.x * 256 + threadIdx.x;
	if (k == 0 || k >= n_segs) return;
	if (k % 7u == 3u) seg_start[k] = BAM_NONE;
	else if (k % 3u == 1u && seg_start[k] != BAM_NONE) seg_start[k] += 1;
}

// This translation unit's kernels are loaded onto the device by the first launch of one of them (~10 ms): a context does it when it is created
// (dropest_amd.hip), with the other start-up costs, so that it does not fall into the first window of the first BAM file.
extern "C" void dropest_bgzf_warm_up(void *stream) {
	hipLaunchKernelGGL(bam_spoil_guesses_kernel, dim3(1), dim3(256), 0, hipStream_t(stream), (uint64_t *)nullptr, 0u);      // (no segment: nothing is touched)
	(void)hipGetLastError();
}

// The device BAM decoder (dropest_bam_decoder_*), in this translation unit so that the one launch above loads its kernels as well
#include "bam_read_params.h"        // -r: the read-parameter table, an object of its own beside the decoders
#include "bam_decoder.h"            // the state, the shared helpers, its life cycle, buffer sizing
#include "bam_decoder_dict.h"       // the dictionaries and the annotation
#include "bam_decoder_upload.h"     // staging, pinned pieces, the compressed bytes sent ahead of the window call
#include "bam_decoder_window.h"     // the window calls
#include "bam_decoder_fetch.h"      // the last finished window: fetch / columns / quality / patch
#include "bam_decoder_tag.h"        // -b: the last window's accepted records with their tags edited
