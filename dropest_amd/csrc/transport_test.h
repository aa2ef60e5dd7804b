// transport_test.h -- test hooks of the shard transports (transport.h; included by shard_run.h): the HostMailbox between processes on the
// CPU (tests/test_host_mailbox.py), and the all-to-all(v) and the device gather of a Transport driven directly with small patterned arrays
// instead of through a whole sharded pass (tests/test_gpu_transport.py).
#pragma once

#include <thread>

namespace dropest {

// Every rank of the group calls this once.  cnt[src][dst] comes from {0, 1, 5, 257} by (3 * src + dst + shift) % 4, with source row 1
// and destination column 2 forced to 0 from three ranks on: zeros, a whole zero row and column, a 1, a size beyond 256.  shift 0 leaves
// every rank's own block empty ((4 * r) % 4 = 0), so the same checks run once more with shift 3, where it holds 257 elements.
// Returns 0 or the number of the first check that failed; the collectives that follow a failed check are still made (the peers wait in them).
inline int transport_selftest(Transport &t, hipStream_t st, uint32_t in_place) {
	const int W = t.world, R = t.rank;
	const size_t elem[3] = {8, 4, 1};
	constexpr uint64_t GAP = 3;
	constexpr unsigned char SENTINEL = 0xFF;
	// element i of array a in the block from s to d: never all-ones, and the low byte alone still tells s, d, a and i apart
	auto pattern = [](int s, int d, int a, uint64_t i, size_t bytes) { const uint64_t x = ((uint64_t(s) * 64 + uint64_t(d)) * 4 + uint64_t(a)) * 1024 + i; return bytes == 1 ? x % 251 + 1 : x; };
	int bad = 0, check = 0;
	for (int shift : {0, 3}) {
		auto cnt = [&](int s, int d) -> uint64_t { static const uint64_t v[4] = {0, 1, 5, 257}; return W >= 3 && (s == 1 || d == 2) ? 0 : v[(3 * s + d + shift) % 4]; };
		std::vector<uint64_t> sc(static_cast<size_t>(W)), rc(static_cast<size_t>(W)), so[2], ro[2];
		uint64_t ns = 0, nr = 0;
		for (int p = 0; p < W; ++p) {   // offsets [0]: the prefix sums exchange() derives; [1]: every piece shifted by a gap that must stay sentinel
			sc[size_t(p)] = cnt(R, p); rc[size_t(p)] = cnt(p, R);
			so[0].push_back(ns); ro[0].push_back(nr); so[1].push_back(ns + GAP * uint64_t(p + 1)); ro[1].push_back(nr + GAP * uint64_t(p + 1));
			ns += sc[size_t(p)]; nr += rc[size_t(p)];
		}
		const uint64_t cap_s = ns + GAP * uint64_t(W + 1), cap_r = nr + GAP * uint64_t(W + 1);
		for (int at = 0; at < 2; ++at) {
			DevBuf<unsigned char> d_s[3], d_r[3];
			std::vector<unsigned char> h_s[3], h_r[3];
			const void *snd[3]; void *rcv[3];
			for (int a = 0; a < 3; ++a) {
				h_s[a].assign(size_t(cap_s) * elem[a], SENTINEL); h_r[a].assign(size_t(cap_r) * elem[a], SENTINEL);
				for (int p = 0; p < W; ++p)
					for (uint64_t i = 0; i < sc[size_t(p)]; ++i) { const uint64_t x = pattern(R, p, a, i, elem[a]); std::memcpy(&h_s[a][size_t(so[at][size_t(p)] + i) * elem[a]], &x, elem[a]); }
				d_s[a].alloc(h_s[a].size()); d_r[a].alloc(h_r[a].size());
				HIP_CHECK(hipMemcpyAsync(d_s[a].p, h_s[a].data(), h_s[a].size(), hipMemcpyHostToDevice, st));
				HIP_CHECK(hipMemcpyAsync(d_r[a].p, h_r[a].data(), h_r[a].size(), hipMemcpyHostToDevice, st));
				snd[a] = d_s[a].p; rcv[a] = d_r[a].p;
			}
			if (at) t.exchange_at(3, snd, rcv, elem, so[1].data(), sc.data(), ro[1].data(), rc.data(), st, in_place);
			else t.exchange(3, snd, rcv, elem, sc.data(), rc.data(), st, in_place);
			for (int a = 0; a < 3; ++a) HIP_CHECK(hipMemcpyAsync(h_r[a].data(), d_r[a].p, h_r[a].size(), hipMemcpyDeviceToHost, st));
			HIP_CHECK(stream_wait(st));
			for (int a = 0; a < 3; ++a) {
				++check;
				std::vector<unsigned char> want(h_r[a].size(), SENTINEL);   // the kept block of an in-place array is not copied: sentinel as well
				for (int p = 0; p < W; ++p)
					for (uint64_t i = 0; i < (p == R && (in_place >> a & 1u) ? 0 : rc[size_t(p)]); ++i) { const uint64_t x = pattern(p, R, a, i, elem[a]); std::memcpy(&want[size_t(ro[at][size_t(p)] + i) * elem[a]], &x, elem[a]); }
				if (!bad && want != h_r[a]) bad = check;
			}
		}
	}
	// gather_dev: blocks of unequal sizes, rank 1's empty, a gap in front of every block
	std::vector<size_t> off(static_cast<size_t>(W)), bytes(static_cast<size_t>(W));
	size_t total = 0;
	for (int p = 0; p < W; ++p) { bytes[size_t(p)] = p == 1 ? 0 : size_t(8 * (p + 3)); off[size_t(p)] = total + 8; total = off[size_t(p)] + bytes[size_t(p)]; }
	std::vector<unsigned char> mine(std::max<size_t>(bytes[size_t(R)], 1)), all(total + 8, SENTINEL), want(total + 8, SENTINEL);
	for (int p = 0; p < W; ++p) for (size_t i = 0; i < bytes[size_t(p)]; ++i) want[off[size_t(p)] + i] = (unsigned char)(p * 37 + i * 11);
	for (size_t i = 0; i < bytes[size_t(R)]; ++i) mine[i] = (unsigned char)(R * 37 + i * 11);
	DevBuf<unsigned char> d_mine, d_all;
	d_mine.alloc(mine.size()); d_all.alloc(all.size());
	HIP_CHECK(hipMemcpyAsync(d_mine.p, mine.data(), mine.size(), hipMemcpyHostToDevice, st));
	HIP_CHECK(hipMemcpyAsync(d_all.p, all.data(), all.size(), hipMemcpyHostToDevice, st));
	t.gather_dev(d_mine.p, d_all.p, off.data(), bytes.data(), st);
	HIP_CHECK(hipMemcpyAsync(all.data(), d_all.p, all.size(), hipMemcpyDeviceToHost, st));
	HIP_CHECK(stream_wait(st));
	++check;
	if (!bad && all != want) bad = check;
	return bad;
}

}  // namespace dropest

extern "C" {

// HostMailbox (tests/test_host_mailbox.py: processes on the CPU): `rounds` gathers of `bytes` patterned bytes per rank, every one checked;
// returns 0, or the round (1-based) in which a slot did not hold what its rank wrote
int dropest_test_host_mailbox(uint64_t token, int32_t rank, int32_t world, uint32_t rounds, uint64_t bytes) {
	try {
		dropest::HostMailbox mb(token, rank, world);
		std::vector<unsigned char> mine(bytes), all(size_t(bytes) * size_t(world));
		for (uint32_t r = 0; r < rounds; ++r) {
			const size_t n = r % 3 == 2 ? size_t(bytes) / 2 : size_t(bytes);          // sizes change between rounds (the same on every rank)
			for (size_t i = 0; i < n; ++i) mine[i] = (unsigned char)(rank * 131 + r * 7 + i * 13);
			mb.gather(mine.data(), n, all.data());
			for (int p = 0; p < world; ++p)
				for (size_t i = 0; i < n; ++i) if (all[size_t(p) * n + i] != (unsigned char)(p * 131 + r * 7 + i * 13)) return int(r + 1);
		}
		mb.barrier();
		return 0;
	} catch (const std::exception &e) { g_last_error = e.what(); return -1; }
}

// plane 0: a LocalHub and `world` threads on `device` (rank and id are not used); plane 1: this process is rank `rank` of `world` over an
// RcclTransport (its data plane follows DROPEST_SHARD_DATAPLANE as in a real run).  0, the number of the first failed check (1-6: exchange
// then exchange_at, arrays of 8 / 4 / 1 bytes; 7-12: the same with the own block filled; 13: gather_dev), or -1 with dropest_last_error set.
int dropest_test_transport(int plane, int32_t rank, int32_t world, const uint8_t id[128], int device, uint32_t in_place) {
	using namespace dropest;
	struct Stream { hipStream_t s = nullptr; Stream() { HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); } ~Stream() { (void)hipStreamDestroy(s); } };
	try {
		if (world < 1 || world > 64 || (plane == 1 && (!id || rank < 0 || rank >= world))) throw InvalidError("rank / world out of range, or no id");
		if (plane == 1) {
			HIP_CHECK(hipSetDevice(device));
			Stream st;
			RcclTransport t(rank, world, id, st.s);
			return transport_selftest(t, st.s, in_place);
		}
		auto hub = std::make_shared<LocalHub>(world);
		std::vector<int> rc(static_cast<size_t>(world), 0);
		std::vector<std::string> err(static_cast<size_t>(world));
		std::vector<std::thread> threads;
		for (int r = 0; r < world; ++r)
			threads.emplace_back([&, r] {
				try {
					HIP_CHECK(hipSetDevice(device));
					Stream st;
					LocalTransport t(hub, r);
					rc[size_t(r)] = transport_selftest(t, st.s, in_place);
				} catch (const std::exception &e) { hub->fail(); err[size_t(r)] = e.what(); rc[size_t(r)] = -1; }
			});
		for (std::thread &th : threads) th.join();
		for (int r = 0; r < world; ++r) if (rc[size_t(r)] < 0) throw DeviceError(err[size_t(r)]);
		for (int r = 0; r < world; ++r) if (rc[size_t(r)]) return rc[size_t(r)];
		return 0;
	} catch (const std::exception &e) { g_last_error = e.what(); return -1; }
}

}  // extern "C"
