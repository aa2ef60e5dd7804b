// transport.h -- how the shards of a sharded run (shard_run.h) reach each other: the RCCL loader, the Transport interface and its planes.
//   LocalTransport  shards inside one process (one host thread each, several shards per device allowed): device-to-device copies and a
//                   host barrier over a LocalHub
//   RcclTransport   one process per GPU: grouped ncclSend / ncclRecv over xGMI for the device data, the HostMailbox (POSIX shared memory)
//                   for the small host tables; DROPEST_SHARD_DATAPLANE=shm stands in for RCCL between processes that share a GPU
// Every plane has ONE all-to-all(v), exchange_at; Transport::exchange is that with prefix-sum offsets.
#pragma once

#include <rccl/rccl.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <sched.h>
#include <sys/stat.h>
#include <dlfcn.h>
#include <fcntl.h>
#include <mutex>
#include <sys/mman.h>
#include <unistd.h>

namespace dropest {

// ---- RCCL, bound at run time (the library also works on hosts without it: single-GPU use never touches it) -----------
struct RcclApi {
	void *handle = nullptr;
	ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
	ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
	ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
	ncclResult_t (*GroupStart)() = nullptr;
	ncclResult_t (*GroupEnd)() = nullptr;
	ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
	ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
	ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
	const char *(*GetErrorString)(ncclResult_t) = nullptr;
	static RcclApi &get() {
		static RcclApi api = [] {
			RcclApi a;
			// The RCCL that belongs to the HIP runtime this library runs on: a process may hold two ROCm trees (PyTorch ships its
			// own next to /opt/rocm), and an RCCL from the other tree opens ITS libhsa-runtime64 -- not initialised -- and fails
			// with "no ROCm-capable device".  So: the directory libamdhip64 was loaded from first, then the default search.
			Dl_info hip{};
			if (dladdr(reinterpret_cast<void *>(&hipGetDeviceCount), &hip) && hip.dli_fname) {
				std::string dir(hip.dli_fname);
				const size_t slash = dir.rfind('/');
				if (slash != std::string::npos) {
					dir.resize(slash + 1);
					for (const char *name : {"librccl.so.1", "librccl.so"}) if ((a.handle = dlopen((dir + name).c_str(), RTLD_NOW | RTLD_GLOBAL))) break;
				}
			}
			if (!a.handle) for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) if ((a.handle = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
			if (!a.handle) return a;
			auto sym = [&](const char *n) { return dlsym(a.handle, n); };
			a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(sym("ncclGetUniqueId"));
			a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(sym("ncclCommInitRank"));
			a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(sym("ncclCommDestroy"));
			a.GroupStart = reinterpret_cast<decltype(a.GroupStart)>(sym("ncclGroupStart"));
			a.GroupEnd = reinterpret_cast<decltype(a.GroupEnd)>(sym("ncclGroupEnd"));
			a.Send = reinterpret_cast<decltype(a.Send)>(sym("ncclSend"));
			a.Recv = reinterpret_cast<decltype(a.Recv)>(sym("ncclRecv"));
			a.AllGather = reinterpret_cast<decltype(a.AllGather)>(sym("ncclAllGather"));
			a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(sym("ncclGetErrorString"));
			if (!a.GetUniqueId || !a.CommInitRank || !a.CommDestroy || !a.GroupStart || !a.GroupEnd || !a.Send || !a.Recv || !a.AllGather) a.handle = nullptr;
			return a;
		}();
		if (!api.handle) throw DeviceError("RCCL (librccl.so) is not available: sharded runs over several GPUs need it");
		return api;
	}
	void check(ncclResult_t r, const char *what) const {
		if (r != ncclSuccess) throw DeviceError(std::string("RCCL ") + what + ": " + (GetErrorString ? GetErrorString(r) : "error"));
	}
};

// ---- transports --------------------------------------------------------------------------------------------------------
struct Transport {
	int rank = 0, world = 1;
	virtual ~Transport() {}
	virtual const char *name() const = 0;
	// all-to-all(v) of n_arrays device arrays at once: array a has elem[a]-byte elements; the piece for peer p starts at element send_off[p]
	// of d_send[a] (send_cnt[p] elements) and lands at element recv_off[p] of d_recv[a] (recv_cnt[p] elements).
	// in_place: bit a set = the piece of array a that stays on this shard is NOT copied (the caller reads it in d_send[a])
	// Enqueued on `st`.  The local and the shm plane return when the pieces have landed; RCCL does NOT wait: the caller orders its consumers
	// on `st` (kernels queued behind it, or an event -- a chunk of the exchange travels while the next is partitioned and the previous hashed).
	virtual void exchange_at(int n_arrays, const void *const *d_send, void *const *d_recv, const size_t *elem, const uint64_t *send_off, const uint64_t *send_cnt,
	                         const uint64_t *recv_off, const uint64_t *recv_cnt, hipStream_t st, uint32_t in_place = 0) = 0;
	// The same with the blocks back to back: the one for peer p starts at element sum(send_cnt[< p]) and lands at element sum(recv_cnt[< p]).
	void exchange(int n_arrays, const void *const *d_send, void *const *d_recv, const size_t *elem, const uint64_t *send_cnt, const uint64_t *recv_cnt,
	              hipStream_t st, uint32_t in_place = 0) {
		std::vector<uint64_t> send_off(static_cast<size_t>(world), 0), recv_off(static_cast<size_t>(world), 0);
		for (int p = 1; p < world; ++p) { send_off[size_t(p)] = send_off[size_t(p) - 1] + send_cnt[p - 1]; recv_off[size_t(p)] = recv_off[size_t(p) - 1] + recv_cnt[p - 1]; }
		exchange_at(n_arrays, d_send, d_recv, elem, send_off.data(), send_cnt, recv_off.data(), recv_cnt, st, in_place);
	}
	virtual void gather_host(const void *mine, size_t bytes, void *all) = 0;   // all: world x bytes, rank order
	// every shard's device block to every shard: block of rank p = bytes[p] at d_all + off[p]
	virtual void gather_dev(const void *d_mine, void *d_all, const size_t *off, const size_t *bytes, hipStream_t st) = 0;
	virtual void barrier() = 0;
	// host memory shared by the shards of the node (collective call; at least `bytes`); *d_ptr = this shard's device view
	virtual void *shared_host(int slot, size_t bytes, void **d_ptr) = 0;

	template <class T>
	void gather_vec(const std::vector<T> &mine, std::vector<T> &all, std::vector<size_t> &count) {   // variable-length host rows
		// ONE collective when every rank's rows fit a small fixed slot (the length travels in front of them) -- most of a pass's
		// host gathers are a few hundred bytes, and a collective of staged bytes costs its latency, not its size; a second one
		// with the padded rows only when somebody's did not fit.
		constexpr size_t SLOT = 16384;
		const uint64_t n = mine.size();
		const size_t fit = (SLOT - 8) / sizeof(T);
		std::vector<unsigned char> slot(SLOT, 0), slots(SLOT * size_t(world));
		std::memcpy(slot.data(), &n, 8);
		if (n && n <= fit) std::memcpy(slot.data() + 8, mine.data(), size_t(n) * sizeof(T));
		gather_host(slot.data(), SLOT, slots.data());
		std::vector<uint64_t> ns(size_t(world), 0);
		uint64_t mx = 0;
		for (int p = 0; p < world; ++p) { std::memcpy(&ns[size_t(p)], slots.data() + size_t(p) * SLOT, 8); mx = std::max(mx, ns[size_t(p)]); }
		count.assign(size_t(world), 0);
		all.clear();
		if (mx <= fit) {
			for (int p = 0; p < world; ++p) {
				count[size_t(p)] = size_t(ns[size_t(p)]);
				const T *rows = reinterpret_cast<const T *>(slots.data() + size_t(p) * SLOT + 8);
				all.insert(all.end(), rows, rows + ns[size_t(p)]);
			}
			return;
		}
		std::vector<T> pad(mx), buf(size_t(mx) * size_t(world));
		if (n) std::memcpy(static_cast<void *>(pad.data()), mine.data(), size_t(n) * sizeof(T));
		gather_host(pad.data(), size_t(mx) * sizeof(T), buf.data());
		for (int p = 0; p < world; ++p) {
			count[size_t(p)] = size_t(ns[size_t(p)]);
			all.insert(all.end(), buf.begin() + size_t(p) * mx, buf.begin() + size_t(p) * mx + ns[size_t(p)]);
		}
	}
};

// Shards inside one process.  One hub per group; every member runs on its own host thread.
struct LocalHub {
	int n;
	std::mutex m;
	std::condition_variable cv;
	int arrived = 0;
	uint64_t generation = 0;
	std::vector<const void *> p0, p1;   // per rank: pointers published for the current collective
	struct Shared { void *host = nullptr; size_t bytes = 0; } shared[4];
	bool failed = false;                // a member threw: wake the others instead of deadlocking
	explicit LocalHub(int n_) : n(n_), p0(size_t(n_), nullptr), p1(size_t(n_), nullptr) {}
	~LocalHub() { for (auto &s : shared) if (s.host) (void)hipHostFree(s.host); }
	void barrier() {
		std::unique_lock<std::mutex> lk(m);
		if (failed) throw DeviceError("another shard of the group failed");
		const uint64_t g = generation;
		if (++arrived == n) { arrived = 0; ++generation; cv.notify_all(); return; }
		cv.wait(lk, [&] { return generation != g || failed; });
		if (failed && generation == g) throw DeviceError("another shard of the group failed");
	}
	void fail() { std::lock_guard<std::mutex> lk(m); failed = true; cv.notify_all(); }
};

struct LocalTransport : Transport {
	std::shared_ptr<LocalHub> hub;
	LocalTransport(std::shared_ptr<LocalHub> h, int r) : hub(std::move(h)) { rank = r; world = hub->n; }
	const char *name() const override { return "local"; }
	struct PubAt { const void *const *d_send; const size_t *elem; const uint64_t *send_off, *send_cnt; };
	void exchange_at(int n_arrays, const void *const *d_send, void *const *d_recv, const size_t *elem, const uint64_t *send_off, const uint64_t *send_cnt,
	                 const uint64_t *recv_off, const uint64_t *recv_cnt, hipStream_t st, uint32_t in_place = 0) override {
		HIP_CHECK(stream_wait(st));   // the pieces the peers copy were written before this point of `st`
		PubAt pub{d_send, elem, send_off, send_cnt};
		hub->p0[size_t(rank)] = &pub;
		hub->barrier();
		for (int p = 0; p < world; ++p) {
			const PubAt *src = static_cast<const PubAt *>(hub->p0[size_t(p)]);
			if (src->send_cnt[rank] != recv_cnt[p]) throw DeviceError("exchange: a peer's piece differs from the agreed size");
			for (int a = 0; a < n_arrays; ++a)
				if (recv_cnt[p] && !(p == rank && (in_place >> a & 1u)))
					HIP_CHECK(hipMemcpyAsync(static_cast<char *>(d_recv[a]) + recv_off[p] * elem[a], static_cast<const char *>(src->d_send[a]) + src->send_off[rank] * elem[a],
					                         size_t(recv_cnt[p]) * elem[a], hipMemcpyDefault, st));
		}
		HIP_CHECK(stream_wait(st));
		hub->barrier();   // the senders' buffers may be reused
	}
	void gather_host(const void *mine, size_t bytes, void *all) override {
		hub->p0[size_t(rank)] = mine;
		hub->barrier();
		for (int p = 0; p < world; ++p) std::memcpy(static_cast<char *>(all) + size_t(p) * bytes, hub->p0[size_t(p)], bytes);
		hub->barrier();
	}
	void gather_dev(const void *d_mine, void *d_all, const size_t *off, const size_t *bytes, hipStream_t st) override {
		HIP_CHECK(stream_wait(st));   // what the peers are about to read was produced on this stream
		hub->p1[size_t(rank)] = d_mine;
		hub->barrier();
		for (int p = 0; p < world; ++p)
			if (bytes[p]) HIP_CHECK(hipMemcpyAsync(static_cast<char *>(d_all) + off[p], hub->p1[size_t(p)], bytes[p], hipMemcpyDefault, st));
		HIP_CHECK(stream_wait(st));
		hub->barrier();
	}
	void barrier() override { hub->barrier(); }
	void *shared_host(int slot, size_t bytes, void **d_ptr) override {
		hub->barrier();
		if (rank == 0) {
			LocalHub::Shared &s = hub->shared[slot];
			if (s.bytes < bytes) {
				if (s.host) HIP_CHECK(hipHostFree(s.host));
				s.host = nullptr; s.bytes = 0;
				const size_t cap = bytes + bytes / 4 + 4096;
				HIP_CHECK(hipHostMalloc(&s.host, cap, hipHostMallocPortable | hipHostMallocMapped));
				s.bytes = cap;
			}
		}
		hub->barrier();
		void *host = hub->shared[slot].host;
		HIP_CHECK(hipHostGetDevicePointer(d_ptr, host, 0));
		return host;
	}
};

// The small host tables of the processes of one node meet in shared memory, not on the device: a pass makes a dozen host collectives of
// a few bytes to a few hundred KB, and each one staged through the GPU (copy in, ncclAllGather, copy out, stream wait) costs ~50-100 us
// of launch and synchronisation latency whatever its size.  HostMailbox: one POSIX shm object per run (named by the run's unique id;
// rank 0 creates it, the others attach, rank 0 unlinks it once all are in), `world` slots of SLOT bytes, twice (two halves used in
// turn), and a sense-reversing barrier on an atomic counter.  A gather = write my slot, barrier, read all slots: ONE barrier -- a rank
// can only be two collectives ahead of another when that one has passed the barrier in between, i.e. has finished reading the half
// about to be overwritten.  Payloads beyond SLOT bytes take the RCCL path.  A rank that does not arrive within TIMEOUT_S (a peer died)
// fails the collective instead of hanging.
struct HostMailbox {
	static constexpr size_t SLOT = size_t(1) << 20;
	// seconds a rank waits for the others (attach, barrier) before it fails the collective for everybody; DROPEST_MAILBOX_TIMEOUT_S (tests)
	static unsigned timeout_s() { static const unsigned t = [] { const char *e = getenv("DROPEST_MAILBOX_TIMEOUT_S"); return e ? unsigned(std::max(1, atoi(e))) : 300u; }(); return t; }
	struct Header { std::atomic<uint32_t> attached, arrived, generation, failed; std::atomic<uint64_t> magic; };
	static uint64_t magic_of(uint64_t token) { return mix64(token ^ 0x6d61696c626f7821ull) | 1ull; }   // never 0: a fresh object reads as zeros
	int rank = 0, world = 1;
	char *base = nullptr;
	size_t bytes = 0;
	uint64_t phase = 0;
	Header *hdr() const { return reinterpret_cast<Header *>(base); }
	char *slot(uint64_t ph, int p) const { return base + 4096 + ((ph & 1) * size_t(world) + size_t(p)) * SLOT; }
	HostMailbox(uint64_t token, int r, int w) : rank(r), world(w) {
		bytes = 4096 + 2 * size_t(w) * SLOT;
		char path[96];
		std::snprintf(path, sizeof(path), "/dropest_mb_%llx_%d", (unsigned long long)token, w);
		int fd = -1;
		const auto t0 = std::chrono::steady_clock::now();
		if (r == 0) {
			shm_unlink(path);   // a leftover of a crashed run with the same id cannot be ours
			fd = shm_open(path, O_CREAT | O_EXCL | O_RDWR, 0600);
			if (fd < 0 || ftruncate(fd, off_t(bytes)) != 0) { if (fd >= 0) { close(fd); shm_unlink(path); } throw DeviceError("cannot create the host mailbox in /dev/shm"); }
		} else {
			for (;;) {   // rank 0 may not be there yet; a file that exists but is not sized yet is not ready either
				fd = shm_open(path, O_RDWR, 0600);
				if (fd >= 0) { struct stat st; if (fstat(fd, &st) == 0 && size_t(st.st_size) >= bytes) break; close(fd); fd = -1; }
				if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(timeout_s())) throw DeviceError("host mailbox: rank 0 did not create it");
				usleep(200);
			}
		}
		void *m = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
		close(fd);
		if (m == MAP_FAILED) { if (r == 0) shm_unlink(path); throw DeviceError("cannot map the host mailbox"); }
		base = static_cast<char *>(m);   // (a fresh shm object reads as zeros: the header starts at 0 / 0 / 0 / 0)
		// rank 0 signs the object it has just created; the others attach only to a signed one (an object of the same name that rank 0 is
		// about to unlink and replace -- a leftover -- never carries this run's word)
		// (a wait that times out leaves the constructor by an exception: no destructor runs, so the mapping -- and on rank 0 the name, which
		// is otherwise unlinked only once everybody is in -- are released here)
		try {
			if (r == 0) hdr()->magic.store(magic_of(token), std::memory_order_release);
			else wait_until([&] { return hdr()->magic.load(std::memory_order_acquire) == magic_of(token); }, "signature", false);
			hdr()->attached.fetch_add(1, std::memory_order_acq_rel);
			wait_until([&] { return hdr()->attached.load(std::memory_order_acquire) >= uint32_t(world); }, "attach");
		} catch (...) {
			munmap(base, bytes); base = nullptr;
			if (r == 0) shm_unlink(path);
			throw;
		}
		if (r == 0) shm_unlink(path);   // the mappings keep it alive; nothing is left behind on a crash
	}
	~HostMailbox() { if (base) munmap(base, bytes); }
	HostMailbox(const HostMailbox &) = delete;
	template <class F> void wait_until(F &&done, const char *what, bool heed_failed = true) {
		const auto t0 = std::chrono::steady_clock::now();
		for (uint32_t spins = 0; !done(); ++spins) {
			if (heed_failed && hdr()->failed.load(std::memory_order_acquire)) throw DeviceError("another shard of the run failed");
			if (spins < 2000) { dropest::host_cpu_relax(); continue; }
			sched_yield();
			if ((spins & 1023u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(timeout_s())) {
				hdr()->failed.store(1, std::memory_order_release);
				throw DeviceError(std::string("host mailbox: a shard did not arrive (") + what + ")");
			}
		}
	}
	void fail() { if (base) hdr()->failed.store(1, std::memory_order_release); }
	void barrier() {
		Header *h = hdr();
		const uint32_t g = h->generation.load(std::memory_order_acquire);
		if (h->arrived.fetch_add(1, std::memory_order_acq_rel) + 1 == uint32_t(world)) {
			h->arrived.store(0, std::memory_order_relaxed);
			h->generation.store(g + 1, std::memory_order_release);
			return;
		}
		wait_until([&] { return h->generation.load(std::memory_order_acquire) != g; }, "barrier");
	}
	bool fits(size_t n) const { return n <= SLOT; }
	void gather(const void *mine, size_t n, void *all) {   // n <= SLOT, the same on every rank
		const uint64_t ph = phase++;
		if (n) std::memcpy(slot(ph, rank), mine, n);
		barrier();
		for (int p = 0; p < world; ++p) if (n) std::memcpy(static_cast<char *>(all) + size_t(p) * n, slot(ph, p), n);
	}
};

// One process per GPU: RCCL for the device data; the small host tables through the HostMailbox above (RCCL all-gathers of staged bytes
// for payloads beyond its slots, or for everything with DROPEST_HOST_COLLECTIVES=rccl).  Shared host memory for the results: a POSIX
// shm object mapped and registered by every process of the node.
struct RcclTransport : Transport {
	ncclComm_t comm = nullptr;
	hipStream_t st0 = nullptr;          // the owning context's stream
	DevBuf<unsigned char> stage_in, stage_out;
	PinnedBuf<unsigned char> h_in, h_out;
	uint64_t token = 0;
	std::unique_ptr<HostMailbox> mailbox;
	struct Shm { void *host = nullptr; size_t bytes = 0; int gen = 0; } shm[4];
	// DROPEST_SHARD_DATAPLANE=shm: the device data of the collectives (exchange, gather_dev) crosses through POSIX shared memory instead of
	// RCCL -- every process stages what it sends in a segment of its own, the peers read it after a barrier.  For runs whose processes
	// share GPUs (RCCL refuses two ranks on one device): the multi-process tests on a one-GPU box run the whole step this way -- the
	// mailbox, the shared result buffers, the sequence of collectives are the real ones, only ncclSend / ncclRecv are stood in for.
	bool shm_plane = false;
	struct Stage { void *host = nullptr; size_t bytes = 0; uint64_t gen = 0; };
	Stage my_stage;
	std::vector<Stage> peer_stage;
	static void stage_path(char *out, size_t n, uint64_t token, int rank, uint64_t gen) { std::snprintf(out, n, "/dropest_dp_%llx_%d_%llu", (unsigned long long)token, rank, (unsigned long long)gen); }
	// collective: every rank makes sure its segment holds `need` bytes, then maps the peers' segments (again) where they were replaced
	void stage_prepare(size_t need) {
		uint64_t row[2] = {my_stage.gen, 0};
		if (need > my_stage.bytes) {
			if (my_stage.host) { char old[128]; stage_path(old, sizeof(old), token, rank, my_stage.gen); munmap(my_stage.host, my_stage.bytes); shm_unlink(old); my_stage.host = nullptr; }
			const size_t cap = need + need / 4 + 4096;
			char path[128];
			stage_path(path, sizeof(path), token, rank, my_stage.gen + 1);
			shm_unlink(path);
			const int fd = shm_open(path, O_CREAT | O_EXCL | O_RDWR, 0600);
			if (fd < 0 || posix_fallocate(fd, 0, off_t(cap)) != 0) { if (fd >= 0) { close(fd); shm_unlink(path); } throw DeviceError("cannot create the staging segment of the shm data plane"); }
			void *m = mmap(nullptr, cap, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
			close(fd);
			if (m == MAP_FAILED) { shm_unlink(path); throw DeviceError("cannot map the staging segment of the shm data plane"); }
			my_stage.host = m; my_stage.bytes = cap; ++my_stage.gen;
			row[0] = my_stage.gen;
		}
		row[1] = my_stage.bytes;
		std::vector<uint64_t> all(size_t(world) * 2);
		gather_host(row, 16, all.data());
		peer_stage.resize(size_t(world));
		for (int p = 0; p < world; ++p) {
			if (p == rank) continue;
			Stage &ps = peer_stage[size_t(p)];
			if (ps.gen == all[size_t(p) * 2] && ps.host) continue;
			if (ps.host) { munmap(ps.host, ps.bytes); ps.host = nullptr; }
			ps.gen = all[size_t(p) * 2]; ps.bytes = size_t(all[size_t(p) * 2 + 1]);
			if (!ps.gen) continue;
			char path[128];
			stage_path(path, sizeof(path), token, p, ps.gen);
			const int fd = shm_open(path, O_RDONLY, 0600);
			void *m = fd >= 0 ? mmap(nullptr, ps.bytes, PROT_READ, MAP_SHARED, fd, 0) : MAP_FAILED;
			if (fd >= 0) close(fd);
			if (m == MAP_FAILED) throw DeviceError("cannot map a peer's staging segment of the shm data plane");
			ps.host = m;
		}
	}
	RcclTransport(int r, int w, const uint8_t id_bytes[128], hipStream_t st) : st0(st) {
		rank = r; world = w;
		for (int i = 0; i < 128; ++i) token = token * 1099511628211ull + id_bytes[i];
		{ const char *dp = getenv("DROPEST_SHARD_DATAPLANE"); shm_plane = dp && std::string(dp) == "shm"; }
		if (shm_plane) { mailbox = std::make_unique<HostMailbox>(token, r, w); return; }   // one host by construction; no communicator
		const RcclApi &api = RcclApi::get();
		ncclUniqueId id;
		static_assert(sizeof(id) == 128, "ncclUniqueId");
		std::memcpy(&id, id_bytes, 128);
		api.check(api.CommInitRank(&comm, w, id, r), "ncclCommInitRank");
		const char *hc = getenv("DROPEST_HOST_COLLECTIVES");
		bool use_mailbox = !(hc && std::string(hc) == "rccl");
		if (use_mailbox && w > 1) {
			// The mailbox is POSIX shared memory: every rank must be on ONE host.  The ranks compare a word that names the host's running
			// kernel instance (boot id, else the host name) over the communicator first; ranks on several hosts keep the RCCL path for
			// their host collectives instead of waiting 300 s for a shm object that will never show up.
			uint64_t mine = 1469598103934665603ull;
			auto fold = [&](const char *s) { for (; *s; ++s) { mine ^= (unsigned char)*s; mine *= 1099511628211ull; } };
			char buf[256] = {0};
			if (FILE *f = fopen("/proc/sys/kernel/random/boot_id", "r")) { if (fgets(buf, sizeof(buf), f)) fold(buf); fclose(f); }
			if (!buf[0] && gethostname(buf, sizeof(buf) - 1) == 0) fold(buf);
			std::vector<uint64_t> all(size_t(w), 0);
			gather_host(&mine, 8, all.data());   // (no mailbox yet: the staged RCCL all-gather)
			for (int p = 0; p < w; ++p) use_mailbox &= all[size_t(p)] == mine;
		}
		if (use_mailbox) mailbox = std::make_unique<HostMailbox>(token, r, w);
	}
	~RcclTransport() override {
		for (auto &ps : peer_stage) if (ps.host) munmap(ps.host, ps.bytes);
		if (my_stage.host) { char path[128]; stage_path(path, sizeof(path), token, rank, my_stage.gen); munmap(my_stage.host, my_stage.bytes); shm_unlink(path); }
		for (auto &s : shm) if (s.host) { (void)hipHostUnregister(s.host); munmap(s.host, s.bytes); }
		if (comm) (void)RcclApi::get().CommDestroy(comm);
	}
	const char *name() const override { return shm_plane ? "shm" : "rccl"; }
	void exchange_at(int n_arrays, const void *const *d_send, void *const *d_recv, const size_t *elem, const uint64_t *send_off, const uint64_t *send_cnt,
	                 const uint64_t *recv_off, const uint64_t *recv_cnt, hipStream_t st, uint32_t in_place = 0) override {
		for (int a = 0; a < n_arrays; ++a)   // the piece a shard keeps never leaves the device: a plain copy (a self send / recv pair moves it at a fifth of the rate)
			if (send_cnt[rank] && !(in_place >> a & 1u))
				HIP_CHECK(hipMemcpyAsync(static_cast<char *>(d_recv[a]) + recv_off[rank] * elem[a], static_cast<const char *>(d_send[a]) + send_off[rank] * elem[a],
				                         size_t(send_cnt[rank]) * elem[a], hipMemcpyDeviceToDevice, st));
		if (shm_plane) {   // processes that share GPUs: the pieces cross through the staging segments, with the host in between
			uint64_t total = 0;
			for (int p = 0; p < world; ++p) total += p == rank ? 0 : send_cnt[p];
			size_t need = size_t(world) * 16;
			for (int a = 0; a < n_arrays; ++a) need += ((size_t(total) * elem[a] + 63) & ~size_t(63));
			stage_prepare(need);
			char *mine = static_cast<char *>(my_stage.host);
			// header: for every peer, where its piece starts in each array's staged run (in elements) and its length
			uint64_t *hdr = reinterpret_cast<uint64_t *>(mine);
			uint64_t run = 0;
			for (int p = 0; p < world; ++p) { hdr[2 * p] = run; hdr[2 * p + 1] = p == rank ? 0 : send_cnt[p]; run += hdr[2 * p + 1]; }
			HIP_CHECK(stream_wait(st));
			size_t at = size_t(world) * 16;
			for (int a = 0; a < n_arrays; ++a) {
				for (int p = 0; p < world; ++p)
					if (p != rank && send_cnt[p])
						HIP_CHECK(hipMemcpy(mine + at + size_t(hdr[2 * p]) * elem[a], static_cast<const char *>(d_send[a]) + send_off[p] * elem[a], size_t(send_cnt[p]) * elem[a], hipMemcpyDeviceToHost));
				at += (size_t(total) * elem[a] + 63) & ~size_t(63);
			}
			barrier();
			for (int p = 0; p < world; ++p) {
				if (p == rank || !recv_cnt[p]) continue;
				const char *peer = static_cast<const char *>(peer_stage[size_t(p)].host);
				const uint64_t *ph = reinterpret_cast<const uint64_t *>(peer);
				if (ph[2 * rank + 1] != recv_cnt[p]) throw DeviceError("shm data plane: a peer's piece differs from the agreed size");
				uint64_t ptotal = 0;
				for (int q = 0; q < world; ++q) ptotal += ph[2 * q + 1];
				size_t pat = size_t(world) * 16;
				for (int a = 0; a < n_arrays; ++a) {
					HIP_CHECK(hipMemcpy(static_cast<char *>(d_recv[a]) + recv_off[p] * elem[a], peer + pat + size_t(ph[2 * rank]) * elem[a], size_t(recv_cnt[p]) * elem[a], hipMemcpyHostToDevice));
					pat += (size_t(ptotal) * elem[a] + 63) & ~size_t(63);
				}
			}
			barrier();   // nobody overwrites its segment while a peer still reads it
			HIP_CHECK(stream_wait(st));   // (the copies above are synchronous and the kept piece was waited for before them: nothing is left on `st`)
			return;
		}
		// (no wait on this plane: whatever reads the received pieces is queued behind them on `st` -- cb_sample, cb_insert -- or behind an event
		// on it, and the send buffers are not rewritten before the next pass's partition, on the context's stream too)
		const RcclApi &api = RcclApi::get();
		api.check(api.GroupStart(), "ncclGroupStart");
		for (int a = 0; a < n_arrays; ++a)
			for (int p = 0; p < world; ++p) {
				if (p == rank) continue;
				if (send_cnt[p]) api.check(api.Send(static_cast<const char *>(d_send[a]) + send_off[p] * elem[a], size_t(send_cnt[p]) * elem[a], ncclUint8, p, comm, st), "ncclSend");
				if (recv_cnt[p]) api.check(api.Recv(static_cast<char *>(d_recv[a]) + recv_off[p] * elem[a], size_t(recv_cnt[p]) * elem[a], ncclUint8, p, comm, st), "ncclRecv");
			}
		api.check(api.GroupEnd(), "ncclGroupEnd");
	}
	void gather_host(const void *mine, size_t bytes, void *all) override {
		if (mailbox && mailbox->fits(bytes)) { mailbox->gather(mine, bytes, all); return; }
		if (shm_plane) {   // no communicator: a payload beyond a slot goes through the mailbox slot by slot
			std::vector<unsigned char> part(HostMailbox::SLOT * size_t(world));
			for (size_t at = 0; at < bytes; at += HostMailbox::SLOT) {
				const size_t n = std::min(HostMailbox::SLOT, bytes - at);
				mailbox->gather(static_cast<const char *>(mine) + at, n, part.data());
				for (int p = 0; p < world; ++p) std::memcpy(static_cast<char *>(all) + size_t(p) * bytes + at, part.data() + size_t(p) * n, n);
			}
			return;
		}
		const RcclApi &api = RcclApi::get();
		const size_t b = std::max<size_t>(bytes, 1);
		stage_in.ensure(b); stage_out.ensure(b * size_t(world)); h_in.ensure(b); h_out.ensure(b * size_t(world));
		std::memcpy(h_in.p, mine, bytes);
		HIP_CHECK(hipMemcpyAsync(stage_in.p, h_in.p, b, hipMemcpyHostToDevice, st0));
		api.check(api.AllGather(stage_in.p, stage_out.p, b, ncclUint8, comm, st0), "ncclAllGather");
		HIP_CHECK(hipMemcpyAsync(h_out.p, stage_out.p, b * size_t(world), hipMemcpyDeviceToHost, st0));
		HIP_CHECK(stream_wait(st0));
		for (int p = 0; p < world; ++p) std::memcpy(static_cast<char *>(all) + size_t(p) * bytes, h_out.p + size_t(p) * b, bytes);
	}
	void gather_dev(const void *d_mine, void *d_all, const size_t *off, const size_t *bytes, hipStream_t st) override {
		if (shm_plane) {
			stage_prepare(bytes[rank] + 64);
			HIP_CHECK(stream_wait(st));
			if (bytes[rank]) HIP_CHECK(hipMemcpy(my_stage.host, d_mine, bytes[rank], hipMemcpyDeviceToHost));
			barrier();
			for (int p = 0; p < world; ++p) {
				if (!bytes[p]) continue;
				if (p == rank) HIP_CHECK(hipMemcpy(static_cast<char *>(d_all) + off[p], d_mine, bytes[p], hipMemcpyDeviceToDevice));
				else HIP_CHECK(hipMemcpy(static_cast<char *>(d_all) + off[p], peer_stage[size_t(p)].host, bytes[p], hipMemcpyHostToDevice));
			}
			barrier();
			return;
		}
		const RcclApi &api = RcclApi::get();
		api.check(api.GroupStart(), "ncclGroupStart");
		for (int p = 0; p < world; ++p) {
			if (bytes[rank]) api.check(api.Send(d_mine, bytes[rank], ncclUint8, p, comm, st), "ncclSend");
			if (bytes[p]) api.check(api.Recv(static_cast<char *>(d_all) + off[p], bytes[p], ncclUint8, p, comm, st), "ncclRecv");
		}
		api.check(api.GroupEnd(), "ncclGroupEnd");   // (stream-ordered like exchange(): the kernels that read d_all follow on `st`)
	}
	void barrier() override { unsigned char x = 0; std::vector<unsigned char> all(static_cast<size_t>(world)); gather_host(&x, 1, all.data()); }
	void *shared_host(int slot, size_t bytes, void **d_ptr) override {
		Shm &s = shm[slot];
		// every rank must take the same branch: agree on the capacity first
		uint64_t want = s.bytes >= bytes ? 0 : uint64_t(bytes + bytes / 4 + 4096);
		std::vector<uint64_t> wants(static_cast<size_t>(world));
		gather_host(&want, 8, wants.data());
		uint64_t cap = 0;
		for (uint64_t w : wants) cap = std::max(cap, w);
		if (cap) {
			cap = std::max<uint64_t>(cap, s.bytes);
			if (s.host) { HIP_CHECK(hipHostUnregister(s.host)); munmap(s.host, s.bytes); s.host = nullptr; s.bytes = 0; }
			++s.gen;
			uint64_t pid0 = uint64_t(getpid());
			std::vector<uint64_t> pids(static_cast<size_t>(world));
			gather_host(&pid0, 8, pids.data());
			char path[128];
			std::snprintf(path, sizeof(path), "/dropest_%llx_%llu_%d_%d", (unsigned long long)token, (unsigned long long)pids[0], slot, s.gen);
			uint64_t ok = 1;
			int fd = -1;
			if (rank == 0) {
				fd = shm_open(path, O_CREAT | O_EXCL | O_RDWR, 0600);
				// The pages are reserved now (a full tmpfs fails here, not with SIGBUS later) -- on the NUMA node of this rank's GPU, where ROCm
				// puts pinned host memory and where the threads that widen the matrices into this buffer run (matrix_decode.h): left to the
				// default policy they land on whatever node this thread happens to run on, and every slot is then written across the sockets.
				h_in.ensure(4096);
				const int node = dropest::numa_node_of(h_in.p);
				unsigned long mask[16] = {0};
				const bool bound = node >= 0 && node < 1024 && (mask[node / 64] |= 1ul << (node % 64), syscall(SYS_set_mempolicy, 1 /* MPOL_PREFERRED */, mask, 1024ul) == 0);
				if (fd < 0 || posix_fallocate(fd, 0, off_t(cap)) != 0) ok = 0;
				if (bound) (void)syscall(SYS_set_mempolicy, 0 /* MPOL_DEFAULT */, nullptr, 0ul);
			}
			std::vector<uint64_t> oks(static_cast<size_t>(world));
			gather_host(&ok, 8, oks.data());
			if (!oks[0]) { if (fd >= 0) { close(fd); shm_unlink(path); } throw DeviceError("cannot reserve the shared result buffer in /dev/shm"); }
			if (rank != 0) fd = shm_open(path, O_RDWR, 0600);
			void *host = fd >= 0 ? mmap(nullptr, size_t(cap), PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0) : MAP_FAILED;
			if (fd >= 0) close(fd);
			ok = host != MAP_FAILED && hipHostRegister(host, size_t(cap), hipHostRegisterMapped | hipHostRegisterPortable) == hipSuccess;
			gather_host(&ok, 8, oks.data());
			if (rank == 0) shm_unlink(path);   // the mappings keep it alive; nothing is left behind on a crash
			for (uint64_t o : oks) if (!o) throw DeviceError("cannot map / register the shared result buffer");
			s.host = host; s.bytes = size_t(cap);
		}
		HIP_CHECK(hipHostGetDevicePointer(d_ptr, s.host, 0));
		return s.host;
	}
};

}  // namespace dropest
