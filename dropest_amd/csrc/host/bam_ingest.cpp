// bam_ingest.cpp -- see bam_ingest.h: BamReader (the host reader), BamRecord and the inflate of one block.  The controller is in
// bam_controller.cpp, the device path in bam_device.cpp.
#include "bam_parse.h"
#include "fast_inflate.h"

#include <zlib.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <deque>
#include <memory>

static inline void bam_cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
	__builtin_ia32_pause();
#elif defined(__aarch64__)
	__asm__ __volatile__("yield");
#endif
}

namespace Estimation {
namespace BamProcessing {

void inflate_block(const RawBlock &b, uint8_t *out) {
	if (b.isize == 0) return;
	// the block decoder of fast_inflate.h first (about three times zlib 1.2.11's rate); a block it refuses -- and any block when
	// DROPEST_BAM_ZLIB is set -- goes through zlib below.  Either way CRC-32 and ISIZE of the block are checked.
	static const bool force_zlib = getenv("DROPEST_BAM_ZLIB") != nullptr;
	if (!force_zlib && fastinflate::inflate_raw(b.cdata, b.clen, out, b.isize)) {
		if (fastinflate::crc32(out, b.isize) != b.crc) throw std::runtime_error("Corrupt BGZF block (CRC)");
		return;
	}
	// one inflate state per thread, reset per block (inflateInit2 allocates its 40 KB window every time)
	struct State { z_stream zs; bool ready = false; ~State() { if (ready) inflateEnd(&zs); } };
	static thread_local State st;
	z_stream &zs = st.zs;
	if (!st.ready) {
		std::memset(&zs, 0, sizeof(zs));
		if (inflateInit2(&zs, -15) != Z_OK) throw std::runtime_error("zlib: inflateInit2 failed");
		st.ready = true;
	} else if (inflateReset2(&zs, -15) != Z_OK) throw std::runtime_error("zlib: inflateReset2 failed");
	zs.next_in = const_cast<Bytef *>(b.cdata); zs.avail_in = uInt(b.clen);
	zs.next_out = out; zs.avail_out = b.isize;
	const int rc = inflate(&zs, Z_FINISH);
	if (rc != Z_STREAM_END || zs.total_out != b.isize) throw std::runtime_error("Corrupt BGZF block (inflate)");
	if (crc32(crc32(0L, Z_NULL, 0), out, b.isize) != b.crc) throw std::runtime_error("Corrupt BGZF block (CRC)");
}

struct BamReader::Impl {
	std::string path;
	const uint8_t *map = nullptr;                      // the whole file, mapped read-only
	size_t map_size = 0, map_at = 0;
	unsigned threads = 1;
	static constexpr size_t BATCH_BLOCKS = 512;        // <= 32 MB of BAM per batch (a window of ~2e5 records; the workers are persistent: a dispatch costs microseconds)
	std::unique_ptr<WorkerPool> pool;                  // inflate workers (only touched by the one batch loader running at a time)
	static constexpr size_t HEADROOM = 1 << 20;
	// Decompressed windows live in a few recycled buffers (a fresh 32 MB allocation per batch would spend more time in
	// page faults than the inflate takes).  A batch leaves HEADROOM bytes free in front: the unconsumed tail of the
	// previous window (a partial record) is copied there, so a new batch is adopted without moving it.
	struct Buf {
		std::unique_ptr<uint8_t[]> p; size_t cap = 0, size = 0;
		void need(size_t n) { if (n > cap) { p.reset(new uint8_t[n]); cap = n; } }
		// Record boundaries found by the loader (walk_records): starts of the COMPLETE records that begin in this batch (buffer offsets),
		// first_start = the first of them or tail_start, tail_start = where the unfinished last record begins (= size if none).
		std::vector<uint32_t> rec_off;
		bool walked = false, consumed = false;
		size_t first_start = 0, tail_start = 0;
	};
	Buf cur;                                           // window being parsed: bytes [pos, cur.size)
	std::vector<Buf> spare;                            // recycled buffers (under qm)
	size_t pos = 0;
	bool file_done = false;
	// Batches are loaded by ONE background thread, strictly one after the other (block discovery, the walk chain and the cut record carry
	// state from batch to batch), up to DEPTH ahead of the parser: with a single batch in flight every slow batch of either side -- the
	// hosts are shared -- stalled the other (215 ms of waiting in a 950 ms ingest whose loader and parser each needed ~700).
	static constexpr size_t DEPTH = 3;
	std::thread loader;
	std::mutex qm;
	std::condition_variable q_cv;
	std::deque<Buf> ready;
	bool loader_started = false, loader_finished = false, loader_stop = false;
	std::exception_ptr loader_error;
	void loader_main() {
		try {
			for (;;) {
				Buf b;
				{
					std::unique_lock<std::mutex> lk(qm);
					q_cv.wait(lk, [&] { return loader_stop || ready.size() < DEPTH; });
					if (loader_stop) break;
					b = take_spare();
				}
				Buf out = load_batch(std::move(b));
				const bool last = file_done;
				{ std::lock_guard<std::mutex> lk(qm); ready.push_back(std::move(out)); if (last) loader_finished = true; }
				q_cv.notify_all();
				if (last) break;
			}
		} catch (...) {
			{ std::lock_guard<std::mutex> lk(qm); loader_error = std::current_exception(); loader_finished = true; }
			q_cv.notify_all();
		}
	}
	bool next_batch(Buf &out) {   // false: the stream has ended (an error of the loader is rethrown here)
		if (!loader_started) { loader_started = true; loader = std::thread([this] { loader_main(); }); }
		std::unique_lock<std::mutex> lk(qm);
		q_cv.wait(lk, [&] { return !ready.empty() || loader_finished; });
		if (ready.empty()) { if (loader_error) std::rethrow_exception(loader_error); return false; }
		out = std::move(ready.front());
		ready.pop_front();
		lk.unlock();
		q_cv.notify_all();
		return true;
	}
	void stop_loader() {
		if (!loader_started) return;
		{ std::lock_guard<std::mutex> lk(qm); loader_stop = true; }
		q_cv.notify_all();
		if (loader.joinable()) loader.join();
	}
	std::vector<std::string> refs;
	std::string text;
	const uint8_t *bytes() const { return cur.p.get(); }

	// The walk over the records (every record's length says where the next one starts: a dependent chain) used to run on the caller's
	// thread over data the inflate workers had just written on other cores -- 4 ms per 32 MB window, the floor of the whole ingest
	// (profiles/NOTES_r03.md).  Now every worker, after inflating block i, waits for the position block i - 1's walker ended at, walks
	// ITS block while it is hot in its own cache and hands the position on; the loader of a batch knows where the last record of the
	// batch before was cut.  walk_state: what the next batch needs to know about that cut.
	bool loader_walks = getenv("DROPEST_BAM_CALLER_WALKS") == nullptr;
	struct WalkState { bool valid = false; size_t tail_len = 0; uint8_t tail[4] = {0, 0, 0, 0}; uint32_t tail_record = 0; } walk_state;
	std::vector<std::vector<uint32_t>> block_starts;
	double load_ms = 0, discover_ms = 0; size_t n_batches = 0, n_walked = 0;   // diagnostics (DROPEST_BAM_TRACE)
	size_t first_batch_compressed = 0;                           // bytes of the file the first batch covered (read-count estimate)
	Buf load_batch(Buf out) {
		const auto t_begin = std::chrono::steady_clock::now();
		std::vector<RawBlock> blocks;
		blocks.reserve(BATCH_BLOCKS);
		while (blocks.size() < BATCH_BLOCKS) {
			RawBlock b;
			if (!read_block(map, map_size, map_at, b, path)) { file_done = true; break; }
			blocks.push_back(std::move(b));
		}
		if (!n_batches) first_batch_compressed = map_at;
		discover_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
		std::vector<size_t> off(blocks.size() + 1, HEADROOM);
		for (size_t i = 0; i < blocks.size(); ++i) off[i + 1] = off[i] + blocks[i].isize;
		out.need(off.back());
		out.size = off.back();
		uint8_t *base = out.p.get();
		// (inflate + the walk chain stop scaling at about 16 workers -- the chain is serial -- and more of them only take cores from
		// the parsers, which do scale: 64 inflate workers measured a third of the rate of 16)
		if (!pool) pool.reset(new WorkerPool(std::max(1u, std::min(threads, 16u))));
		const unsigned nt = pool->size();
		std::atomic<size_t> next_block{0};            // blocks differ in cost: taken one at a time, in file order
		out.walked = out.consumed = false; out.rec_off.clear();
		// where this batch's first record starts (buffer offset), if the batch before told us; batch 0 holds the header: walked below
		const size_t NB = blocks.size();
		bool chain = loader_walks && n_batches > 0 && walk_state.valid && NB > 0;
		size_t p0 = HEADROOM;
		bool size_from_new = false;                   // the cut went through the length field: its missing bytes open this batch
		if (chain) {
			if (walk_state.tail_len >= 4) p0 = HEADROOM + 4 + size_t(walk_state.tail_record) - walk_state.tail_len;
			else if (walk_state.tail_len > 0) size_from_new = true;
		}
		std::unique_ptr<std::atomic<uint64_t>[]> carry;   // carry[i] = 1 + position the walker of block i starts at (0: not known yet)
		std::atomic<bool> abort_walk{false}, corrupt{false};
		if (chain) {
			carry.reset(new std::atomic<uint64_t>[NB + 1]);
			for (size_t i = 0; i <= NB; ++i) carry[i].store(0, std::memory_order_relaxed);
			if (!size_from_new) carry[0].store(uint64_t(p0) + 1, std::memory_order_release);
			if (block_starts.size() < NB) block_starts.resize(NB);
		}
		try {
			pool->run([&](unsigned) {
				for (size_t i; (i = next_block.fetch_add(1)) < NB;) {
					try { inflate_block(blocks[i], base + off[i]); } catch (...) { abort_walk = true; throw; }
					if (!chain) continue;
					if (i == 0 && size_from_new) {
						const size_t missing = 4 - walk_state.tail_len;
						if (off[1] - off[0] < missing) { abort_walk = true; continue; }   // (a block shorter than the rest of a length field: the caller walks this batch)
						uint8_t sz[4];
						std::memcpy(sz, walk_state.tail, walk_state.tail_len);
						std::memcpy(sz + walk_state.tail_len, base + HEADROOM, missing);
						carry[0].store(uint64_t(HEADROOM + 4 + size_t(le32(sz)) - walk_state.tail_len) + 1, std::memory_order_release);
					}
					uint64_t c;
					for (unsigned spins = 0; (c = carry[i].load(std::memory_order_acquire)) == 0; ++spins) {
						if (abort_walk.load(std::memory_order_relaxed)) break;
						if (spins < 2000) bam_cpu_relax(); else std::this_thread::yield();   // (the walker before us may have lost its core)
					}
					if (c == 0) continue;
					size_t P = size_t(c - 1);
					std::vector<uint32_t> &st = block_starts[i];
					st.clear();
					const size_t end_i = off[i + 1];
					while (P + 4 <= end_i) {
						const uint32_t bs = le32(base + P);
						if (bs < 32 || P > 0xFFFFFFF0ull) { corrupt = true; abort_walk = true; break; }
						st.push_back(uint32_t(P));
						P += 4 + size_t(bs);
					}
					carry[i + 1].store(uint64_t(P) + 1, std::memory_order_release);
				}
			});
		} catch (const std::exception &e) { throw std::runtime_error(std::string(e.what()) + ": " + path); }
		(void)nt;
		if (corrupt) throw std::runtime_error("Corrupt BAM record: " + path);
		if (chain && !abort_walk) {
			size_t total = 0;
			for (size_t i = 0; i < NB; ++i) total += block_starts[i].size();
			out.rec_off.resize(total);
			size_t at = 0;
			for (size_t i = 0; i < NB; ++i) { if (!block_starts[i].empty()) std::memcpy(out.rec_off.data() + at, block_starts[i].data(), block_starts[i].size() * 4); at += block_starts[i].size(); }
			finish_walk(out, size_t(carry[NB].load() - 1));
		} else if (loader_walks && n_batches == 0 && NB > 0) walk_first_batch(out);
		else walk_state.valid = false;                 // (the caller walks; a later batch cannot know where its records start)
		load_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(); ++n_batches;
		return out;
	}
	// After the starts are known: drop the ones whose record does not end inside the batch (they are the tail), remember the cut.
	void finish_walk(Buf &out, size_t next_start) {
		const uint8_t *base = out.p.get();
		size_t tail_start = next_start;              // the position after the last started record (its length field may be cut: < 4 bytes left)
		while (!out.rec_off.empty()) {
			const size_t s = out.rec_off.back();
			if (s + 4 + size_t(le32(base + s)) <= out.size) break;
			tail_start = s;
			out.rec_off.pop_back();
		}
		if (tail_start > out.size) {                 // a record that runs past this whole batch: the caller's path handles such giants
			out.rec_off.clear(); out.walked = false; walk_state.valid = false;
			return;
		}
		out.walked = true; out.tail_start = tail_start; ++n_walked;
		out.first_start = !out.rec_off.empty() ? size_t(out.rec_off.front()) : tail_start;
		walk_state.valid = true;
		walk_state.tail_len = out.size - tail_start;
		if (walk_state.tail_len >= 4) walk_state.tail_record = le32(base + tail_start);
		else std::memcpy(walk_state.tail, base + tail_start, walk_state.tail_len);
	}
	// Batch 0 starts with the header (magic, text, reference names): parsed here only to find the first record, then one serial walk.
	void walk_first_batch(Buf &out) {
		walk_state.valid = false;
		const uint8_t *base = out.p.get();
		size_t o = HEADROOM;
		auto have = [&](size_t n) { return o + n <= out.size; };
		if (!have(12) || std::memcmp(base + o, "BAM\1", 4) != 0) return;
		const size_t l_text = le32(base + o + 4);
		if (!have(12 + l_text)) return;
		const uint32_t n_ref = le32(base + o + 8 + l_text);
		o += 12 + l_text;
		for (uint32_t r = 0; r < n_ref; ++r) {
			if (!have(4)) return;
			const size_t l_name = le32(base + o);
			if (!have(8 + l_name)) return;
			o += 8 + l_name;
		}
		size_t P = o;
		while (P + 4 <= out.size) {
			const uint32_t bs = le32(base + P);
			if (bs < 32 || P > 0xFFFFFFF0ull) throw std::runtime_error("Corrupt BAM record: " + path);
			out.rec_off.push_back(uint32_t(P));
			P += 4 + size_t(bs);
		}
		finish_walk(out, P);
		if (out.walked && out.rec_off.empty()) out.first_start = out.tail_start;
	}
	Buf take_spare() {
		if (spare.empty()) return Buf();
		Buf b = std::move(spare.back());
		spare.pop_back();
		return b;
	}
	// makes at least `need` bytes available at bytes()[pos..]; false if the stream ends first
	bool ensure(size_t need) {
		while (cur.size - pos < need) {
			Buf next;
			if (!next_batch(next)) return false;
			if (next.size <= HEADROOM) {   // an empty batch (the end of the file fell on a batch boundary): the next call ends the stream
				if (next.cap) { std::lock_guard<std::mutex> lk(qm); if (spare.size() < DEPTH + 2) spare.push_back(std::move(next)); }
				continue;
			}
			const size_t tail = cur.size - pos;
			if (tail <= HEADROOM && next.size >= HEADROOM) {
				if (tail) std::memcpy(next.p.get() + HEADROOM - tail, cur.p.get() + pos, tail);
				std::swap(cur, next);
				pos = HEADROOM - tail;
			} else {   // a tail longer than the headroom (one enormous record): concatenate into a larger buffer
				Buf big;
				const size_t payload = next.size > HEADROOM ? next.size - HEADROOM : 0;
				big.need(tail + payload);
				if (tail) std::memcpy(big.p.get(), cur.p.get() + pos, tail);
				if (payload) std::memcpy(big.p.get() + tail, next.p.get() + HEADROOM, payload);
				big.size = tail + payload;
				std::swap(cur, big);
				pos = 0;
				if (big.cap) { std::lock_guard<std::mutex> lk(qm); spare.push_back(std::move(big)); }
			}
			if (next.cap) { std::lock_guard<std::mutex> lk(qm); if (spare.size() < DEPTH + 2) spare.push_back(std::move(next)); }   // the old window, recycled
		}
		return true;
	}
};

BamReader::BamReader(const std::string &path, unsigned threads) : impl(new Impl()) {
	impl->path = path;
	impl->threads = threads ? threads : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
	{
		const int fd = open(path.c_str(), O_RDONLY);
		struct stat sb;
		if (fd < 0 || fstat(fd, &sb) != 0) { if (fd >= 0) close(fd); delete impl; throw std::runtime_error("Can't open BAM file: " + path); }
		impl->map_size = size_t(sb.st_size);
		void *m = impl->map_size ? mmap(nullptr, impl->map_size, PROT_READ, MAP_PRIVATE, fd, 0) : nullptr;
		close(fd);
		if (impl->map_size && m == MAP_FAILED) { delete impl; throw std::runtime_error("Can't open BAM file: " + path); }
		impl->map = static_cast<const uint8_t *>(m);
		if (m) (void)madvise(m, impl->map_size, MADV_SEQUENTIAL);
	}
	try {
		Impl &m = *impl;
		if (!m.ensure(12) || std::memcmp(m.bytes() + m.pos, "BAM\1", 4) != 0) throw std::runtime_error("Can't open BAM file: " + path);
		const uint32_t l_text = le32(m.bytes() + m.pos + 4);
		if (!m.ensure(12 + size_t(l_text))) throw std::runtime_error("Truncated BAM header: " + path);
		m.text.assign(reinterpret_cast<const char *>(m.bytes() + m.pos + 8), l_text);
		const uint32_t n_ref = le32(m.bytes() + m.pos + 8 + l_text);
		m.pos += 12 + size_t(l_text);
		for (uint32_t r = 0; r < n_ref; ++r) {
			if (!m.ensure(4)) throw std::runtime_error("Truncated BAM header: " + path);
			const uint32_t l_name = le32(m.bytes() + m.pos);
			if (!m.ensure(8 + size_t(l_name))) throw std::runtime_error("Truncated BAM header: " + path);
			m.refs.emplace_back(reinterpret_cast<const char *>(m.bytes() + m.pos + 4), l_name ? l_name - 1 : 0);
			m.pos += 8 + size_t(l_name);
		}
	} catch (...) {
		impl->stop_loader();
		if (impl->map) munmap(const_cast<uint8_t *>(impl->map), impl->map_size);
		delete impl; throw;
	}
}

BamReader::~BamReader() {
	impl->stop_loader();
	if (bam_trace_wanted()) std::fprintf(stderr, "[bam] %zu batches (%zu with the record boundaries from the loader), load %.1f ms (block discovery %.1f ms), %u inflate threads\n", impl->n_batches, impl->n_walked, impl->load_ms, impl->discover_ms, impl->threads);
	if (impl->map) munmap(const_cast<uint8_t *>(impl->map), impl->map_size);
	delete impl;
}

const std::vector<std::string> &BamReader::reference_names() const { return impl->refs; }
double BamReader::file_over_first_batch() const { return impl->first_batch_compressed ? double(impl->map_size) / double(impl->first_batch_compressed) : 1.0; }
const std::string &BamReader::header_text() const { return impl->text; }

void BamReader::parse_record(const uint8_t *at, BamRecord &rec) {
	const uint32_t block_size = le32(at);
	const uint8_t *p = at + 4;
	rec.ref_id = int32_t(le32(p));
	rec.position = int32_t(le32(p + 4));
	const uint32_t l_read_name = p[8];
	const uint32_t n_cigar = le16(p + 12);
	rec.flag = le16(p + 14);
	const uint32_t l_seq = le32(p + 16);
	const size_t fixed = 32, name_end = fixed + l_read_name;
	const size_t aux = name_end + size_t(n_cigar) * 4 + (size_t(l_seq) + 1) / 2 + l_seq;
	if (block_size < 32 || aux > block_size) throw std::runtime_error("Corrupt BAM record");
	int64_t ref_len = 0;                                                 // CIGAR ops: MIDNSHP=X -> 0..8 (SAMv1 §4.2)
	for (uint32_t k = 0; k < n_cigar; ++k) {
		const uint32_t op = le32(p + name_end + size_t(k) * 4);
		const uint32_t kind = op & 0xF;
		if (kind == 0 || kind == 2 || kind == 3 || kind == 7 || kind == 8) ref_len += op >> 4;
	}
	rec.end_position = int32_t(int64_t(rec.position) + ref_len);
	rec.name_view = std::string_view(reinterpret_cast<const char *>(p + fixed), l_read_name ? l_read_name - 1 : 0);
	rec.tags = p + aux; rec.tags_size = block_size - aux;
}

bool BamReader::next(BamRecord &rec) {
	Impl &m = *impl;
	if (!m.ensure(4)) return false;
	const uint32_t block_size = le32(m.bytes() + m.pos);
	if (block_size < 32) throw std::runtime_error("Corrupt BAM record: " + m.path);
	if (!m.ensure(4 + size_t(block_size))) throw std::runtime_error("Truncated BAM record: " + m.path);
	parse_record(m.bytes() + m.pos, rec);
	rec.name.assign(rec.name_view);
	m.pos += 4 + size_t(block_size);
	return true;
}

bool BamReader::next_window(const uint8_t *&data, std::vector<uint32_t> &offsets) {
	Impl &m = *impl;
	offsets.clear();
	if (m.cur.walked && m.cur.consumed) {   // the window handed out last time was the whole batch: what is left is the cut record
		const size_t tail = m.cur.size - m.pos;
		if (!m.ensure(tail + 1)) { if (tail) throw std::runtime_error("Truncated BAM record: " + m.path); return false; }
	} else if (!m.ensure(4)) return false;
	if (m.cur.walked && !m.cur.consumed) {
		// records of this batch as its loader found them; in front of them the record the last batch was cut in (its head was copied
		// to just before this batch's first byte, its end is where this batch's first own record starts)
		data = m.bytes() + m.pos;
		if (m.pos < m.cur.first_start) {
			const uint32_t bs = le32(data);
			if (bs < 32 || m.pos + 4 + size_t(bs) != m.cur.first_start) throw std::runtime_error("Corrupt BAM record: " + m.path);
			offsets.push_back(0);
		}
		offsets.reserve(offsets.size() + m.cur.rec_off.size());
		for (uint32_t s : m.cur.rec_off) offsets.push_back(uint32_t(s - m.pos));
		m.pos = m.cur.tail_start;
		m.cur.consumed = true;
		if (!offsets.empty()) return true;
		return next_window(data, offsets);       // (a batch without a single complete record: go on with the next one)
	}
	// (after a consumed batch only tail + 1 bytes are known to be there: the length field itself may be cut by the end of the file)
	if (!m.ensure(4)) { if (m.cur.size > m.pos) throw std::runtime_error("Truncated BAM record: " + m.path); return false; }
	const uint32_t first_size = le32(m.bytes() + m.pos);
	if (first_size < 32) throw std::runtime_error("Corrupt BAM record: " + m.path);
	if (!m.ensure(4 + size_t(first_size))) throw std::runtime_error("Truncated BAM record: " + m.path);
	data = m.bytes() + m.pos;
	const size_t avail = m.cur.size - m.pos;
	size_t o = 0;
	while (o + 4 <= avail) {
		const uint32_t bs = le32(data + o);
		if (bs < 32) throw std::runtime_error("Corrupt BAM record: " + m.path);
		if (o + 4 + size_t(bs) > avail || o > 0xFFFFFFF0ull) break;
		offsets.push_back(uint32_t(o));
		o += 4 + size_t(bs);
	}
	m.pos += o;
	return true;
}

bool BamRecord::get_string_tag(const std::string &tag, std::string_view &value, char *type_out) const {
	if (tag.size() != 2) return false;
	size_t o = 0;
	while (o + 3 <= tags_size) {
		const char t0 = char(tags[o]), t1 = char(tags[o + 1]), type = char(tags[o + 2]);
		o += 3;
		size_t len = 0;
		bool text = false;
		switch (type) {
			case 'A': case 'c': case 'C': len = 1; break;
			case 's': case 'S': len = 2; break;
			case 'i': case 'I': case 'f': len = 4; break;
			case 'Z': case 'H': { const void *e = std::memchr(tags + o, 0, tags_size - o); if (!e) return false; len = size_t(static_cast<const uint8_t *>(e) - (tags + o)) + 1; text = true; break; }
			case 'B': {
				if (o + 5 > tags_size) return false;
				const char sub = char(tags[o]);
				const uint32_t cnt = le32(tags + o + 1);
				const size_t w = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
				len = 5 + size_t(cnt) * w;
				break;
			}
			default: return false;   // unknown type: cannot skip safely
		}
		if (o + len > tags_size) return false;
		if (t0 == tag[0] && t1 == tag[1]) {
			if (type_out) *type_out = type;
			if (text) { value = std::string_view(reinterpret_cast<const char *>(tags + o), len - 1); return true; }
			if (type == 'A') { value = std::string_view(reinterpret_cast<const char *>(tags + o), 1); return true; }
			// numeric tag where a string is asked for: treated as absent; said once, the counters tell the rest
			static std::atomic<bool> warned{false};
			if (!warned.exchange(true))
				std::fprintf(stderr, "WARNING: BAM tag %c%c has the numeric type '%c' where a string (Z) is expected; records with it are handled as if the tag were absent\n", t0, t1, type);
			return false;
		}
		o += len;
	}
	return false;
}

void BamRecord::get_string_tags(const uint16_t *wanted, int n_wanted, std::string_view *values, bool *found) const {
	for (int k = 0; k < n_wanted; ++k) found[k] = false;
	bool closed[16] = {false};   // a tag met with a numeric type counts as absent, and later records of the same name are not looked at
	size_t o = 0;
	while (o + 3 <= tags_size) {
		const uint16_t name = uint16_t(tags[o] | (tags[o + 1] << 8));
		const char type = char(tags[o + 2]);
		o += 3;
		size_t len = 0;
		bool text = false;
		switch (type) {
			case 'A': case 'c': case 'C': len = 1; break;
			case 's': case 'S': len = 2; break;
			case 'i': case 'I': case 'f': len = 4; break;
			case 'Z': case 'H': { const void *e = std::memchr(tags + o, 0, tags_size - o); if (!e) return; len = size_t(static_cast<const uint8_t *>(e) - (tags + o)) + 1; text = true; break; }
			case 'B': {
				if (o + 5 > tags_size) return;
				const char sub = char(tags[o]);
				const uint32_t cnt = le32(tags + o + 1);
				const size_t w = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
				len = 5 + size_t(cnt) * w;
				break;
			}
			default: return;   // unknown type: cannot skip safely
		}
		if (o + len > tags_size) return;
		for (int k = 0; k < n_wanted && k < 16; ++k) {
			if (wanted[k] != name || !wanted[k] || found[k] || closed[k]) continue;
			if (text) { values[k] = std::string_view(reinterpret_cast<const char *>(tags + o), len - 1); found[k] = true; }
			else if (type == 'A') { values[k] = std::string_view(reinterpret_cast<const char *>(tags + o), 1); found[k] = true; }
			else {
				closed[k] = true;
				static std::atomic<bool> warned{false};
				if (!warned.exchange(true))
					std::fprintf(stderr, "WARNING: BAM tag %c%c has the numeric type '%c' where a string (Z) is expected; records with it are handled as if the tag were absent\n", char(name & 0xFF), char(name >> 8), type);
			}
		}
		o += len;
	}
}

bool BamRecord::get_string_tag(const std::string &tag, std::string &value, char *type_out) const {
	std::string_view v;
	if (!get_string_tag(tag, v, type_out)) return false;
	value.assign(v);
	return true;
}

}  // namespace BamProcessing
}  // namespace Estimation

// test hooks (tests/test_fast_inflate.py): the block decoder and the CRC against zlib's
extern "C" int dropest_test_fast_inflate(const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_len) {
	return fastinflate::inflate_raw(in, size_t(in_len), out, size_t(out_len)) ? 1 : 0;
}
extern "C" uint32_t dropest_test_crc32(const uint8_t *p, uint64_t n) { return fastinflate::crc32(p, size_t(n)); }
