// shard_validation.h -- merge validation statistics (`dropest -S`, validation.h) for the shards of a sharded or split run (included by shard_run.h).
//
// After a step every shard holds the same table G of the filtered candidates and the same column order of cm (mat[0]).  The statistics need
// pairs of ANY two filtered cells, so every shard ends with the same view of ALL filtered cells' molecules and the same estimator tables:
//   keys      every shard keys the rows of ITS filtered cells as validation_build_view does (molecule table rows of groups the UMI merge did not
//             rewrite, the umi_overrides rows on top), with the cell's GLOBAL position -- its column of cm, found through G by (rank, local id)
//             -- in the cell field, and sorts them.  Override UMIs above the UMI field: the distinct ones of all shards are gathered and
//             sorted, code = umask + 1 + index, so every shard numbers them alike and decides the "one more bit" alike.
//   gather    the row counts per position (host), then one gather_dev of the sorted blocks: 8 bytes per molecule of a filtered cell on EVERY
//             shard -- the price of a replicated view.
//   place     the gathered buffer is `world` sorted blocks and a cell's rows lie in exactly one: validation_place_kernel copies every cell's
//             segment to its place in the global order.  No sort of the union.
//             keys / gather / place are global_molecule_keys + gather_place_keys below: the read corrections of a sharded run
//             (shard_read_corrections.h) take the same sorted array and the rows of every column from them.
//   onwards   dropest_ctx::validation_finish_view: the (cell, gene) rows, the cells' ranges, the Poisson tables -- the one context's code.
//   sampler   dropest_ctx::validation_sample on the global barcode rows, on every shard: the same GlibcRand(42), the same pairs, no collective
//             inside the rounds.  cell1 / cell2 are COLUMNS OF THE FILTERED MATRIX.
//   pairs     common genes of all pairs on every shard (cheap), the pairs cut into `world` contiguous ranges of balanced key counts
//             (dropest_validation_cut_pairs), shard r runs the chunk loop on range r, the ranges' numbers are gathered on the host.
// Refusals that every shard reaches from the same gathered data (InvalidError, UnsupportedError) are thrown by all of them and leave the
// group usable; anything else fails the transport so that no peer waits for a shard that has left.
#pragma once

struct ValidationAgreed { int gene_bits = 0, umi_bits = 0; bool any_rows = false; std::vector<dropest::u64> above; };

// `k`: this shard's n_loc keys column | ..., sorted, the column above bit cell_shift (every key's column is one of this shard's own cells);
// with_vals (the same on every shard): one u64 of `vals` travels beside every key.  COLLECTIVE.  K.key / K.val: the keys (values) of all shards placed in global order, K.n of
// them, K.begin / K.count the rows of every column.  `keys_phase` is closed once the local rows are counted.
void dropest_shard::gather_place_keys(const u64 *k, const u64 *vals, bool with_vals, u32 n_loc, int cell_shift, u32 F, const std::string &what, const char *gather_phase,
                                      std::unique_ptr<Phase> &keys_phase, GlobalKeys &K) {
	using namespace dropest;
	dropest_ctx &c = *ctx;
	const Mat &M = mat[0];
	// rows per position: mine from the sorted keys, everybody's through the host, scanned
	struct CellCount { u32 col, count; };
	std::vector<CellCount> mine, every;
	if (n_loc) {
		DevBuf<u32> seg; seg.alloc(size_t(F) * 2);
		HIP_CHECK(hipMemsetAsync(seg.p, 0, size_t(F) * 8, c.stream));
		hipLaunchKernelGGL(validation_cell_segments_kernel, dim3(div_up(n_loc, 256)), dim3(256), 0, c.stream, k, n_loc, cell_shift, F, seg.p, seg.p + F);
		HIP_CHECK(hipGetLastError());
		std::vector<u32> h(size_t(F) * 2);
		c.fetch(h.data(), seg.p, size_t(F) * 8);
		uint64_t sum = 0;
		for (u32 j = 0; j < F; ++j)
			if (h[size_t(F) + j] > h[j]) {
				if (h[j] != sum) throw DeviceError("internal: a shard's view keys do not lie cell by cell");
				mine.push_back({j, h[size_t(F) + j] - h[j]}); sum += mine.back().count;
			}
		if (sum != n_loc) throw DeviceError("internal: a shard's view keys do not add up to its cells");
	}
	if (keep_validation_keys && !with_vals) { val_keys_local.resize(n_loc); if (n_loc) c.fetch(val_keys_local.data(), k, size_t(n_loc) * 8); }
	std::vector<size_t> cells_of;
	keys_phase.reset();
	Phase ph_gather(this, gather_phase);
	tr->gather_vec(mine, every, cells_of);
	std::vector<u32> cell_src(F, 0), &cell_cnt = K.count, &cell_dst = K.begin;
	cell_cnt.assign(F, 0); cell_dst.assign(F, 0);
	std::vector<size_t> off(static_cast<size_t>(world)), bytes(static_cast<size_t>(world));
	uint64_t N = 0;
	{
		size_t at = 0;
		for (int p = 0; p < world; ++p) {
			off[size_t(p)] = size_t(N) * 8;
			uint64_t run = N;
			for (size_t i = 0; i < cells_of[size_t(p)]; ++i, ++at) {
				const CellCount &cc = every[at];
				if (cc.col >= F || cell_cnt[cc.col] || int(G[M.col_row[cc.col]].rank) != p) throw InvalidError("internal: two shards claim rows of one filtered cell");
				if (run + cc.count >= 0xFFFFFFF0ull) throw UnsupportedError(what + ": too many molecules");
				cell_src[cc.col] = u32(run); cell_cnt[cc.col] = cc.count;
				run += cc.count;
			}
			bytes[size_t(p)] = size_t(run - N) * 8;
			N = run;
		}
	}
	if (size_t(n_loc) * 8 != bytes[size_t(rank)]) throw DeviceError("internal: the gathered row counts differ from this shard's rows");
	K.n = 0;
	if (!N) return;
	std::vector<u32> piece_cell, piece_first;
	{
		u32 run = 0;
		for (u32 j = 0; j < F; ++j) {
			cell_dst[j] = run; run += cell_cnt[j];
			for (u32 f = 0; f < cell_cnt[j]; f += VAL_SEG) { piece_cell.push_back(j); piece_first.push_back(f); }
		}
	}
	DevBuf<u64> gathered; gathered.alloc(size_t(N));
	const u32 n_pieces = u32(piece_cell.size());
	DevBuf<u32> d_cells, d_pieces; d_cells.alloc(size_t(F) * 3); d_pieces.alloc(size_t(n_pieces) * 2);
	c.upload(d_cells.p, cell_src.data(), size_t(F) * 4);
	c.upload(d_cells.p + F, cell_cnt.data(), size_t(F) * 4);
	c.upload(d_cells.p + 2 * size_t(F), cell_dst.data(), size_t(F) * 4);
	c.upload(d_pieces.p, piece_cell.data(), size_t(n_pieces) * 4);
	c.upload(d_pieces.p + n_pieces, piece_first.data(), size_t(n_pieces) * 4);
	DevBuf<u64> dummy; dummy.alloc(1);
	for (int pass = 0; pass < (with_vals ? 2 : 1); ++pass) {
		const u64 *src = pass ? vals : k;
		DevBuf<u64> &dst = pass ? K.val : K.key;
		tr->gather_dev(src ? src : dummy.p, gathered.p, off.data(), bytes.data(), c.stream);
		phases[gather_phase].bytes += double(N - n_loc) * 8;
		dst.alloc(size_t(N) + 1);
		c.timed("validation_place", double(N) * 16, [&] {
			hipLaunchKernelGGL(validation_place_kernel, dim3(std::min<u32>(n_pieces, 2048)), dim3(256), 0, c.stream, gathered.p, dst.p, d_cells.p, d_cells.p + F,
			                   d_cells.p + 2 * size_t(F), d_pieces.p, d_pieces.p + n_pieces, n_pieces);
		});
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(stream_wait(c.stream));   // (the tables of the launch leave this scope; `gathered` is written again)
	}
	K.n = u32(N);
}

// The molecules of ALL filtered cells under keys column of cm | gene | UMI field, sorted, on this shard (header comment: keys, gather, place).
// COLLECTIVE.  with_above: override UMIs the field cannot hold get codes above it (merge validation counts them); without, they are left
// out (no read carries one: the read corrections).  `what` starts the refusals' messages.
void dropest_shard::global_molecule_keys(GlobalKeys &K, bool with_above, const std::string &what, const char *keys_phase, const char *gather_phase) {
	using namespace dropest;
	dropest_ctx &c = *ctx;
	const Mat &M = mat[0];
	const u32 F = K.F = u32(M.ncols);
	K.n = 0; K.any_rows = false;
	std::unique_ptr<Phase> ph_keys(new Phase(this, keys_phase));
	const KeyLayout &L = c.layout;
	const u32 nm = c.initialized ? c.n_mol : 0;
	// my cells' positions; rewritten groups of my filtered cells: their keys for the device to skip, their rows under view keys
	std::vector<u32> pos(std::max<u32>(c.n_cells, 1), 0xFFFFFFFFu);
	u32 mine_cells = 0;
	for (u32 j = 0; j < F; ++j) {
		const GRow &r = G[M.col_row[j]];
		if (int(r.rank) != rank) continue;
		if (r.local_id >= c.n_cells) throw DeviceError("internal: a row of the global table names a cell this shard does not have");
		pos[r.local_id] = j; ++mine_cells;
	}
	std::vector<u64> rewritten;
	struct Row { u64 cg, umi; bool above; };
	std::vector<Row> orows;
	std::vector<u64> above_mine;
	if (mine_cells)
		for (auto const &kv : c.umi_overrides) {
			const u32 cell = u32(kv.first >> L.gene_bits);
			if (cell >= c.n_cells || pos[cell] == 0xFFFFFFFFu) continue;
			rewritten.push_back(kv.first);
			if ((kv.first & L.gene_none) == L.gene_none) continue;
			for (const UmiOverride &o : kv.second) {
				u64 field = 0;
				const bool in_field = c.map_umi(o.umi, field);
				if (!in_field && !with_above) continue;
				if (!in_field) above_mine.push_back(o.umi);
				orows.push_back({(u64(pos[cell]) << L.gene_bits) | (kv.first & L.gene_none), in_field ? field : o.umi, !in_field});
			}
		}
	std::sort(rewritten.begin(), rewritten.end());
	std::sort(above_mine.begin(), above_mine.end());
	above_mine.erase(std::unique(above_mine.begin(), above_mine.end()), above_mine.end());
	// one host gather: who has rows, the key fields they were keyed with, a local table too large to count, the UMIs above the field
	ValidationAgreed A;
	bool too_many = false;
	{
		const bool has = mine_cells && (nm || !orows.empty());
		std::vector<u64> words{has ? 1ull : 0ull, u64(L.gene_bits), u64(L.umi_bits), (u64(nm) + orows.size() >= 0xFFFFFFF0ull) ? 1ull : 0ull}, all;
		words.insert(words.end(), above_mine.begin(), above_mine.end());
		std::vector<size_t> cnt;
		tr->gather_vec(words, all, cnt);
		size_t at = 0;
		for (int p = 0; p < world; ++p) {
			const u64 *w = all.data() + at;
			if (cnt[size_t(p)] < 4) throw DeviceError("internal: a shard's validation header is short");
			if (w[0]) {
				if (A.any_rows && (A.gene_bits != int(w[1]) || A.umi_bits != int(w[2]))) throw InvalidError("internal: the shards keyed their molecules with different gene / UMI fields");
				A.any_rows = true; A.gene_bits = int(w[1]); A.umi_bits = int(w[2]);
			}
			too_many |= w[3] != 0;
			A.above.insert(A.above.end(), w + 4, w + cnt[size_t(p)]);
			at += cnt[size_t(p)];
		}
		std::sort(A.above.begin(), A.above.end());
		A.above.erase(std::unique(A.above.begin(), A.above.end()), A.above.end());
	}
	if (too_many) throw UnsupportedError(what + ": too many molecules");
	if (!A.any_rows) return;
	K.any_rows = true;
	const u64 umask = A.umi_bits ? ((1ull << A.umi_bits) - 1ull) : 0ull;
	K.gene_bits = A.gene_bits;
	K.umi_bits = A.umi_bits + (A.above.empty() ? 0 : 1);
	if (u64(A.above.size()) > umask + 1) throw UnsupportedError(what + ": more rewritten UMIs outside the UMI field than one more bit holds");
	const int rank_bits = std::max(1, bit_length(uint64_t(F ? F - 1 : 0)));
	const int total_bits = rank_bits + A.gene_bits + K.umi_bits;
	if (total_bits > 64) throw UnsupportedError(what + ": the view's key (cell rank, gene, UMI) is wider than 64 bits");
	std::vector<u64> extra;
	extra.reserve(orows.size());
	for (const Row &r : orows) {
		const u64 code = r.above ? umask + 1 + u64(std::lower_bound(A.above.begin(), A.above.end(), r.umi) - A.above.begin()) : r.umi;
		extra.push_back((r.cg << K.umi_bits) | code);
	}

	// my rows under view keys, sorted
	const size_t cap = std::max<size_t>(size_t(nm) + extra.size(), 1);
	c.keys_a.ensure(cap); c.keys_b.ensure(cap); c.vals_a.ensure(cap); c.vals_b.ensure(cap);
	u32 n_loc = 0;
	if (mine_cells && (nm || !extra.empty())) {
		u32 kept = 0;
		if (nm) {
			c.remap.ensure(pos.size());
			c.upload(c.remap.p, pos.data(), pos.size() * 4);
			DevBuf<u64> d_rewritten; d_rewritten.alloc(std::max<size_t>(rewritten.size(), 1));
			c.upload(d_rewritten.p, rewritten.data(), rewritten.size() * 8);
			c.scalars.ensure(16);
			HIP_CHECK(hipMemsetAsync(c.scalars.p, 0, 16, c.stream));
			hipLaunchKernelGGL(validation_view_keys_kernel, dim3(div_up(nm, 256)), dim3(256), 0, c.stream, c.mol_key.p, nm, L.umi_bits, L.gene_bits, L.gene_none,
			                   K.umi_bits, c.remap.p, d_rewritten.p, u32(rewritten.size()), c.keys_a.p, c.scalars.p);
			HIP_CHECK(hipGetLastError());
			c.fetch(&kept, c.scalars.p, 4);
		}
		c.upload(c.keys_a.p + kept, extra.data(), extra.size() * 8);
		n_loc = kept + u32(extra.size());
	}
	u64 *k = c.keys_a.p, *k_alt = c.keys_b.p;
	u32 *v = c.vals_a.p, *v_alt = c.vals_b.p;
	if (n_loc) c.radix_sort(k, v, k_alt, v_alt, n_loc, total_bits >= 64 ? ~0ull : ((1ull << total_bits) - 1ull));
	gather_place_keys(k, nullptr, false, n_loc, A.gene_bits + K.umi_bits, F, what, gather_phase, ph_keys, K);
}

void dropest_shard::validation_global_view(dropest_ctx::ValidationView &V) {
	using namespace dropest;
	dropest_ctx &c = *ctx;
	const auto t0 = std::chrono::steady_clock::now();
	const Mat &M = mat[0];
	if (M.col_row.size() != M.ncols) throw DeviceError("internal: the filtered matrix has no column table");
	const u32 F = V.F = u32(M.ncols);
	V.n_mol = V.n_cg = 0;
	V.cells.resize(F); V.umis.resize(F);
	for (u32 j = 0; j < F; ++j) { V.cells[j] = j; V.umis[j] = u32(G[M.col_row[j]].total_umis); }   // Cell::umis_number() = the TOTAL_UMIS stat
	if (F < 2) return;
	{
		std::vector<std::string> text(F);
		for (u32 j = 0; j < F; ++j) text[j] = decode_code(G[M.col_row[j]].barcode, c.side);   // (every shard has the whole side-string table)
		c.validation_set_barcodes(V, text);
	}
	GlobalKeys K;
	global_molecule_keys(K, true, "merge validation", "validation:keys", "validation:gather_place");
	if (K.any_rows) { V.gene_bits = K.gene_bits; V.gene_none = (1ull << K.gene_bits) - 1ull; V.umi_bits = K.umi_bits; }
	if (!K.n) { V.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); return; }
	V.mol_key = std::move(K.key);
	V.n_mol = K.n;
	if (keep_validation_keys) { val_keys_placed.resize(size_t(K.n)); c.fetch(val_keys_placed.data(), V.mol_key.p, size_t(K.n) * 8); }
	{ Phase ph_rows(this, "validation:rows_tables"); c.validation_finish_view(V); }
	V.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// Plain host code: pairs [bounds[r], bounds[r + 1]) go to shard r.  Range r ends behind the first pair at which the running sum of cnt
// reaches (r + 1) * total / world; pairs without common genes ride along; without any common gene the pairs are dealt in equal numbers.
static void validation_cut_pairs(const uint32_t *cnt, uint64_t n_pairs, int32_t world, uint64_t *bounds) {
	unsigned __int128 total = 0;
	for (uint64_t p = 0; p < n_pairs; ++p) total += cnt[p];
	bounds[0] = 0;
	if (total == 0) {
		for (int32_t r = 1; r <= world; ++r) bounds[r] = uint64_t((unsigned __int128)n_pairs * unsigned(r) / unsigned(world));
		return;
	}
	unsigned __int128 run = 0;
	uint64_t p = 0;
	for (int32_t r = 0; r < world; ++r) {
		const unsigned __int128 target = total * unsigned(r + 1) / unsigned(world);
		while (p < n_pairs && run < target) run += cnt[p++];
		bounds[r + 1] = p;
	}
	bounds[world] = n_pairs;
}

void dropest_shard::run_merge_validation(const dropest_validation_opts *opts_in, dropest_validation_sample *samples, u32 n_samples) {
	using namespace dropest;
	dropest_ctx &c = *ctx;
	if (!stepped || !c.initialized) throw InvalidError("You must initialize container");
	if (n_samples && !samples) throw InvalidError("null argument");
	const dropest_validation_opts opts = opts_in ? *opts_in : dropest_validation_opts{0, 0, 0};
	// The first collective: do all shards ask for the same thing?  Every shard sees every shard's words and all of them refuse alike, before
	// any collective of data whose size or number depends on the request.
	{
		std::vector<u64> words{u64(n_samples), opts.max_draws, opts.round_candidates, opts.max_keys_per_chunk}, all;
		for (u32 s = 0; s < n_samples; ++s) { words.push_back(samples[s].min_ed); words.push_back(samples[s].max_ed); words.push_back(samples[s].n_pairs); }
		std::vector<size_t> cnt;
		tr->gather_vec(words, all, cnt);
		size_t at = 0;
		for (int p = 0; p < world; ++p) {
			if (cnt[size_t(p)] != cnt[0] || !std::equal(all.begin() + long(at), all.begin() + long(at + cnt[size_t(p)]), all.begin()))
				throw InvalidError("merge validation: shard " + std::to_string(p) + " was called with other samples or options than shard 0 (every shard of the run makes the same call)");
			at += cnt[size_t(p)];
		}
	}
	for (u32 s = 0; s < n_samples; ++s)
		if (samples[s].n_pairs > 0xFFFFFFF0ull) throw UnsupportedError("more than 2^32-16 pairs in one validation sample");
	HIP_CHECK(hipSetDevice(c.cfg.device));
	Phase whole(this, "validation");
	dropest_ctx::ValidationView V;
	{ Phase ph(this, "validation:view"); validation_global_view(V); }
	std::vector<u32> a, b;
	for (u32 s = 0; s < n_samples; ++s) {
		dropest_validation_sample &S = samples[s];
		S.ms_view = V.ms; S.ms_sampler = S.ms_evaluation = 0; S.chunks = 0;
		{ Phase ph(this, "validation:sampler"); c.validation_sample(V, opts, S, a, b); }
		Phase ph(this, "validation:evaluation");
		const auto t0 = std::chrono::steady_clock::now();
		const u32 NP = u32(a.size());
		if (!NP) continue;
		std::vector<u32> inter(NP, 0);
		std::vector<double> expected(NP, 0.0), prob(NP, 1.0);
		dropest_ctx::ValidationPairs P;
		if (c.validation_common_genes(V, a, b, P)) {   // (the same answer on every shard: the views are identical)
			std::vector<uint64_t> bounds(size_t(world) + 1);
			validation_cut_pairs(P.cnt.data(), NP, world, bounds.data());
			const u32 q0 = u32(bounds[size_t(rank)]), q1 = u32(bounds[size_t(rank) + 1]);
			struct Rec { double expected, prob; u32 inter, chunks; };
			std::vector<Rec> mine(q1 - q0), every;
			u32 chunks = 0;
			if (q1 > q0) {
				chunks = c.validation_evaluate_range(V, opts, P, q0, q1, inter.data(), expected.data());
				dropest_ctx::validation_tail(q1 - q0, inter.data() + q0, expected.data() + q0, prob.data() + q0);
			}
			for (u32 p = q0; p < q1; ++p) mine[p - q0] = Rec{expected[p], prob[p], inter[p], 0};
			std::vector<size_t> cnt;
			tr->gather_vec(mine, every, cnt);
			std::vector<u32> chunks_all(static_cast<size_t>(world));
			tr->gather_host(&chunks, 4, chunks_all.data());
			if (every.size() != NP) throw DeviceError("internal: the shards' ranges of pairs do not add up to the sample");
			for (u32 p = 0; p < NP; ++p) { inter[p] = every[p].inter; expected[p] = every[p].expected; prob[p] = every[p].prob; }
			for (u32 x : chunks_all) S.chunks += x;
		} else
			dropest_ctx::validation_tail(NP, inter.data(), expected.data(), prob.data());
		for (u32 p = 0; p < NP; ++p) {
			if (S.intersection) S.intersection[p] = inter[p];
			if (S.expected) S.expected[p] = expected[p];
			if (S.probability) S.probability[p] = prob[p];
		}
		S.ms_evaluation = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	}
	c.collect_timings();
}

extern "C" {

dropest_status dropest_validation_cut_pairs(const uint32_t *cnt, uint64_t n_pairs, int32_t world, uint64_t *bounds) {
	return guarded([&] {
		if (!bounds || (n_pairs && !cnt)) throw InvalidError("null argument");
		if (world < 1) throw InvalidError("a number of shards above 0");
		validation_cut_pairs(cnt, n_pairs, world, bounds);
	});
}

dropest_status dropest_shard_merge_validation_samples(dropest_shard *s, const dropest_validation_opts *opts, dropest_validation_sample *samples, uint32_t n_samples) {
	return guarded([&] {
		if (!s) throw InvalidError("null shard");
		try { s->run_merge_validation(opts, samples, n_samples); }
		catch (const InvalidError &) { throw; }       // (reached by every shard alike: nobody is left waiting)
		catch (const UnsupportedError &) { throw; }
		catch (...) {   // the other shards must not wait for this one forever
			if (auto *lt = dynamic_cast<dropest::LocalTransport *>(s->tr.get())) lt->hub->fail();
			if (auto *rt = dynamic_cast<dropest::RcclTransport *>(s->tr.get())) if (rt->mailbox) rt->mailbox->fail();
			throw;
		}
	});
}

dropest_status dropest_shard_group_merge_validation_samples(dropest_shard *const *shards, int32_t n, const dropest_validation_opts *opts, dropest_validation_sample *samples,
                                                            uint32_t n_samples) {
	return guarded([&] {
		if (!shards || n < 1 || (n_samples && !samples)) throw InvalidError("null argument");
		// shard 0 fills the caller's arrays; the others compute the same numbers and keep none of them
		std::vector<std::vector<dropest_validation_sample>> own(static_cast<size_t>(n));
		for (int i = 1; i < n; ++i) {
			own[size_t(i)].assign(samples, samples + n_samples);
			for (dropest_validation_sample &S : own[size_t(i)]) { S.cell1 = S.cell2 = nullptr; S.umis1 = S.umis2 = S.edit_distance = S.intersection = nullptr; S.expected = S.probability = nullptr; }
		}
		std::vector<dropest_status> rc(size_t(n), DROPEST_OK);
		std::vector<std::string> msg(static_cast<size_t>(n));
		std::vector<std::thread> pool;
		for (int i = 0; i < n; ++i)
			pool.emplace_back([&, i] {
				rc[size_t(i)] = dropest_shard_merge_validation_samples(shards[i], opts, i ? own[size_t(i)].data() : samples, n_samples);
				if (rc[size_t(i)] != DROPEST_OK) msg[size_t(i)] = dropest_last_error();
			});
		for (auto &t : pool) t.join();
		for (int i = 0; i < n; ++i)
			if (rc[size_t(i)] != DROPEST_OK && msg[size_t(i)].find("another shard of the group failed") == std::string::npos) {
				if (rc[size_t(i)] == DROPEST_ERR_UNSUPPORTED) throw UnsupportedError("shard " + std::to_string(i) + ": " + msg[size_t(i)]);
				throw InvalidError("shard " + std::to_string(i) + ": " + msg[size_t(i)]);
			}
		for (int i = 0; i < n; ++i) if (rc[size_t(i)] != DROPEST_OK) throw InvalidError("shard " + std::to_string(i) + ": " + msg[size_t(i)]);
	});
}

// Test hook (tests/test_gpu_validation_sharded.py): the view keys of the last validation on a shard whose option "keep_validation_keys" is
// on.  which = 0: this shard's own sorted block, 1: the placed keys of all shards.  out may be null (the count alone).
int dropest_test_validation_keys(dropest_shard *s, int which, uint64_t *n, uint64_t *out) {
	if (!s || !n) return -1;
	const std::vector<dropest::u64> &k = which ? s->val_keys_placed : s->val_keys_local;
	*n = k.size();
	if (out && !k.empty()) std::memcpy(out, k.data(), k.size() * 8);
	return 0;
}

}  // extern "C"
