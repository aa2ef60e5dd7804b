// validation.h -- merge validation statistics, `dropest -S` (ResultsPrinter::save_validation_stats, ResultsPrinter.cpp:476-509, over
// MergeProbabilityValidator::run_validation, MergeProbabilityValidator.cpp:8-46): random pairs of filtered cells at a given barcode
// distance and the estimator's numbers for each, on the state the container is in NOW.
//
//   view      The filtered cells' molecules under keys of their own: rank in filtered_cells() | gene | UMI field.  The molecule table on the
//             device gives every row of a filtered cell that bears a gene and whose (cell, gene) group the UMI merge has not rewritten; the
//             rewritten groups' rows come from the host map umi_overrides, as for_each_molecule reads them (an override UMI with no place in
//             this pass's UMI field gets a code above the field, one more bit).  radix_sort, then run_segmented_reduce for the (cell, gene)
//             rows and the cells' row ranges: the pair kernels of -M (common_genes, pair_ranges, umig_intersect) read the view unchanged.
//             Nothing but mol_key / n_mol of the context's tables is read, so what a merge left of the other tables does not matter.
//   tables    UMI distribution -> classes -> collisions table, once per validation from the view (poisson_tables_from_umi_codes).
//   sampler   k_validation.h, in rounds; rand() values from a GlibcRand of this call, seeded 42 for every sample.
//   pairs     in chunks of at most max_keys_per_chunk common genes: umig_intersect, then keys -> distinct keys -> est() -> sums
//             (poisson_expected_pairs).  A pair's numbers depend on its own keys only: est() of a key is one block's fixed-order sum, the
//             pair's sum runs in gene order.  The Poisson tail on host threads (poisson_upper_tail).
#pragma once

#include "k_validation.h"

// barcodes as text: the packed codes do not hold 'N' or other escaped barcodes
void dropest_ctx::validation_set_barcodes(ValidationView &V, const std::vector<std::string> &text) {
	using namespace dropest;
	const size_t F = text.size();
	std::vector<unsigned char> rows(F * VAL_STRIDE, 0);
	for (size_t i = 0; i < F; ++i) {
		const std::string &s = text[i];
		if (s.size() >= size_t(VAL_COL)) throw UnsupportedError("merge validation takes barcodes of at most 31 characters");
		std::memcpy(rows.data() + i * VAL_STRIDE, s.data(), s.size());
		rows[i * VAL_STRIDE + VAL_STRIDE - 1] = (unsigned char)s.size();
	}
	V.barcodes.alloc(F * (VAL_STRIDE / 16));
	upload(V.barcodes.p, rows.data(), rows.size());
}

// From the sorted view keys onwards: V.mol_key (n_mol keys, ascending; one word of room behind them), F and umi_bits are set by whoever made
// the keys -- this context from its own tables (validation_build_view), or a shard from the blocks of all shards (shard_validation.h).
void dropest_ctx::validation_finish_view(ValidationView &V) {
	using namespace dropest;
	const u32 n = V.n_mol, F = V.F;
	V.n_cg = 0;
	if (!n) return;
	// (the scratch of the sorts below: a shard's own tables may be smaller than the view of all shards)
	keys_a.ensure(n); keys_b.ensure(n); vals_a.ensure(n); vals_b.ensure(n);
	// (cell, gene) rows: runs of key >> UMI bits, their lengths scanned into cg_mol_begin
	DevBuf<u32> run_cnt;
	{
		hipLaunchKernelGGL(validation_shift_keys_kernel, dim3(div_up(n, 256)), dim3(256), 0, stream, V.mol_key.p, n, V.umi_bits, ~0ull, keys_a.p);
		UmiRuns p{};
		p.keys = keys_a.p;
		V.n_cg = run_segmented_reduce(*this, "validation:cell_gene", p, n, 8, [&](u32 t) {
			V.cg_key.alloc(size_t(t) + 1); run_cnt.alloc(size_t(t) + 1); V.cg_mol_begin.alloc(size_t(t) + 1);
			zero_async(*this, run_cnt.p, (size_t(t) + 1) * 4);
			p.run_key = V.cg_key.p; p.out[0] = run_cnt.p;
		});
		scan_counts(run_cnt.p, V.cg_mol_begin.p, V.n_cg, scalars.p);
		HIP_CHECK(hipMemcpyAsync(V.cg_mol_begin.p + V.n_cg, &V.n_mol, 4, hipMemcpyHostToDevice, stream));
		HIP_CHECK(stream_wait(stream));
	}
	// cells: runs of (cell, gene) key >> gene bits -> the row range of every rank (cells without molecules keep 0, 0)
	{
		V.cell_cg_begin.alloc(F); V.cell_cg_count.alloc(F);
		zero_async(*this, V.cell_cg_begin.p, size_t(F) * 4);
		zero_async(*this, V.cell_cg_count.p, size_t(F) * 4);
		hipLaunchKernelGGL(validation_shift_keys_kernel, dim3(div_up(V.n_cg, 256)), dim3(256), 0, stream, V.cg_key.p, V.n_cg, V.gene_bits, ~0ull, keys_a.p);
		UmiRuns p{};
		p.keys = keys_a.p;
		DevBuf<u64> run_cell; DevBuf<u32> cell_cnt, cell_begin;
		const u32 runs = run_segmented_reduce(*this, "validation:cells", p, V.n_cg, 8, [&](u32 t) {
			run_cell.alloc(size_t(t) + 1); cell_cnt.alloc(size_t(t) + 1); cell_begin.alloc(size_t(t) + 1);
			zero_async(*this, cell_cnt.p, (size_t(t) + 1) * 4);
			p.run_key = run_cell.p; p.out[0] = cell_cnt.p;
		});
		scan_counts(cell_cnt.p, cell_begin.p, runs, scalars.p);
		hipLaunchKernelGGL(validation_cell_rows_kernel, dim3(div_up(runs, 256)), dim3(256), 0, stream, run_cell.p, cell_cnt.p, cell_begin.p, runs,
		                   V.cell_cg_begin.p, V.cell_cg_count.p);
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(stream_wait(stream));
	}

	// the estimator's tables, once: UMI fields of the view's rows -> distribution -> classes -> collisions table
	{
		scalars.ensure(16);
		HIP_CHECK(hipMemsetAsync(scalars.p, 0, 16, stream));
		hipLaunchKernelGGL(max_gene_size_kernel, dim3(div_up(V.n_cg, 256)), dim3(256), 0, stream, V.cg_key.p, V.cg_mol_begin.p, V.n_cg, V.gene_none, scalars.p + 1);
		const u64 code_mask = V.umi_bits >= 64 ? ~0ull : ((1ull << V.umi_bits) - 1ull);
		hipLaunchKernelGGL(validation_shift_keys_kernel, dim3(div_up(n, 256)), dim3(256), 0, stream, V.mol_key.p, n, 0, code_mask, keys_a.p);
		HIP_CHECK(hipGetLastError());
		u32 head[2] = {0, 0};
		fetch(head, scalars.p, 8);
		ptab = PoissonTables{};
		if (head[1]) poisson_tables_from_umi_codes(n, code_mask, head[1]);
	}
}

void dropest_ctx::validation_build_view(ValidationView &V) {
	using namespace dropest;
	const auto t0 = std::chrono::steady_clock::now();
	const KeyLayout &L = layout;
	V.cells = filtered_cells();
	const u32 F = V.F = u32(V.cells.size());
	V.n_mol = V.n_cg = 0;
	V.gene_bits = L.gene_bits; V.gene_none = L.gene_none;
	V.umis.resize(F);
	for (u32 i = 0; i < F; ++i) V.umis[i] = u32(real[filtered_ridx[i]].row.total_umis);   // Cell::umis_number() = the TOTAL_UMIS stat
	if (F < 2) return;
	{
		std::vector<std::string> text(F);
		for (u32 i = 0; i < F; ++i) text[i] = barcode_of(real[filtered_ridx[i]]);
		validation_set_barcodes(V, text);
	}
	if (!n_mol) return;

	// rewritten groups of filtered cells: their keys for the device to skip, their rows under view keys
	std::vector<u32> rank(n_cells, 0xFFFFFFFFu);
	for (u32 i = 0; i < F; ++i) rank[V.cells[i]] = i;
	const u64 umask = L.umi_bits ? ((1ull << L.umi_bits) - 1ull) : 0ull;
	std::vector<u64> rewritten, extra;
	struct Row { u64 cg; u64 umi; };
	std::vector<Row> orows;
	std::unordered_map<u64, u64> above;   // override UMIs outside this pass's UMI field -> codes above it
	for (auto const &kv : umi_overrides) {
		const u32 cell = u32(kv.first >> L.gene_bits);
		if (cell >= n_cells || rank[cell] == 0xFFFFFFFFu) continue;
		rewritten.push_back(kv.first);
		if ((kv.first & L.gene_none) == L.gene_none) continue;
		for (const UmiOverride &o : kv.second) {
			u64 field = 0;
			if (!map_umi(o.umi, field)) field = umask + 1 + above.emplace(o.umi, u64(above.size())).first->second;
			orows.push_back({(u64(rank[cell]) << L.gene_bits) | (kv.first & L.gene_none), field});
		}
	}
	std::sort(rewritten.begin(), rewritten.end());
	V.umi_bits = L.umi_bits + (above.empty() ? 0 : 1);
	if (u64(above.size()) > umask + 1) throw UnsupportedError("merge validation: more rewritten UMIs outside the UMI field than one more bit holds");
	const int rank_bits = std::max(1, bit_length(uint64_t(F - 1)));
	const int total_bits = rank_bits + L.gene_bits + V.umi_bits;
	if (total_bits > 64) throw UnsupportedError("merge validation: the view's key (cell rank, gene, UMI) is wider than 64 bits");
	extra.reserve(orows.size());
	for (const Row &r : orows) extra.push_back((r.cg << V.umi_bits) | r.umi);

	const size_t cap = size_t(n_mol) + extra.size();
	if (cap >= 0xFFFFFFF0ull) throw UnsupportedError("merge validation: too many molecules");
	keys_a.ensure(cap); keys_b.ensure(cap); vals_a.ensure(cap); vals_b.ensure(cap);
	remap.ensure(std::max<u32>(n_cells, 1));
	upload(remap.p, rank.data(), size_t(n_cells) * 4);
	DevBuf<u64> d_rewritten; d_rewritten.alloc(std::max<size_t>(rewritten.size(), 1));
	upload(d_rewritten.p, rewritten.data(), rewritten.size() * 8);
	scalars.ensure(16);
	HIP_CHECK(hipMemsetAsync(scalars.p, 0, 16, stream));
	hipLaunchKernelGGL(validation_view_keys_kernel, dim3(div_up(n_mol, 256)), dim3(256), 0, stream, mol_key.p, n_mol, L.umi_bits, L.gene_bits, L.gene_none,
	                   V.umi_bits, remap.p, d_rewritten.p, u32(rewritten.size()), keys_a.p, scalars.p);
	HIP_CHECK(hipGetLastError());
	u32 kept = 0;
	fetch(&kept, scalars.p, 4);
	upload(keys_a.p + kept, extra.data(), extra.size() * 8);
	const u32 n = V.n_mol = kept + u32(extra.size());
	if (!n) return;

	u64 *k = keys_a.p, *k_alt = keys_b.p;
	u32 *v = vals_a.p, *v_alt = vals_b.p;
	radix_sort(k, v, k_alt, v_alt, n, total_bits >= 64 ? ~0ull : ((1ull << total_bits) - 1ull));
	V.mol_key.alloc(size_t(n) + 1);
	HIP_CHECK(hipMemcpyAsync(V.mol_key.p, k, size_t(n) * 8, hipMemcpyDeviceToDevice, stream));

	validation_finish_view(V);
	V.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

void dropest_ctx::validation_sample(const ValidationView &V, const dropest_validation_opts &opts, dropest_validation_sample &S, std::vector<u32> &a,
                                    std::vector<u32> &b) {
	using namespace dropest;
	const auto t0 = std::chrono::steady_clock::now();
	constexpr uint64_t MAX_ROUND = uint64_t(1) << 22;
	const u32 n = u32(S.n_pairs), F = V.F;
	const uint64_t max_draws = opts.max_draws ? opts.max_draws : (uint64_t(1) << 30);
	S.n_found = S.draws_used = 0; S.complete = 0; S.rounds = 0;
	a.clear(); b.clear();
	if (F < 2 || n == 0) { S.complete = n == 0; return; }
	GlibcRand gen(42);   // srand(42) at the start of every run (MergeProbabilityValidator.cpp:14); never the container's own sequence
	DevBuf<u32> d_a, d_b, d_ed, d_cand, d_rnd, d_res, d_bcount, d_boff;
	d_a.alloc(n); d_b.alloc(n); d_ed.alloc(n); d_cand.alloc(n);
	std::vector<u32> rnd;
	uint64_t tested = 0;
	u32 found = 0;
	while (found < n && tested < max_draws) {
		uint64_t R;
		if (opts.round_candidates) R = opts.round_candidates;
		else if (tested == 0) R = uint64_t(n) + n / 8 + 64;
		else if (found == 0) R = MAX_ROUND;
		else R = uint64_t(double(n - found) * double(tested) / double(found) * 1.125) + 64;
		R = std::min(std::min(R, MAX_ROUND), max_draws - tested);
		const u32 r = u32(R), blocks = div_up(r, u32(VAL_THREADS));
		rnd.resize(size_t(r) * 2);
		for (size_t i = 0; i < rnd.size(); ++i) rnd[i] = u32(gen.next());
		d_rnd.ensure(rnd.size()); d_res.ensure(r); d_bcount.ensure(blocks); d_boff.ensure(blocks);
		upload(d_rnd.p, rnd.data(), rnd.size() * 4);
		scalars.ensure(16);
		timed("validation_sample", double(r) * 12, [&] {
			hipLaunchKernelGGL(validation_sample_kernel, dim3(blocks), dim3(VAL_THREADS), 0, stream, d_rnd.p, r, F, V.barcodes.p, S.min_ed, S.max_ed, d_res.p,
			                   d_bcount.p);
		});
		scan_counts(d_bcount.p, d_boff.p, blocks, scalars.p);
		hipLaunchKernelGGL(validation_scatter_kernel, dim3(blocks), dim3(VAL_THREADS), 0, stream, d_rnd.p, d_res.p, r, F, d_boff.p, found, n, d_a.p, d_b.p, d_ed.p,
		                   d_cand.p);
		HIP_CHECK(hipGetLastError());
		u32 accepted = 0;
		fetch(&accepted, scalars.p, 4);
		++S.rounds;
		if (uint64_t(found) + accepted >= n) {   // the n-th pair lies in this round: the reference stops drawing right behind it
			u32 last = 0;
			fetch(&last, d_cand.p + (n - 1), 4);
			S.draws_used = tested + last + 1;
			found = n;
			break;
		}
		found += accepted;
		tested += r;
		S.draws_used = tested;
	}
	S.n_found = found;
	S.complete = found == n;
	a.resize(found); b.resize(found);
	std::vector<u32> ed(found);
	fetch(a.data(), d_a.p, size_t(found) * 4);
	fetch(b.data(), d_b.p, size_t(found) * 4);
	fetch(ed.data(), d_ed.p, size_t(found) * 4);
	for (u32 p = 0; p < found; ++p) {
		if (S.cell1) S.cell1[p] = V.cells[a[p]];
		if (S.cell2) S.cell2[p] = V.cells[b[p]];
		if (S.umis1) S.umis1[p] = V.umis[a[p]];
		if (S.umis2) S.umis2[p] = V.umis[b[p]];
		if (S.edit_distance) S.edit_distance[p] = ed[p];
	}
	S.ms_sampler = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The evaluation in three steps, so that the shards of a run can share the pairs of one sample (shard_validation.h): the common genes of
// every pair (cheap, the same on every shard), the chunk loop over a range of the pairs, the Poisson tail of a range.
bool dropest_ctx::validation_common_genes(const ValidationView &V, const std::vector<u32> &a, const std::vector<u32> &b, ValidationPairs &P) {
	using namespace dropest;
	const u32 NP = u32(a.size());
	P.cnt.assign(NP, 0);
	if (!NP || !V.n_mol || !ptab.ready) return false;
	P.d_pb.alloc(NP); P.d_pc.alloc(NP); P.d_cnt.alloc(NP); P.d_inter.alloc(NP); P.d_pr.alloc(NP);
	upload(P.d_pb.p, a.data(), size_t(NP) * 4);
	upload(P.d_pc.p, b.data(), size_t(NP) * 4);
	hipLaunchKernelGGL(common_genes_kernel<false>, dim3(div_up(NP, 256)), dim3(256), 0, stream, P.d_pb.p, P.d_pc.p, NP, V.cell_cg_begin.p, V.cell_cg_count.p,
	                   V.cg_key.p, V.cg_mol_begin.p, V.gene_none, ptab.adj.p, P.d_cnt.p, nullptr, nullptr);
	HIP_CHECK(hipGetLastError());
	fetch(P.cnt.data(), P.d_cnt.p, size_t(NP) * 4);
	return true;
}

// pairs [q0, q1) of P: inter / expected are the arrays of ALL pairs; returns the number of chunks
dropest::u32 dropest_ctx::validation_evaluate_range(const ValidationView &V, const dropest_validation_opts &opts, ValidationPairs &P, u32 q0, u32 q1, u32 *inter,
                                                    double *expected) {
	using namespace dropest;
	const PoissonSource src{V.cell_cg_begin.p, V.cell_cg_count.p, V.cg_key.p, V.cg_mol_begin.p, V.gene_none};
	const std::vector<u32> &cnt = P.cnt;
	uint64_t budget = opts.max_keys_per_chunk;
	if (!budget) {   // a key costs about 64 bytes along the chain (keys, sort ping-pong with values, distinct keys)
		size_t free_b = 0, total_b = 0;
		HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
		budget = std::max<uint64_t>(uint64_t(1) << 16, free_b / 2 / 64);
	}
	budget = std::min<uint64_t>(budget, uint64_t(1) << 31);
	const int low_bits = V.gene_bits + V.umi_bits;
	const u64 low_mask = low_bits >= 64 ? ~0ull : ((1ull << low_bits) - 1ull);
	u32 chunks = 0;
	for (u32 p0 = q0; p0 < q1;) {
		u32 p1 = p0;
		uint64_t keys = 0;
		while (p1 < q1 && (p1 == p0 || keys + cnt[p1] <= budget)) keys += cnt[p1++];
		const u32 np = p1 - p0;
		hipLaunchKernelGGL(pair_ranges_kernel, dim3(div_up(np, 256)), dim3(256), 0, stream, P.d_pb.p + p0, P.d_pc.p + p0, np, src.cell_cg_begin, src.cell_cg_count,
		                   src.cg_mol_begin, P.d_pr.p);
		HIP_CHECK(hipGetLastError());
		timed("umig_intersect", double(np) * 64, [&] {
			hipLaunchKernelGGL(umig_intersect_kernel, dim3(np), dim3(256), 0, stream, P.d_pr.p, np, V.mol_key.p, V.mol_key.p, low_mask, V.umi_bits,
			                   V.gene_none, P.d_inter.p);
		});
		fetch(inter + p0, P.d_inter.p, size_t(np) * 4);
		if (keys) poisson_expected_pairs(src, P.d_pb.p + p0, P.d_pc.p + p0, np, cnt.data() + p0, expected + p0);
		++chunks;
		p0 = p1;
	}
	return chunks;
}

// PoissonTargetEstimator::estimate_intersection_prob (:67-94): an empty intersection gives -1 and 1
void dropest_ctx::validation_tail(size_t n, const u32 *inter, double *expected, double *prob) {
	dropest::parallel_ranges(n, [&](size_t p0, size_t p1, unsigned) {
		for (size_t p = p0; p < p1; ++p) {
			if (inter[p] == 0) { expected[p] = -1.0; prob[p] = 1.0; }
			else prob[p] = poisson_upper_tail(long(inter[p]), expected[p]);
		}
	}, 4096, dropest::HostPool::MAX);
}

void dropest_ctx::validation_evaluate(const ValidationView &V, const dropest_validation_opts &opts, dropest_validation_sample &S, const std::vector<u32> &a,
                                      const std::vector<u32> &b) {
	using namespace dropest;
	const auto t0 = std::chrono::steady_clock::now();
	const u32 NP = u32(a.size());
	S.chunks = 0;
	if (!NP) return;
	std::vector<u32> inter(NP, 0);
	std::vector<double> expected(NP, 0.0), prob(NP, 1.0);
	ValidationPairs P;
	if (validation_common_genes(V, a, b, P)) S.chunks = validation_evaluate_range(V, opts, P, 0, NP, inter.data(), expected.data());
	validation_tail(NP, inter.data(), expected.data(), prob.data());
	for (u32 p = 0; p < NP; ++p) {
		if (S.intersection) S.intersection[p] = inter[p];
		if (S.expected) S.expected[p] = expected[p];
		if (S.probability) S.probability[p] = prob[p];
	}
	S.ms_evaluation = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

void dropest_ctx::run_merge_validation(const dropest_validation_opts *opts_in, dropest_validation_sample *samples, u32 n_samples) {
	using namespace dropest;
	if (is_shard_ctx) throw UnsupportedError("merge validation statistics are not computed by one context of a sharded run: this context belongs to a shard -- call dropest_shard_merge_validation_samples on every shard, or dropest_shard_group_merge_validation_samples");
	if (was_split) throw UnsupportedError("merge validation statistics are not computed by a split context: dropest_ctx_split handed this context's reads to shards -- call dropest_shard_group_merge_validation_samples on them");
	if (!initialized) throw InvalidError("You must initialize container");
	if (n_samples && !samples) throw InvalidError("null argument");
	const dropest_validation_opts opts = opts_in ? *opts_in : dropest_validation_opts{0, 0, 0};
	for (u32 s = 0; s < n_samples; ++s)
		if (samples[s].n_pairs > 0xFFFFFFF0ull) throw UnsupportedError("more than 2^32-16 pairs in one validation sample");
	HIP_CHECK(hipSetDevice(cfg.device));
	HostStage hs(this, "merge_validation");
	ValidationView V;
	validation_build_view(V);
	std::vector<u32> a, b;
	for (u32 s = 0; s < n_samples; ++s) {
		dropest_validation_sample &S = samples[s];
		S.ms_view = V.ms; S.ms_sampler = S.ms_evaluation = 0; S.chunks = 0;
		validation_sample(V, opts, S, a, b);
		validation_evaluate(V, opts, S, a, b);
	}
	collect_timings();
}
