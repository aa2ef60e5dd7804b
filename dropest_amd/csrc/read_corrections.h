// read_corrections.h -- per-read corrected cell barcode and UMI, `dropest -F` (BamController::write_filtered_bam_files ->
// FilteringBamProcessor::write_alignment, Estimation/BamProcessing/FilteringBamProcessor.cpp:14-40, :61-96), on the state the container is
// in NOW.  Device part: k_readfix.h.  Included by dropest_amd.hip.
//
//   targets   Gene::merge_targets() (Gene.cpp:54-57), kept when dropest_set_save_umi_merge_targets is on: every (source, target) pair a UMI
//             merge applies -- the two strategies (umi_merge_host.h, umi_directional_host.h; the groups -u decides on the device are read back
//             from the re-keyed molecule table before it is folded) and dropest_merge_umis (mutate_host.h) -- is logged as (cell, gene,
//             source, target) in the order it was applied.  umi_merge_target_rows() orders the log by (cell, gene, source) and keeps the LAST
//             row of each source: the reference's `_merge_targets[source] = target`.  The rows stay with the cell they were made in
//             (Gene::merge(const Gene &) copies no targets, Gene.cpp:26-36).
//   kept      filtered_cells() and their ranks; a cell the barcode merge folded takes its target's rank (merge_targets()[b],
//             FilteringBamProcessor.cpp:30-37; pairs merged by hand through dropest_merge_cells are not the strategy's and do not count).
//   molecules as the view of merge validation (validation.h): the molecule table's rows of the kept cells that bear a gene and whose
//             (cell, gene) group no UMI merge has rewritten, plus the rows of umi_overrides for the rewritten groups, under keys rank | gene |
//             UMI field, sorted.  An override UMI the field cannot hold (a random fill of another length) is left out: no read carries it.
//   sources   the target rows of the kept cells under the same keys, sorted with their row index as the value, the targets gathered behind.
#pragma once

#include "k_readfix.h"

void dropest_ctx::record_umi_target(u32 cell, u32 gene, u64 source, u64 target) {
	if (!save_umi_targets || source == target) return;
	umi_targets.push_back(UmiTargetRow{cell, gene, source, target});
	umi_targets_ordered = false;
}

// -u decided these groups on the device: keys_new[i] is where molecule row i of mol_key goes (n_changed of them moved)
void dropest_ctx::record_rekeyed_molecules(const u64 *keys_new, u32 n_changed) {
	using namespace dropest;
	if (!save_umi_targets || !n_changed || !n_mol) return;
	DevBuf<u64> d_old, d_new;
	d_old.alloc(n_changed); d_new.alloc(n_changed);
	scalars.ensure(16);
	HIP_CHECK(hipMemsetAsync(scalars.p + 8, 0, 4, stream));
	hipLaunchKernelGGL(umi_rekeyed_rows_kernel, dim3(div_up(n_mol, 256)), dim3(256), 0, stream, mol_key.p, keys_new, n_mol, n_changed, d_old.p, d_new.p,
	                   scalars.p + 8);
	HIP_CHECK(hipGetLastError());
	u32 got = 0;
	fetch(&got, scalars.p + 8, 4);
	if (got > n_changed) throw InvalidError("internal: more re-keyed molecules than the UMI merge counted");
	n_changed = got;
	std::vector<u64> ko(n_changed), kn(n_changed);
	fetch(ko.data(), d_old.p, size_t(n_changed) * 8);
	fetch(kn.data(), d_new.p, size_t(n_changed) * 8);
	const KeyLayout &L = layout;
	const u64 umask = L.umi_bits ? ((1ull << L.umi_bits) - 1ull) : 0ull;
	for (u32 i = 0; i < n_changed; ++i) {
		const u64 cg = ko[i] >> L.umi_bits;
		record_umi_target(u32(cg >> L.gene_bits), u32(cg & L.gene_none), unmap_umi(ko[i] & umask), unmap_umi(kn[i] & umask));
	}
}

const std::vector<dropest_ctx::UmiTargetRow> &dropest_ctx::umi_merge_target_rows() {
	if (umi_targets_ordered) return umi_targets;
	auto before = [](const UmiTargetRow &a, const UmiTargetRow &b) {
		if (a.cell != b.cell) return a.cell < b.cell;
		if (a.gene != b.gene) return a.gene < b.gene;
		return a.source < b.source;
	};
	std::stable_sort(umi_targets.begin(), umi_targets.end(), before);
	size_t out = 0;
	for (size_t i = 0; i < umi_targets.size(); ++i) {
		const bool last = i + 1 == umi_targets.size() || before(umi_targets[i], umi_targets[i + 1]);
		if (last) umi_targets[out++] = umi_targets[i];
	}
	umi_targets.resize(out);
	umi_targets_ordered = true;
	return umi_targets;
}

void dropest_ctx::build_read_corrections() {
	using namespace dropest;
	if (is_shard_ctx) throw UnsupportedError("read corrections are not computed by one context of a sharded run: this context belongs to a shard -- call dropest_shard_read_corrections on every shard, or dropest_shard_group_read_corrections");
	if (was_split) throw UnsupportedError("read corrections are not computed by a split context: dropest_ctx_split handed this context's reads to shards -- call dropest_shard_group_read_corrections on them");
	if (!initialized) throw InvalidError("You must initialize container");
	if (umi_dict_on) throw UnsupportedError("read corrections are not computed in UMI-dictionary mode: the keys carry UMI ranks, not UMI codes");
	ReadCorrections &R = corrections;
	if (R.valid) return;
	HostStage hs(this, "read_corrections");
	need_columns();
	const KeyLayout &L = layout;
	const u32 n = u32(n_reads);
	R.n = n;
	for (uint64_t &c : R.counts) c = 0;
	R.verdict.ensure(std::max<u32>(n, 1)); R.cell.ensure(std::max<u32>(n, 1)); R.umi.ensure(std::max<u32>(n, 1));
	if (!n) { R.valid = true; return; }

	// the kept cells and every cell's rank among them
	const std::vector<uint64_t> kept = filtered_cells();
	const u32 F = u32(kept.size());
	std::vector<u32> rank(n_cells, RF_NONE), kept_id(std::max<u32>(F, 1), 0);
	for (u32 i = 0; i < F; ++i) { rank[kept[i]] = i; kept_id[i] = u32(kept[i]); }
	const int rank_bits = std::max(1, bit_length(uint64_t(F ? F - 1 : 0)));
	const int total_bits = rank_bits + L.gene_bits + L.umi_bits;
	if (total_bits > 64) throw UnsupportedError("read corrections: the key (cell rank, gene, UMI) is wider than 64 bits");
	const u64 total_mask = total_bits >= 64 ? ~0ull : ((1ull << total_bits) - 1ull);
	const int cell_shift = L.gene_bits + L.umi_bits;
	DevBuf<u32> d_rank, d_kept, d_mb, d_me, d_sb, d_se;
	d_rank.alloc(n_cells); d_kept.alloc(F); d_mb.alloc(F); d_me.alloc(F); d_sb.alloc(F); d_se.alloc(F);
	for (DevBuf<u32> *b : {&d_mb, &d_me, &d_sb, &d_se}) HIP_CHECK(hipMemsetAsync(b->p, 0, std::max<size_t>(F, 1) * 4, stream));
	upload(d_kept.p, kept_id.data(), kept_id.size() * 4);

	// their molecules as they are now: the table's rows, the rewritten groups from the host map
	u32 n_keys = 0;
	const u64 *mol_sorted = nullptr;
	if (F && n_mol) {
		std::vector<u64> rewritten, extra;
		for (auto const &kv : umi_overrides) {
			const u32 cell = u32(kv.first >> L.gene_bits);
			if (cell >= n_cells || rank[cell] == RF_NONE) continue;
			rewritten.push_back(kv.first);
			if ((kv.first & L.gene_none) == L.gene_none) continue;
			for (const UmiOverride &o : kv.second) {
				u64 field = 0;
				if (map_umi(o.umi, field)) extra.push_back((((u64(rank[cell]) << L.gene_bits) | (kv.first & L.gene_none)) << L.umi_bits) | field);
			}
		}
		std::sort(rewritten.begin(), rewritten.end());
		const size_t cap = size_t(n_mol) + extra.size();
		if (cap >= 0xFFFFFFF0ull) throw UnsupportedError("read corrections: too many molecules");
		keys_a.ensure(cap); keys_b.ensure(cap); vals_a.ensure(1); vals_b.ensure(1);
		remap.ensure(std::max<u32>(n_cells, 1));
		upload(remap.p, rank.data(), size_t(n_cells) * 4);
		DevBuf<u64> d_rewritten; d_rewritten.alloc(std::max<size_t>(rewritten.size(), 1));
		upload(d_rewritten.p, rewritten.data(), rewritten.size() * 8);
		scalars.ensure(16);
		HIP_CHECK(hipMemsetAsync(scalars.p, 0, 16, stream));
		hipLaunchKernelGGL(validation_view_keys_kernel, dim3(div_up(n_mol, 256)), dim3(256), 0, stream, mol_key.p, n_mol, L.umi_bits, L.gene_bits, L.gene_none,
		                   L.umi_bits, remap.p, d_rewritten.p, u32(rewritten.size()), keys_a.p, scalars.p);
		HIP_CHECK(hipGetLastError());
		u32 kept_rows = 0;
		fetch(&kept_rows, scalars.p, 4);
		upload(keys_a.p + kept_rows, extra.data(), extra.size() * 8);
		n_keys = kept_rows + u32(extra.size());
		u64 *k = keys_a.p, *k_alt = keys_b.p;
		u32 *v = vals_a.p, *v_alt = vals_b.p;
		radix_sort(k, v, k_alt, v_alt, n_keys, total_mask, 0, "read_corrections:");
		mol_sorted = k;
		if (n_keys) hipLaunchKernelGGL(validation_cell_segments_kernel, dim3(div_up(n_keys, 256)), dim3(256), 0, stream, k, n_keys, cell_shift, F, d_mb.p, d_me.p);
		HIP_CHECK(hipGetLastError());
	}

	// the UMI merge targets of the kept cells
	u32 n_src = 0;
	DevBuf<u64> s_key, s_key_alt, s_tgt_in, s_tgt;
	DevBuf<u32> s_idx, s_idx_alt;
	const u64 *src_sorted = nullptr;
	if (F) {
		std::vector<u64> sk, st;
		for (const UmiTargetRow &r : umi_merge_target_rows()) {
			u64 field = 0;
			if (r.cell >= n_cells || rank[r.cell] == RF_NONE || r.gene >= L.gene_none || !map_umi(r.source, field)) continue;
			sk.push_back((((u64(rank[r.cell]) << L.gene_bits) | r.gene) << L.umi_bits) | field);
			st.push_back(r.target);
		}
		if (sk.size() >= 0xFFFFFFF0ull) throw UnsupportedError("read corrections: too many UMI merge targets");
		n_src = u32(sk.size());
		if (n_src) {
			s_key.alloc(n_src); s_key_alt.alloc(n_src); s_idx.alloc(n_src); s_idx_alt.alloc(n_src); s_tgt_in.alloc(n_src); s_tgt.alloc(n_src);
			upload(s_key.p, sk.data(), size_t(n_src) * 8);
			upload(s_tgt_in.p, st.data(), size_t(n_src) * 8);
			hipLaunchKernelGGL(iota_kernel, dim3(div_up(n_src, 256)), dim3(256), 0, stream, s_idx.p, n_src);
			u64 *k = s_key.p, *k_alt = s_key_alt.p;
			u32 *v = s_idx.p, *v_alt = s_idx_alt.p;
			radix_sort(k, v, k_alt, v_alt, n_src, total_mask, 4, "read_corrections:");
			hipLaunchKernelGGL(gather_u64_kernel, dim3(div_up(n_src, 256)), dim3(256), 0, stream, s_tgt_in.p, v, n_src, s_tgt.p);
			hipLaunchKernelGGL(validation_cell_segments_kernel, dim3(div_up(n_src, 256)), dim3(256), 0, stream, k, n_src, cell_shift, F, d_sb.p, d_se.p);
			HIP_CHECK(hipGetLastError());
			src_sorted = k;
		}
	}

	// merged cells answer with their target's rank
	for (auto const &pr : merge_pairs) {
		if (explicit_sources.count(u32(pr.first))) continue;
		if (pr.first < n_cells && pr.second < n_cells) rank[pr.first] = rank[pr.second];
	}
	upload(d_rank.p, rank.data(), size_t(n_cells) * 4);

	DevBuf<u64> d_counts; d_counts.alloc(5);
	HIP_CHECK(hipMemsetAsync(d_counts.p, 0, 5 * 8, stream));
	ReadFixArgs a{};
	a.cb = d_cb; a.umi = d_umi; a.gene = d_gene; a.n = n; a.table = table;
	a.cell_rank = d_rank.p; a.kept_cell = d_kept.p;
	a.mol_key = mol_sorted ? mol_sorted : keys_a.p; a.mol_begin = d_mb.p; a.mol_end = d_me.p;
	a.src_key = src_sorted; a.src_target = s_tgt.p; a.src_begin = d_sb.p; a.src_end = d_se.p; a.n_src = n_src;
	a.gene_bits = L.gene_bits; a.umi_bits = L.umi_bits; a.gene_none = L.gene_none; a.umi_strip_mask = L.umi_strip_mask; a.umi_escape_base = L.umi_escape_base;
	a.verdict = R.verdict.p; a.cell = R.cell.p; a.umi_out = R.umi.p; a.counts = d_counts.p;
	static const u32 grid_max = resident_grid(read_corrections_kernel<RfOwnCells>, 256, ~0u);
	// algorithmic bytes: 20 in and 13 out per read, one 16-byte table slot, the rank word (the searches' dependent loads are not counted)
	timed("read_corrections", double(n) * (20 + 13 + 16 + 4), [&] {
		hipLaunchKernelGGL(read_corrections_kernel<RfOwnCells>, dim3(std::min<u32>(div_up(n, 256), grid_max)), dim3(256), 0, stream, a);
	});
	fetch(R.counts, d_counts.p, 5 * 8);   // (waits: the local buffers above outlive the kernel)
	R.valid = true;
	collect_timings();
}
