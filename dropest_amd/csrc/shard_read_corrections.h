// shard_read_corrections.h -- per-read corrected cell barcode and UMI (`dropest -F`, the DECISIONS: read_corrections.h, k_readfix.h) for the
// shards of a sharded or split run (included by shard_run.h).  The file writer on top of them: host/bam_device.cpp (FilteredPass's second shape,
// behind BamController::set_sharded_filtered_output), which feeds every window the pieces of these arrays that the shards' ranges cut out of it.
//
// After a step a shard still holds its contiguous range of the stream (r_cb / r_umi / r_gene, n_res reads from first_ordinal on), the global
// table G and cm's column order.  A read's barcode is usually owned by another shard, and the cell it was merged into by a third, so:
//   table     every shard lists (barcode, column of cm) for ITS OWN cells whose final merge target is a column: its filtered cells, and its
//             cells that the strategy's barcode merge folded into a filtered cell wherever that lives (a cell folded into a cell that is not
//             kept is left out; a step applies no pairs by hand).  Counts through the host, ONE gather_dev of 16-byte pairs, and
//             bc_insert_kernel builds the same open-addressed table on every shard: capacity = a power of two of at least twice the
//             entries, 16 bytes a slot, global memory.
//   molecules global_molecule_keys (shard_validation.h), the view -S uses, without the override UMIs that the field cannot hold: the sorted
//             array column | gene | UMI field of ALL filtered cells on every shard, and the rows of every column.
//   sources   Gene::merge_targets() of this shard's filtered cells (dropest_set_save_umi_merge_targets on dropest_shard_ctx, before the step)
//             under the same keys, sorted here, gathered and placed by column the same way, the target codes travelling behind them.
//   kernel    read_corrections_kernel<RfColumnTable> over the resident range only: one probe of the table gives the column, the rest is the
//             one context's code with rank = column.
// Memory on EVERY GPU while the call runs: 8 bytes per molecule of a filtered cell (twice that while the gathered blocks are placed), as -S
// pays, plus 16 bytes x the table's capacity; 13 bytes per resident read stay until the next step.
// Refusals come from gathered data, so that all shards throw alike and the group stays usable (shard_validation.h's rule): before a step,
// UMI-dictionary mode, a key wider than 64 bits, 2^32 - 16 or more rows.  The gathers have only ever run between shards of one GPU.
#pragma once

// the table of `n` pairs (device) in `table`; returns BC_FLAG_* (0: fine).  Waits for the stream.
static dropest::u32 bc_table_build(const dropest::BcPair *d_pairs, dropest::u32 n, dropest::DevBuf<dropest::BcColSlot> &table, dropest::u32 &capacity, hipStream_t st) {
	using namespace dropest;
	capacity = 2;
	while (capacity < 2ull * n) capacity <<= 1;
	table.ensure(capacity);
	DevBuf<u32> flags; flags.alloc(1);
	HIP_CHECK(hipMemsetAsync(table.p, 0, size_t(capacity) * sizeof(BcColSlot), st));
	HIP_CHECK(hipMemsetAsync(flags.p, 0, 4, st));
	if (n) hipLaunchKernelGGL(bc_insert_kernel, dim3(div_up(n, 256)), dim3(256), 0, st, d_pairs, n, table.p, capacity - 1, flags.p);
	HIP_CHECK(hipGetLastError());
	u32 got = 0;
	HIP_CHECK(hipMemcpyAsync(&got, flags.p, 4, hipMemcpyDeviceToHost, st));
	HIP_CHECK(stream_wait(st));
	return got;
}

void dropest_shard::build_read_corrections() {
	using namespace dropest;
	dropest_ctx &c = *ctx;
	ReadCorrections &R = corrections;
	if (R.valid) return;   // (every shard of the run computed it in the same call: nobody enters a collective here)
	// The first collective: where every shard stands, and the key fields of those that have reads of their own barcodes.
	struct Head { u64 stepped, dict, has_layout, gene_bits, umi_bits, gene_none, strip_mask, escape_base; };
	Head mine{stepped ? 1ull : 0ull, c.umi_dict_on ? 1ull : 0ull, 0, 0, 0, 0, 0, 0}, agreed{};
	if (stepped && c.initialized && c.n_reads) {
		const KeyLayout &L = c.layout;
		mine.has_layout = 1; mine.gene_bits = u64(L.gene_bits); mine.umi_bits = u64(L.umi_bits); mine.gene_none = L.gene_none;
		mine.strip_mask = L.umi_strip_mask; mine.escape_base = L.umi_escape_base;
	}
	{
		std::vector<Head> all(static_cast<size_t>(world));
		tr->gather_host(&mine, sizeof(Head), all.data());
		bool dict = false;
		for (const Head &h : all) {
			if (!h.stepped) throw InvalidError("You must initialize container: the read corrections of a sharded run follow a step of every shard");
			dict |= h.dict != 0;
		}
		if (dict) throw UnsupportedError("read corrections are not computed in UMI-dictionary mode: the keys carry UMI ranks, not UMI codes");
		for (const Head &h : all) {
			if (!h.has_layout) continue;
			if (agreed.has_layout && (agreed.gene_bits != h.gene_bits || agreed.umi_bits != h.umi_bits || agreed.strip_mask != h.strip_mask || agreed.escape_base != h.escape_base))
				throw InvalidError("internal: the shards keyed their molecules with different gene / UMI fields");
			agreed = h;
		}
	}
	HIP_CHECK(hipSetDevice(c.cfg.device));
	Phase whole(this, "read_corrections");
	const Mat &M = mat[0];
	if (M.col_row.size() != M.ncols) throw DeviceError("internal: the filtered matrix has no column table");
	const u32 F = u32(M.ncols);
	const u32 n = u32(n_res);
	R.n = n_res;
	for (uint64_t &x : R.counts) x = 0;
	R.verdict.ensure(std::max<u32>(n, 1)); R.column.ensure(std::max<u32>(n, 1)); R.umi.ensure(std::max<u32>(n, 1));

	// barcode -> column, the same table on every shard
	DevBuf<BcColSlot> table;
	u32 capacity = 0;
	{
		Phase ph(this, "read_corrections:table");
		std::vector<BcPair> own;
		std::unordered_map<u64, u32> column_of;
		column_of.reserve(size_t(F) * 2);
		for (u32 j = 0; j < F; ++j) {
			const GRow &r = G[M.col_row[j]];
			column_of.emplace(r.barcode, j);
			if (int(r.rank) == rank) own.push_back(BcPair{r.barcode, j, 0});
		}
		name_merged_pairs();
		for (auto const &pr : merged_barcodes) {
			if (int(mix64(pr.first) % u64(world)) != rank) continue;
			auto it = column_of.find(pr.second);
			if (it != column_of.end()) own.push_back(BcPair{pr.first, it->second, 0});
		}
		uint64_t my_n = own.size();
		std::vector<uint64_t> counts(static_cast<size_t>(world));
		tr->gather_host(&my_n, 8, counts.data());
		std::vector<size_t> off(static_cast<size_t>(world)), bytes(static_cast<size_t>(world));
		uint64_t total = 0;
		for (int p = 0; p < world; ++p) { off[size_t(p)] = size_t(total) * sizeof(BcPair); bytes[size_t(p)] = size_t(counts[size_t(p)]) * sizeof(BcPair); total += counts[size_t(p)]; }
		if (total >= (1ull << 30)) throw UnsupportedError("read corrections: 2^30 or more kept and merged cells");
		DevBuf<BcPair> d_own, d_all;
		d_own.alloc(std::max<size_t>(own.size(), 1)); d_all.alloc(std::max<size_t>(size_t(total), 1));
		c.upload(d_own.p, own.data(), own.size() * sizeof(BcPair));
		tr->gather_dev(d_own.p, d_all.p, off.data(), bytes.data(), c.stream);
		phases["read_corrections:table"].bytes += double(total - my_n) * sizeof(BcPair);
		const u32 flags = bc_table_build(d_all.p, u32(total), table, capacity, c.stream);
		// (every shard built its table from the same pairs: all of them see the same flags)
		if (flags & BC_FLAG_DUPLICATE) throw InvalidError("internal: a barcode came to the column table with two different columns");
		if (flags) throw InvalidError("internal: the column table could not take every barcode");
	}

	// the molecules of all filtered cells, and the UMI merge targets of all of them, by column
	GlobalKeys mol, src;
	{
		Phase ph(this, "read_corrections:view");
		global_molecule_keys(mol, false, "read corrections", "read_corrections:keys", "read_corrections:gather_place");
		if (mol.any_rows && (!agreed.has_layout || u64(mol.gene_bits) != agreed.gene_bits || u64(mol.umi_bits) != agreed.umi_bits))
			throw InvalidError("internal: the molecule view was keyed with other fields than the shards agreed on");
		if (mol.any_rows) {   // (agreed by all: a collective inside)
			std::unique_ptr<Phase> ph_keys(new Phase(this, "read_corrections:source_keys"));
			const KeyLayout &L = c.layout;
			std::vector<u32> pos(std::max<u32>(c.n_cells, 1), 0xFFFFFFFFu);
			for (u32 j = 0; j < F; ++j) {
				const GRow &r = G[M.col_row[j]];
				if (int(r.rank) == rank && r.local_id < c.n_cells) pos[r.local_id] = j;
			}
			std::vector<u64> sk, st;
			if (c.initialized)
				for (const dropest_ctx::UmiTargetRow &r : c.umi_merge_target_rows()) {
					u64 field = 0;
					if (r.cell >= c.n_cells || pos[r.cell] == 0xFFFFFFFFu || r.gene >= L.gene_none || !c.map_umi(r.source, field)) continue;
					sk.push_back((((u64(pos[r.cell]) << L.gene_bits) | r.gene) << L.umi_bits) | field);
					st.push_back(r.target);
				}
			if (sk.size() >= 0xFFFFFFF0ull) throw DeviceError("read corrections: too many UMI merge targets on one shard");
			const u32 n_src = u32(sk.size());
			const int total_bits = std::max(1, bit_length(uint64_t(F ? F - 1 : 0))) + mol.gene_bits + mol.umi_bits;   // (<= 64: the view was built)
			DevBuf<u64> s_key, s_key_alt, s_tgt_in, s_tgt;
			DevBuf<u32> s_idx, s_idx_alt;
			const u64 *k_sorted = nullptr;
			if (n_src) {
				s_key.alloc(n_src); s_key_alt.alloc(n_src); s_idx.alloc(n_src); s_idx_alt.alloc(n_src); s_tgt_in.alloc(n_src); s_tgt.alloc(n_src);
				c.upload(s_key.p, sk.data(), size_t(n_src) * 8);
				c.upload(s_tgt_in.p, st.data(), size_t(n_src) * 8);
				hipLaunchKernelGGL(iota_kernel, dim3(div_up(n_src, 256)), dim3(256), 0, c.stream, s_idx.p, n_src);
				u64 *k = s_key.p, *k_alt = s_key_alt.p;
				u32 *v = s_idx.p, *v_alt = s_idx_alt.p;
				c.radix_sort(k, v, k_alt, v_alt, n_src, total_bits >= 64 ? ~0ull : ((1ull << total_bits) - 1ull), 4, "read_corrections:");
				hipLaunchKernelGGL(gather_u64_kernel, dim3(div_up(n_src, 256)), dim3(256), 0, c.stream, s_tgt_in.p, v, n_src, s_tgt.p);
				HIP_CHECK(hipGetLastError());
				k_sorted = k;
			}
			gather_place_keys(k_sorted, s_tgt.p, true, n_src, mol.gene_bits + mol.umi_bits, F, "read corrections", "read_corrections:source_gather_place", ph_keys, src);
		}
	}
	mol.begin.resize(F, 0); mol.count.resize(F, 0); src.begin.resize(F, 0); src.count.resize(F, 0);
	DevBuf<u32> ranges; ranges.alloc(std::max<size_t>(size_t(F) * 4, 1));
	{
		std::vector<u32> h(std::max<size_t>(size_t(F) * 4, 1), 0);
		for (u32 j = 0; j < F; ++j) {
			h[j] = mol.begin[j]; h[size_t(F) + j] = mol.begin[j] + mol.count[j];
			h[2 * size_t(F) + j] = src.begin[j]; h[3 * size_t(F) + j] = src.begin[j] + src.count[j];
		}
		c.upload(ranges.p, h.data(), h.size() * 4);
	}

	if (n) {
		Phase ph(this, "read_corrections:kernel");
		DevBuf<u64> d_counts; d_counts.alloc(5);
		HIP_CHECK(hipMemsetAsync(d_counts.p, 0, 5 * 8, c.stream));
		ReadFixArgs a{};
		a.cb = r_cb; a.umi = r_umi; a.gene = r_gene; a.n = n;
		a.mol_key = mol.key.p; a.mol_begin = ranges.p; a.mol_end = ranges.p + F;
		a.src_key = src.key.p; a.src_target = src.val.p; a.src_begin = ranges.p + 2 * size_t(F); a.src_end = ranges.p + 3 * size_t(F); a.n_src = src.n;
		a.gene_bits = int(agreed.gene_bits); a.umi_bits = int(agreed.umi_bits); a.gene_none = agreed.gene_none; a.umi_strip_mask = agreed.strip_mask; a.umi_escape_base = agreed.escape_base;
		a.verdict = R.verdict.p; a.cell = R.column.p; a.umi_out = R.umi.p; a.counts = d_counts.p;
		a.bc_slots = table.p; a.bc_mask = capacity - 1;
		static const u32 grid_max = resident_grid(read_corrections_kernel<RfColumnTable>, 256, ~0u);
		// algorithmic bytes: 20 in and 13 out per read, one 16-byte table slot (the searches' dependent loads are not counted)
		c.timed("read_corrections_shard", double(n) * (20 + 13 + 16), [&] {
			hipLaunchKernelGGL(read_corrections_kernel<RfColumnTable>, dim3(std::min<u32>(div_up(n, 256), grid_max)), dim3(256), 0, c.stream, a);
		});
		HIP_CHECK(hipGetLastError());
		c.fetch(R.counts, d_counts.p, 5 * 8);   // (waits: the local buffers above outlive the kernel)
	}
	R.valid = true;
	c.collect_timings();
}

// a shard's failure other than a refusal all shards reach alike must not leave its peers waiting
template <class F>
static void shard_collective(dropest_shard *s, F &&f) {
	try { f(); }
	catch (const InvalidError &) { throw; }
	catch (const UnsupportedError &) { throw; }
	catch (...) {
		if (auto *lt = dynamic_cast<dropest::LocalTransport *>(s->tr.get())) lt->hub->fail();
		if (auto *rt = dynamic_cast<dropest::RcclTransport *>(s->tr.get())) if (rt->mailbox) rt->mailbox->fail();
		throw;
	}
}

extern "C" {

dropest_status dropest_shard_read_corrections(dropest_shard *s, uint64_t *n, uint64_t *first_ordinal, const uint8_t **d_verdict, const uint32_t **d_column, const uint64_t **d_umi) {
	return guarded([&] {
		if (!s) throw InvalidError("null shard");
		shard_collective(s, [&] { s->build_read_corrections(); });
		const dropest_shard::ReadCorrections &R = s->corrections;
		if (n) *n = R.n;
		if (first_ordinal) *first_ordinal = s->first_ordinal;
		if (d_verdict) *d_verdict = R.verdict.p;
		if (d_column) *d_column = R.column.p;
		if (d_umi) *d_umi = reinterpret_cast<const uint64_t *>(R.umi.p);
	});
}

dropest_status dropest_shard_group_read_corrections(dropest_shard *const *shards, int32_t n) {
	return guarded([&] {
		if (!shards || n < 1) throw InvalidError("null argument");
		for (int i = 0; i < n; ++i) if (!shards[i]) throw InvalidError("null shard");
		bool all_valid = true;
		for (int i = 0; i < n; ++i) all_valid &= shards[i]->corrections.valid;
		if (all_valid) return;
		std::vector<dropest_status> rc(size_t(n), DROPEST_OK);
		std::vector<std::string> msg(static_cast<size_t>(n));
		std::vector<std::thread> pool;
		for (int i = 0; i < n; ++i)
			pool.emplace_back([&, i] {
				rc[size_t(i)] = dropest_shard_read_corrections(shards[i], nullptr, nullptr, nullptr, nullptr, nullptr);
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

dropest_status dropest_shard_group_read_corrections_host(dropest_shard *const *shards, int32_t n, uint64_t first, uint64_t count, uint8_t *verdict, uint32_t *column, uint64_t *umi) {
	const dropest_status st = dropest_shard_group_read_corrections(shards, n);
	if (st != DROPEST_OK) return st;
	return guarded([&] {
		uint64_t total = 0;
		for (int i = 0; i < n; ++i) total += shards[i]->corrections.n;
		if (first > total || count > total - first) throw RangeError("read ordinal out of range");
		// the stream = the shards' ranges one behind the other (they ascend with the rank)
		uint64_t base = 0;
		for (int i = 0; i < n; ++i) {
			dropest_shard &s = *shards[i];
			const dropest_shard::ReadCorrections &R = s.corrections;
			const uint64_t lo = std::max(first, base), hi = std::min(first + count, base + R.n);
			if (lo < hi) {
				HIP_CHECK(hipSetDevice(s.ctx->cfg.device));
				const uint64_t at = lo - base, to = lo - first, m = hi - lo;
				if (verdict) s.ctx->fetch(verdict + to, R.verdict.p + at, size_t(m));
				if (column) s.ctx->fetch(column + to, R.column.p + at, size_t(m) * 4);
				if (umi) s.ctx->fetch(umi + to, R.umi.p + at, size_t(m) * 8);
			}
			base += R.n;
		}
	});
}

dropest_status dropest_shard_group_read_correction_counts(dropest_shard *const *shards, int32_t n, uint64_t out[5]) {
	const dropest_status st = dropest_shard_group_read_corrections(shards, n);
	if (st != DROPEST_OK) return st;
	return guarded([&] {
		if (!out) throw InvalidError("null argument");
		for (int k = 0; k < 5; ++k) { out[k] = 0; for (int i = 0; i < n; ++i) out[k] += shards[i]->corrections.counts[k]; }
	});
}

dropest_status dropest_shard_filtered_barcodes_device(dropest_shard *s, uint64_t *n, const uint64_t **d_codes) {
	return guarded([&] {
		if (!s || !n || !d_codes) throw InvalidError("null argument");
		if (!s->stepped) throw InvalidError("You must initialize container");
		const dropest_shard::Mat &M = s->mat[0];
		if (M.col_row.size() != M.ncols) throw DeviceError("internal: the filtered matrix has no column table");
		HIP_CHECK(hipSetDevice(s->ctx->cfg.device));
		if (!s->col_barcode_valid) {
			std::vector<dropest::u64> codes(M.ncols);
			for (size_t j = 0; j < codes.size(); ++j) codes[j] = s->G[M.col_row[j]].barcode;
			s->d_col_barcode.ensure(std::max<size_t>(codes.size(), 1));
			s->ctx->upload(s->d_col_barcode.p, codes.data(), codes.size() * 8);
			s->col_barcode_valid = true;
		}
		*n = M.ncols;
		*d_codes = reinterpret_cast<const uint64_t *>(s->d_col_barcode.p);
	});
}

// Test hook (tests/test_gpu_read_corrections_sharded.py): the column table built from `n` pairs and probed with `n_probe` barcodes on `device`.
// probe_column[i] = the column of probe[i] (0xFFFFFFFF: absent), *capacity = the table's slots, *flags = what bc_insert_kernel raised.
int dropest_test_column_table(int device, const uint64_t *barcode, const uint32_t *column, uint32_t n, const uint64_t *probe, uint32_t n_probe, uint32_t *probe_column,
                              uint32_t *capacity, uint32_t *flags) {
	using namespace dropest;
	if (!capacity || !flags || (n && (!barcode || !column)) || (n_probe && (!probe || !probe_column)) || n >= (1u << 30)) return -1;
	const dropest_status st = guarded([&] {
		HIP_CHECK(hipSetDevice(device));
		std::vector<BcPair> pairs(n);
		for (u32 i = 0; i < n; ++i) pairs[i] = BcPair{barcode[i], column[i], 0};
		DevBuf<BcPair> d_pairs; d_pairs.alloc(std::max<u32>(n, 1));
		DevBuf<BcColSlot> table;
		DevBuf<u64> d_probe; d_probe.alloc(std::max<u32>(n_probe, 1));
		DevBuf<u32> d_out; d_out.alloc(std::max<u32>(n_probe, 1));
		if (n) HIP_CHECK(hipMemcpy(d_pairs.p, pairs.data(), size_t(n) * sizeof(BcPair), hipMemcpyHostToDevice));
		*flags = bc_table_build(d_pairs.p, n, table, *capacity, nullptr);
		if (n_probe) {
			HIP_CHECK(hipMemcpy(d_probe.p, probe, size_t(n_probe) * 8, hipMemcpyHostToDevice));
			hipLaunchKernelGGL(bc_probe_kernel, dim3(div_up(n_probe, 256)), dim3(256), 0, nullptr, d_probe.p, n_probe, table.p, *capacity - 1, d_out.p);
			HIP_CHECK(hipGetLastError());
			HIP_CHECK(hipMemcpy(probe_column, d_out.p, size_t(n_probe) * 4, hipMemcpyDeviceToHost));
		}
	});
	return st == DROPEST_OK ? 0 : -1;
}

}  // extern "C"
