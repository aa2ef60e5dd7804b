// shard_matrix.h -- the matrix end of a sharded step (included by shard_run.h; dropest_shard::step lists the steps): the global column
// order, the node-shared result buffer and its layout, the placing of this shard's columns (kernels in k_shard.h), cm_raw planned on the
// device, the 32-bit slots and the byte form's lists.
#pragma once

// 8. one matrix: global column order (identical on every shard), this shard's columns emitted on the device and written to
// their places in the node-shared host buffer
void dropest_shard::assemble_matrix(bool filtered_m) {
	using namespace dropest;
	dropest_ctx &c = *ctx;
	const int slot = filtered_m ? 0 : 1;
	Mat &M = mat[slot];
	ctx->mat[slot].settle();   // (a straggler of the previous widening reads dec_begin / dec_end)
	dropest::DevBuf<u64> &d_desc = d_desc_m[slot];
	dropest::PinnedBuf<u64> &h_desc = h_desc_m[slot];
	std::vector<u32> sel;
	for (u32 i = 0; i < G.size(); ++i) if (!filtered_m || G[i].req_genes >= c.min_after) sel.push_back(i);
	std::vector<u32> order;
	{
		Phase ph(this, filtered_m ? "order:cm" : "order:cm_raw");
		order = order_rows(sel, !filtered_m);
		if (filtered_m && c.cfg.max_cells > 0 && size_t(c.cfg.max_cells) < order.size())   // -C: the largest max_cells cells (CellsDataContainer.cpp:269-273)
			order.erase(order.begin(), order.end() - c.cfg.max_cells);
	}
	Phase ph(this, filtered_m ? "matrix:cm" : "matrix:cm_raw");
	const size_t ncols = order.size();
	M.ncols = ncols; M.colptr.assign(ncols + 1, 0); M.col_barcode.resize(ncols);
	if (filtered_m) M.col_row = order;
	std::vector<u32> &col_cell = M.col_cell, &col_start = M.col_start;   // (members: their copies to the device are not waited for here)
	col_cell.clear(); col_start.clear();
	std::vector<u64> desc;
	uint64_t local_nnz = 0;
	for (size_t j = 0; j < ncols; ++j) {
		const GRow &r = G[order[j]];
		const u32 len = filtered_m ? r.req_genes : r.n_genes;
		M.col_barcode[j] = r.barcode;
		M.colptr[j + 1] = M.colptr[j] + len;
		if (int(r.rank) != rank) continue;
		col_cell.push_back(r.local_id); col_start.push_back(u32(local_nnz));
		desc.push_back(local_nnz); desc.push_back(M.colptr[j]); desc.push_back(len);
		local_nnz += len;
	}
	M.dec_begin.clear(); M.dec_end.clear();
	for (size_t k = 0; k < col_cell.size(); ++k) { M.dec_begin.push_back(u32(desc[3 * k + 1])); M.dec_end.push_back(u32(desc[3 * k + 1] + desc[3 * k + 2])); }
	M.nnz = M.colptr[ncols];
	if (M.nnz > 0xFFFFFFF0ull || local_nnz > 0xFFFFFFF0ull) throw UnsupportedError("count matrix with more than 2^32 non-zeros");
	M.colptr_p = M.colptr.data(); M.barcode_p = M.col_barcode.data();
	M.colptr32.resize(ncols + 1);
	for (size_t j = 0; j <= ncols; ++j) M.colptr32[j] = u32(M.colptr[j]);
	M.colptr32_p = M.colptr32.data();
	SharedLayout L;
	{ Phase p2(this, filtered_m ? "cm:open_shared" : "raw:open_shared"); L = open_shared(M, slot, 0); }
	const u32 nc = u32(col_cell.size());
	if (nc && local_nnz) {
		if (!L.slots) c.emit_columns_device(filtered_m, false, col_cell, col_start, local_nnz, false);   // (a slots step emits the byte form of the local matrix: place_columns)
		// (the same matrix assembled again inside one step -- the overflow fall-back -- or in the next step: the previous copy has left the
		// staging buffer by then in every run seen, but nothing said so: wait, it costs nothing on a drained stream)
		if (desc_in_flight[slot]) HIP_CHECK(stream_wait(c.stream));
		d_desc.ensure(desc.size()); h_desc.ensure(desc.size());
		std::memcpy(h_desc.p, desc.data(), desc.size() * 8);
		HIP_CHECK(hipMemcpyAsync(d_desc.p, h_desc.p, desc.size() * 8, hipMemcpyHostToDevice, c.stream));
		desc_in_flight[slot] = true;
	}
	Phase p3(this, filtered_m ? "cm:place" : "raw:place");
	place_columns(M, slot, filtered_m, L, d_desc.p, nc, local_nnz, nullptr, col_start.data());
}

// The node-shared host buffer of one matrix (collective: every shard takes the same decisions -- the gene ids are the agreed ones).
// [head_bytes of the caller][payload][byte form: one segment per shard].  Payload: 32-bit rows | values; 16-bit rows | values; byte form:
// deltas | values (each padded to 16 bytes).  A segment = 4 words (rows listed, values listed, 0, 0) + 4 arrays of list_cap words (row
// positions, rows, value positions, values); list_cap comes from the GLOBAL nnz: the same on every shard.
dropest_shard::SharedLayout dropest_shard::open_shared(Mat &M, int slot, size_t head_bytes) {
	using namespace dropest;
	dropest_ctx &c = *ctx;
	SharedLayout L{};
	L.bytes = byte_matrix && !wide_now[slot];
	L.narrow = !L.bytes && narrow_matrix && c.narrow_possible();
	L.base = (head_bytes + 15) & ~size_t(15);
	L.list_cap = u32(std::min<uint64_t>(byte_list_cap ? byte_list_cap : (1u << 20), (M.nnz + 15) & ~15ull));
	L.off_val = (size_t(M.nnz) + 15) & ~size_t(15); L.off_seg = 2 * L.off_val; L.seg_bytes = 16 + 16 * size_t(L.list_cap);
	// slots step: the buffer holds the 32-bit slots only -- rows | values, each padded to whole 64-byte lines (the widening stores whole
	// lines); every shard's bytes cross its link as the byte form of its LOCAL matrix and never stand in the shared buffer
	L.slots = L.bytes && slots_matrix;
	if (L.slots) L.bytes = false;
	L.off_slots = (L.base + 63) & ~size_t(63);   // (from the buffer's start: that is page-aligned)
	L.slots_stride = ((size_t(M.nnz) + 15) & ~size_t(15)) * 4;
	const size_t payload = L.slots ? L.off_slots - L.base + std::max<size_t>(2 * L.slots_stride, 64)   // (an empty matrix still gets a buffer: the transports map what they are asked for)
	                               : (L.bytes ? L.off_seg + L.seg_bytes * size_t(world) : std::max<size_t>(size_t(M.nnz), 1) * (L.narrow ? 4 : 8));
	ctx->mat[slot].settle();   // (a straggler of the previous step's widening may still be leaving: the buffer is about to be rewritten or replaced)
	L.host = static_cast<char *>(tr->shared_host(slot, L.base + payload, &L.dev));
	char *host = L.host + L.base;
	M.narrow = L.narrow; M.widened = false; M.ovf_pos.clear(); M.ovf_val.clear();
	M.bytes = L.bytes; M.lists_ready = false;
	M.rows = M.vals = nullptr; M.rows16 = M.vals16 = nullptr; M.delta8 = M.vals8 = nullptr;
	M.slots = L.slots; M.slot_rows = M.slot_vals = nullptr; M.shipped = false; M.encoded = false;
	if (L.slots) {
		M.slot_rows = reinterpret_cast<u32 *>(L.host + L.off_slots); M.slot_vals = reinterpret_cast<u32 *>(L.host + L.off_slots + L.slots_stride);
		M.d_slot_rows = reinterpret_cast<u32 *>(static_cast<char *>(L.dev) + L.off_slots); M.d_slot_vals = reinterpret_cast<u32 *>(static_cast<char *>(L.dev) + L.off_slots + L.slots_stride);
		M.rows = M.slot_rows; M.vals = M.slot_vals;
		return L;
	}
	if (L.bytes) {
		M.delta8 = reinterpret_cast<const uint8_t *>(host); M.vals8 = reinterpret_cast<const uint8_t *>(host) + L.off_val;
		M.segments = host + L.off_seg; M.seg_bytes = L.seg_bytes; M.list_cap = L.list_cap;
	} else if (L.narrow) { M.rows16 = reinterpret_cast<const uint16_t *>(host); M.vals16 = reinterpret_cast<const uint16_t *>(host) + M.nnz; }
	else { M.rows = reinterpret_cast<const u32 *>(host); M.vals = reinterpret_cast<const u32 *>(host) + M.nnz; }
	return L;
}

// this shard's columns (emitted into c.mat[slot] on the device; d_descr: local offset, global offset, length of each) -> their global
// places in the shared buffer, in the form open_shared chose
void dropest_shard::place_columns(Mat &M, int slot, bool filtered_m, const SharedLayout &L, const unsigned long long *d_descr, dropest::u32 nc, uint64_t local_nnz, hipStream_t st,
                                  const dropest::u32 *local_start) {
	using namespace dropest;
	dropest_ctx &c = *ctx;
	if (!st) st = c.stream;
	char *d_payload = static_cast<char *>(L.dev) + L.base;
	const dropest_ctx::MatrixResult &R = c.mat[slot];
	const bool work = nc && local_nnz;
	if (L.slots) {
		// The columns leave as the byte form of this shard's LOCAL matrix (the emit and the chunked copies of one context: whole lines at the
		// link's streaming rate, whatever the columns' lengths -- placing bytes at their GLOBAL places straight from a kernel met ragged column
		// ends with byte stores over PCIe: 22 GB/s on cm_raw's short columns), and the pool's host threads widen every chunk of columns into the
		// shared 32-bit slots at the columns' global places as soon as its arrival flag is up (matrix_decode.h).
		M.d_descr = d_descr; M.nc = nc; M.local_nnz = local_nnz;
		if (!work) return;
		dropest_ctx::WireTarget T;
		T.rows = M.slot_rows; T.vals = M.slot_vals; T.global_nnz = M.nnz; T.d_descr = d_descr;
		T.begin = M.dec_begin.empty() ? M.h_begin.p : M.dec_begin.data();
		T.end = M.dec_end.empty() ? M.h_end.p : M.dec_end.data();
		const std::vector<u32> &cells = filtered_m ? M.col_cell : raw_plan.col_cell, &starts = filtered_m ? M.col_start : raw_plan.col_start;
		c.ship_columns_to_slots(filtered_m, false, cells, starts, local_nnz, T, st);
		M.shipped = true;
		return;
	}
	if (L.bytes) {
		u32 *seg_words = reinterpret_cast<u32 *>(d_payload + L.off_seg + L.seg_bytes * size_t(rank));
		d_list_count.ensure(8);
		u32 *cnt = d_list_count.p + 4 * slot;
		HIP_CHECK(hipMemsetAsync(cnt, 0, 16, st));
		if (work) {
			u32 *lists = seg_words + 4;
			const size_t cap = L.list_cap;
			{
			auto launch = [&] {
				hipLaunchKernelGGL(place_columns_bytes_kernel, dim3(nc), dim3(filtered_m ? 256 : 64), 0, st, d_descr, R.d_row.p, R.d_val.p,
				                   reinterpret_cast<uint8_t *>(d_payload), reinterpret_cast<uint8_t *>(d_payload) + L.off_val, cnt,
				                   lists, lists + cap, lists + 2 * cap, lists + 3 * cap, L.list_cap);
			};
			if (st == c.stream) c.timed(filtered_m ? "place_columns:cm" : "place_columns:cm_raw", double(local_nnz) * 10, launch);
			else launch();   // (the context's launch timer brackets its own stream)
			}
		}
		hipLaunchKernelGGL(copy_words_kernel, dim3(1), dim3(64), 0, st, cnt, seg_words, 4u);   // the counts, behind the lists on the stream
		HIP_CHECK(hipGetLastError());
		return;
	}
	constexpr u32 OVF_CAP = 1u << 16;
	if (work) {
		if (L.narrow) {
			d_ovf.ensure(1 + 3 * size_t(OVF_CAP));
			HIP_CHECK(hipMemsetAsync(d_ovf.p, 0, 4, c.stream));
			hipLaunchKernelGGL(place_columns_narrow_kernel, dim3(nc), dim3(256), 0, c.stream, d_descr, R.d_row.p, R.d_val.p,
			                   reinterpret_cast<uint16_t *>(d_payload), reinterpret_cast<uint16_t *>(d_payload) + M.nnz, d_ovf.p, OVF_CAP);
		} else
			hipLaunchKernelGGL(place_columns_kernel, dim3(nc), dim3(256), 0, c.stream, d_descr, R.d_row.p, R.d_val.p,
			                   reinterpret_cast<u32 *>(d_payload), reinterpret_cast<u32 *>(d_payload) + M.nnz);
		HIP_CHECK(hipGetLastError());
	}
	if (L.narrow) {   // the (rare) entries beyond 16 bits of every shard, gathered on the host
		struct Ovf { u64 pos; u32 val, pad; };
		std::vector<Ovf> mine, all;
		if (work) {
			u32 count = 0;
			c.fetch(&count, d_ovf.p, 4);
			if (count > OVF_CAP) throw UnsupportedError("more than 2^16 matrix entries beyond 65534 on one shard: set the shard option narrow_matrix to 0");
			if (count) {
				std::vector<u32> raw(3 * size_t(count));
				c.fetch(raw.data(), d_ovf.p + 1, raw.size() * 4);
				for (u32 i = 0; i < count; ++i) mine.push_back(Ovf{u64(raw[3 * i]) | (u64(raw[3 * i + 1]) << 32), raw[3 * i + 2], 0});
			}
		}
		std::vector<size_t> cnt;
		tr->gather_vec(mine, all, cnt);
		std::sort(all.begin(), all.end(), [](const Ovf &a, const Ovf &b) { return a.pos < b.pos; });
		for (const Ovf &o : all) { M.ovf_pos.push_back(o.pos); M.ovf_val.push_back(o.val); }
	}
}

// cm_raw without a host table of all the real cells.  Its columns are the real cells of ALL shards in the order of ONE container's cell
// ids = the stream ordinal of every cell's first read; on a shard the real cells stand in that order already (local ids are first-seen
// ranks, and the blocks a shard received stand in stream order).  So the global matrix is a merge of `world` ascending lists:
//   plan_raw           (host) this shard's columns, their nnz prefix; ONE small collective: columns, nnz and ordinal queries per shard
//   assemble_raw_device        first-read ordinals on the device (the positions did not travel with a packed exchange: two small
//                              device all-to-alls ask the sources), all-gather of (ordinal, nnz prefix) of every shard's columns --
//                              16 bytes per column over the links --, then one thread per local column: binary searches in the other
//                              shards' lists give its global place and nnz offset; it writes colptr / barcode of its column into
//                              the shared buffer and the descriptor the placing kernel reads.
// The host table (build_global_table) then holds the filtered candidates only.  Falls back to the host plan when a shard's cells are
// not in ordinal order (never seen: a guard) or the option raw_on_device is off.
bool dropest_shard::plan_raw() {
	using namespace dropest;
	dropest_ctx &c = *ctx;
	Phase ph(this, "raw:plan");
	RawPlan &P = raw_plan;
	P.col_cell.clear(); P.col_start.clear(); P.query.clear(); P.pre.assign(1, 0);
	const bool ask = exchanged && !idx_exchanged;
	P.q_out.assign(size_t(world), 0);
	uint64_t ok = raw_on_device ? 1 : 0;
	u32 last = 0, src = 0;
	for (const HostCell &h : c.real) {
		if (h.merged || h.excluded || h.row.n_genes < c.min_before) continue;
		const u32 pos = h.row.first_read;
		if (pos == 0xFFFFFFFFu || (!P.col_cell.empty() && pos <= last)) { ok = 0; break; }
		last = pos;
		if (P.pre.back() + h.row.n_genes > 0xFFFFFFF0ull) throw UnsupportedError("count matrix with more than 2^32 non-zeros");
		P.col_cell.push_back(h.id); P.col_start.push_back(u32(P.pre.back())); P.pre.push_back(P.pre.back() + h.row.n_genes);
		if (ask) {
			while (src + 1 < u32(world) && pos >= recv_off[size_t(src) + 1]) ++src;
			P.query.push_back(u32(pos - recv_off[src])); ++P.q_out[src];
		} else
			P.query.push_back(pos);
	}
	// [ok, columns, nnz, queries to shard 0 .. world-1] of every shard
	const size_t w = 3 + size_t(world);
	std::vector<uint64_t> mine(w, 0);
	mine[0] = ok; mine[1] = P.col_cell.size(); mine[2] = P.pre.back();
	for (int p = 0; p < world; ++p) mine[3 + size_t(p)] = P.q_out[size_t(p)];
	P.counts.assign(w * size_t(world), 0);
	tr->gather_host(mine.data(), w * 8, P.counts.data());
	P.ncols = P.nnz = 0;
	P.q_in.assign(size_t(world), 0);
	for (int p = 0; p < world; ++p) {
		const uint64_t *row = P.counts.data() + w * size_t(p);
		ok &= row[0]; P.ncols += row[1]; P.nnz += row[2]; P.q_in[size_t(p)] = row[3 + size_t(rank)];
	}
	if (P.nnz > 0xFFFFFFF0ull) throw UnsupportedError("count matrix with more than 2^32 non-zeros");
	return ok != 0;
}

void dropest_shard::assemble_raw_device() {
	using namespace dropest;
	dropest_ctx &c = *ctx;
	Phase ph(this, "matrix:cm_raw");
	RawPlan &P = raw_plan;
	Mat &M = mat[1];
	ctx->mat[1].settle();
	const size_t w = 3 + size_t(world);
	const u32 nl = u32(P.col_cell.size());
	const uint64_t ncols = P.ncols;
	M.ncols = ncols; M.nnz = P.nnz; M.colptr.clear(); M.col_barcode.clear(); M.colptr32.clear();
	// head of the shared buffer: colptr64[ncols + 1] | colptr32[ncols + 1] | barcodes[ncols]
	const size_t off_c32 = (ncols + 1) * 8, off_bc = (off_c32 + (ncols + 1) * 4 + 15) & ~size_t(15), head = off_bc + ncols * 8;
	const SharedLayout L = open_shared(M, 1, head);
	M.colptr_p = reinterpret_cast<const u64 *>(L.host); M.colptr32_p = reinterpret_cast<const u32 *>(L.host + off_c32);
	M.barcode_p = reinterpret_cast<const u64 *>(L.host + off_bc);
	if (rank == 0) {   // the closing entry is nobody's column
		reinterpret_cast<u64 *>(L.host)[ncols] = P.nnz;
		reinterpret_cast<u32 *>(L.host + off_c32)[ncols] = u32(P.nnz);
	}
	// this shard's (first-read ordinal [nl] | nnz prefix [nl + 1])
	d_plan_mine.ensure(2 * size_t(nl) + 1); d_q.ensure(std::max<u32>(nl, 1)); d_col_cell.ensure(std::max<u32>(nl, 1));
	h_plan.ensure(size_t(nl) + 1 + size_t(nl));   // staging of its own (cm's descriptors may still be on their way from their staging buffer): prefix (u64) | queries, cells (u32)
	std::memcpy(h_plan.p, P.pre.data(), (size_t(nl) + 1) * 8);
	u32 *h32 = reinterpret_cast<u32 *>(h_plan.p + nl + 1);
	if (nl) { std::memcpy(h32, P.query.data(), size_t(nl) * 4); std::memcpy(h32 + nl, P.col_cell.data(), size_t(nl) * 4); }
	HIP_CHECK(hipMemcpyAsync(d_plan_mine.p + nl, h_plan.p, (size_t(nl) + 1) * 8, hipMemcpyHostToDevice, c.stream));
	if (nl) {
		HIP_CHECK(hipMemcpyAsync(d_q.p, h32, size_t(nl) * 4, hipMemcpyHostToDevice, c.stream));
		HIP_CHECK(hipMemcpyAsync(d_col_cell.p, h32 + nl, size_t(nl) * 4, hipMemcpyHostToDevice, c.stream));
	}
	if (exchanged && !idx_exchanged) {
		QueryTable t{};
		t.world = u32(world);
		uint64_t n_in = 0;
		for (int p = 0; p < world; ++p) {
			t.in_off[p] = n_in; n_in += P.q_in[size_t(p)]; t.part_off[p] = send_off[size_t(p)]; t.first_ord[p] = first_ord[size_t(p)];
			t.out_off[p + 1] = t.out_off[p] + P.q_out[size_t(p)];
		}
		t.in_off[world] = n_in;
		d_q_in.ensure(std::max<uint64_t>(n_in, 1)); d_q_ans.ensure(std::max<uint64_t>(n_in, 1)); d_q_back.ensure(std::max<u32>(nl, 1));
		{ const void *snd[1] = {d_q.p}; void *rcv[1] = {d_q_in.p}; const size_t elem[1] = {4};
		  tr->exchange(1, snd, rcv, elem, P.q_out.data(), P.q_in.data(), c.stream); }
		if (n_in) {
			hipLaunchKernelGGL(answer_queries_kernel, dim3(u32((n_in + 255) / 256)), dim3(256), 0, c.stream, t, d_q_in.p, u32(n_in), p_idx.p, d_q_ans.p);
			HIP_CHECK(hipGetLastError());
		}
		{ const void *snd[1] = {d_q_ans.p}; void *rcv[1] = {d_q_back.p}; const size_t elem[1] = {4};
		  tr->exchange(1, snd, rcv, elem, P.q_in.data(), P.q_out.data(), c.stream); }
		if (nl) hipLaunchKernelGGL(ordinals_from_answers_kernel, dim3((nl + 255) / 256), dim3(256), 0, c.stream, t, d_q_back.p, nl, reinterpret_cast<unsigned long long *>(d_plan_mine.p));
	} else if (nl)
		hipLaunchKernelGGL(ordinals_kernel, dim3((nl + 255) / 256), dim3(256), 0, c.stream, ordinal_map(), d_q.p, nl, reinterpret_cast<unsigned long long *>(d_plan_mine.p));
	HIP_CHECK(hipGetLastError());
	// every shard's block to every shard
	RawPlanTable pt{};
	pt.world = u32(world); pt.rank = u32(rank);
	std::vector<size_t> off(static_cast<size_t>(world), 0), bytes(static_cast<size_t>(world), 0);
	size_t total = 0;
	for (int p = 0; p < world; ++p) {
		const uint64_t n_p = P.counts[w * size_t(p) + 1];
		pt.off[p] = total; pt.n[p] = u32(n_p);
		off[size_t(p)] = total * 8; bytes[size_t(p)] = (2 * size_t(n_p) + 1) * 8;
		total += 2 * size_t(n_p) + 1;
	}
	d_plan_all.ensure(total);
	tr->gather_dev(d_plan_mine.p, d_plan_all.p, off.data(), bytes.data(), c.stream);
	d_desc_raw.ensure(std::max<size_t>(3 * size_t(nl), 1));
	M.dec_begin.clear(); M.dec_end.clear();
	if (L.slots) { M.h_begin.ensure(std::max<u32>(nl, 1)); M.h_end.ensure(std::max<u32>(nl, 1)); }
	if (nl) {
		char *d_head = static_cast<char *>(L.dev);
		hipLaunchKernelGGL(plan_raw_columns_kernel, dim3((nl + 255) / 256), dim3(256), 0, c.stream, pt, reinterpret_cast<const unsigned long long *>(d_plan_all.p),
		                   d_col_cell.p, reinterpret_cast<const unsigned long long *>(c.cell_cb.p), nl, reinterpret_cast<unsigned long long *>(d_desc_raw.p),
		                   reinterpret_cast<unsigned long long *>(d_head), reinterpret_cast<uint32_t *>(d_head + off_c32),
		                   reinterpret_cast<unsigned long long *>(d_head + off_bc), L.slots ? M.h_begin.p : static_cast<u32 *>(nullptr),
		                   L.slots ? M.h_end.p : static_cast<u32 *>(nullptr));
		HIP_CHECK(hipGetLastError());
	}
	const uint64_t local_nnz = P.pre.back();
	if (nl && local_nnz && !L.slots) c.emit_columns_device(false, false, P.col_cell, P.col_start, local_nnz, false);
	// the placing kernel on its own stream (byte form: nothing on the host waits for it before the end of the step)
	hipStream_t st = c.stream;
	if ((L.bytes || L.slots) && !getenv("DROPEST_SHARD_NO_PLACE_STREAM")) {
		if (!place_stream) { HIP_CHECK(hipStreamCreateWithFlags(&place_stream, hipStreamNonBlocking)); HIP_CHECK(hipEventCreateWithFlags(&ev_place, hipEventDisableTiming)); }
		HIP_CHECK(hipEventRecord(ev_place, c.stream));
		HIP_CHECK(hipStreamWaitEvent(place_stream, ev_place, 0));
		st = place_stream;
	}
	place_columns(M, 1, false, L, reinterpret_cast<const unsigned long long *>(d_desc_raw.p), nl, local_nnz, st, P.col_start.data());
}

void dropest_shard::finish_slots(int slot) {
	using namespace dropest;
	Mat &M = mat[slot];
	if (!M.slots || !M.shipped) return;
	M.shipped = false;
	dropest_ctx &c = *ctx;
	if (c.wire_finish(c.mat[slot])) return;
	// The lists of this shard's byte form overflowed (very sparse columns: a small cell lists nearly every row).  The slots ARE the 32-bit
	// form: this shard emits its columns as 32-bit arrays and places them there directly -- its own decision, no collective (ADVICE r3:
	// the step cannot fail for the shape of the data).
	phases["matrix:overflow"].launches++;
	const bool filtered_m = slot == 0;
	c.emit_columns_device(filtered_m, false, filtered_m ? M.col_cell : raw_plan.col_cell, filtered_m ? M.col_start : raw_plan.col_start, M.local_nnz, false);
	const dropest_ctx::MatrixResult &R = c.mat[slot];
	hipLaunchKernelGGL(place_columns_kernel, dim3(M.nc), dim3(256), 0, c.stream, M.d_descr, R.d_row.p, R.d_val.p, M.d_slot_rows, M.d_slot_vals);
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(stream_wait(c.stream));
}

// The byte form of a matrix whose step ended with the slots (dropest_shard_matrix_bytes asks for it): encoded from the slots, once.
void dropest_shard::encode_bytes(Mat &M) {
	using namespace dropest;
	if (M.encoded) return;
	M.enc_delta.assign(size_t(M.nnz), 0); M.enc_vals.assign(size_t(M.nnz), 0);
	M.rl_pos.clear(); M.rl_row.clear(); M.vl_pos.clear(); M.vl_val.clear();
	const u32 *cp = M.colptr32_p;
	for (uint64_t c = 0; c < M.ncols; ++c) {
		uint32_t prev1 = 0;
		for (uint32_t k = cp[c]; k < cp[c + 1]; ++k) {
			const uint32_t row = M.slot_rows[k], v = M.slot_vals[k], d = row + 1u - prev1;
			prev1 = row + 1u;
			M.enc_delta[k] = uint8_t(d >= 255u ? 255u : d); M.enc_vals[k] = uint8_t(v >= 255u ? 255u : v);
			if (d >= 255u) { M.rl_pos.push_back(k); M.rl_row.push_back(row); }
			if (v >= 255u) { M.vl_pos.push_back(k); M.vl_val.push_back(v); }
		}
	}
	M.delta8 = M.enc_delta.data(); M.vals8 = M.enc_vals.data(); M.lists_ready = true; M.encoded = true;
}

// the byte form's lists: every shard's segment of the shared buffer (written through its PCIe link, complete after the barrier)
// -> one list of a kind (a matrix whose lists overflowed on some shard was placed again without the byte form before this: step())
bool dropest_shard::lists_overflowed(const Mat &M) const {
	if (!M.bytes) return false;
	for (int p = 0; p < world; ++p) {
		const u32 *w = reinterpret_cast<const u32 *>(M.segments + M.seg_bytes * size_t(p));
		if (w[0] > M.list_cap || w[1] > M.list_cap) return true;
	}
	return false;
}

void dropest_shard::collect_lists(Mat &M) {
	using namespace dropest;
	if (!M.bytes || M.lists_ready) return;
	size_t nr = 0, nv = 0;
	for (int p = 0; p < world; ++p) {
		const u32 *w = reinterpret_cast<const u32 *>(M.segments + M.seg_bytes * size_t(p));
		if (w[0] > M.list_cap || w[1] > M.list_cap) throw InvalidError("internal: a byte-form matrix kept overflowed lists");
		nr += w[0]; nv += w[1];
	}
	M.rl_pos.resize(nr); M.rl_row.resize(nr); M.vl_pos.resize(nv); M.vl_val.resize(nv);
	size_t ar = 0, av = 0;
	for (int p = 0; p < world; ++p) {
		const u32 *w = reinterpret_cast<const u32 *>(M.segments + M.seg_bytes * size_t(p));
		const u32 *l = w + 4;
		if (w[0]) { std::memcpy(M.rl_pos.data() + ar, l, size_t(w[0]) * 4); std::memcpy(M.rl_row.data() + ar, l + M.list_cap, size_t(w[0]) * 4); ar += w[0]; }
		if (w[1]) { std::memcpy(M.vl_pos.data() + av, l + 2 * size_t(M.list_cap), size_t(w[1]) * 4); std::memcpy(M.vl_val.data() + av, l + 3 * size_t(M.list_cap), size_t(w[1]) * 4); av += w[1]; }
	}
	M.lists_ready = true;
}
