// matrix_emit.h -- the count matrices cm (filtered) and cm_raw: planning their columns on the host, the emit kernels' launches, the three
// forms a matrix leaves the device in (32-bit arrays, 16-bit arrays, bytes), the chunked "wire" that carries 32-bit slots as bytes and has
// host threads widen them (matrix_decode.h), cm as a rider on cm_raw, and the C entry points of all of it.
// Included by dropest_amd.hip; the kernels are in k_misc.h, the declarations in context.h.
//
// Every step has one copy here:
//   matrix_source      the source side of MatrixArgs (a slot's column arrays, the tables, the value array of (filtered, reads))
//   matrix_outputs     the target side for a device form, and the buffers behind it
//   launch_emit        the kernel(s) of a device form
//   MatrixResult::List the layout of an overflow list (context.h)
//   start_decode_job   chunked copies behind arrival flags + the job of the host threads
//   checked_nnz        the 2^32 limit
#pragma once

#include <sys/syscall.h>
#include <unistd.h>

static u32 checked_nnz(uint64_t nnz) {
	if (nnz > 0xFFFFFFF0ull) throw UnsupportedError("count matrix with more than 2^32 non-zeros");
	return u32(nnz);
}

void dropest_ctx::matrix_columns(bool filtered_m, std::vector<u32> &col_cell, std::vector<u32> &colptr, uint64_t &nnz) {
	col_cell.clear(); colptr.clear();
	nnz = 0;
	if (filtered_m) {
		filtered_cells();
		for (u32 ri : filtered_ridx) {
			const HostCell &h = real[ri];
			col_cell.push_back(h.id); colptr.push_back(u32(nnz)); nnz += h.row.requested_genes;
		}
	} else {
		// every real cell in cell-id order: millions of rows at C3 size -- counted and filled over contiguous ranges on a few threads
		constexpr unsigned W = dropest::HostPool::MAX;
		size_t cols[W] = {0}; uint64_t sums[W] = {0};
		auto is_col = [&](const HostCell &h) { return !(h.merged || h.excluded || h.row.n_genes < min_before); };
		const unsigned workers = parallel_ranges(real.size(), [&](size_t b, size_t e, unsigned w) {
			size_t c = 0; uint64_t s = 0;
			for (size_t i = b; i < e; ++i) if (is_col(real[i])) { ++c; s += real[i].row.n_genes; }
			cols[w] = c; sums[w] = s;
		}, 100000, W);
		size_t col0[W + 1] = {0}; uint64_t nnz0[W + 1] = {0};
		for (unsigned w = 0; w < workers; ++w) { col0[w + 1] = col0[w] + cols[w]; nnz0[w + 1] = nnz0[w] + sums[w]; }
		nnz = checked_nnz(nnz0[workers]);
		col_cell.resize(col0[workers]); colptr.resize(col0[workers]);
		parallel_ranges(real.size(), [&](size_t b, size_t e, unsigned w) {   // same n and limits: the same ranges
			size_t at = col0[w]; uint64_t run = nnz0[w];
			for (size_t i = b; i < e; ++i) if (is_col(real[i])) { col_cell[at] = real[i].id; colptr[at] = u32(run); run += real[i].row.n_genes; ++at; }
		}, 100000, W);
	}
	colptr.push_back(checked_nnz(nnz));
}

void dropest_ctx::invalidate_prefetch() {
	if (raw_pf.in_flight && stream2) HIP_CHECK(stream_wait(stream2));   // its buffers are about to be reused
	mat[1].settle();   // ... also by the host threads that widen them
	raw_pf.valid = raw_pf.in_flight = false;
}

// Narrow CSC (16-bit row indices and values + an exact overflow list) is possible when every gene id fits 16 bits.
bool dropest_ctx::narrow_possible() const { return n_reads == 0 || ingest.gene_max_plus1 <= 0x10000u; }

static constexpr u32 MATRIX_OVF_CAP = 1u << 20;   // value lists (a count beyond 254 / 65534 is rare in every matrix)
// Row lists of the byte form.  A sparse column (a small cell of cm_raw: a few dozen of 30 000 genes) lists most of its rows; an eighth of
// all entries listed costs as much again as the bytes themselves, and beyond that a wider form is the better wire.
static u32 matrix_row_list_cap(uint64_t nnz) {
	if (const char *e = getenv("DROPEST_MATRIX_ROW_LIST_CAP")) return u32(std::max(1L, atol(e)));   // (tests: a small list overflows on a small matrix)
	return u32(std::min<uint64_t>(std::max<uint64_t>(nnz / 8, MATRIX_OVF_CAP), 1ull << 25));
}

// The source side of an emit launch for matrix slot M.  The slot's column arrays must hold the columns when the kernel runs (uploaded on
// the kernel's stream, or behind an event: the invariant at MatrixResult::d_col_cell).
dropest::MatrixArgs dropest_ctx::matrix_source(const MatrixResult &M, bool filtered_m, bool reads_output) const {
	dropest::MatrixArgs a{};
	a.col_cell = M.d_col_cell.p; a.col_start = M.d_col_start.p; a.cell_cg_begin = cell_cg_begin.p; a.cell_cg_count = cell_cg_count.p; a.cg_key = cg_key.p;
	a.value = filtered_m ? (reads_output ? cg_reads_req.p : cg_n_req.p) : (reads_output ? cg_reads_all.p : cg_n_all.p);
	a.gene_mask = layout.gene_none; a.skip_zero = filtered_m ? 1 : 0;
	return a;
}

// Wires the output side of an emit launch for matrix slot M (device form 0 / 1 / 2) and makes sure the buffers exist.
void dropest_ctx::matrix_outputs(MatrixResult &M, uint64_t nnz, int form, bool to_host, dropest::MatrixArgs &a) {
	M.settle();   // (a decoding thread may still be leaving the slot's previous job: its buffers are about to be rewritten or regrown)
	M.vals.n = M.rows.n = 0;
	if (form) {
		M.vals.ensure(MATRIX_OVF_CAP, to_host);
		a.ovf_count = M.vals.d_count(); a.ovf_pos = M.vals.d_pos(); a.ovf_val = M.vals.d_val(); a.ovf_cap = M.vals.cap;
	}
	if (form == 2) {
		M.d_drow8.ensure(nnz); M.d_val8.ensure(nnz); M.rows.ensure(matrix_row_list_cap(nnz), to_host);
		if (to_host) { M.h_drow8.ensure(nnz); M.h_val8.ensure(nnz); }
		a.t_drow8 = M.d_drow8.p; a.t_val8 = M.d_val8.p;
		a.rovf_count = M.rows.d_count(); a.rovf_pos = M.rows.d_pos(); a.rovf_row = M.rows.d_val(); a.rovf_cap = M.rows.cap;
	} else if (form == 1) {
		M.d_row16.ensure(nnz); M.d_val16.ensure(nnz);
		if (to_host) { M.h_row16.ensure(nnz); M.h_val16.ensure(nnz); }
		a.t_gene16 = M.d_row16.p; a.t_val16 = M.d_val16.p;
	} else {
		M.d_row.ensure(nnz); M.d_val.ensure(nnz);
		if (to_host) { M.h_row.ensure(nnz); M.h_val.ensure(nnz); }
		a.t_gene = M.d_row.p; a.t_val = M.d_val.p;
	}
}

// The emit kernel(s) of device form 0 / 1 / 2 over the columns of M.colptr, on `st`.  Byte form: long columns by the workgroup-per-column
// kernel, short ones (fewer than 256 entries by colptr -- for cm an upper bound: the kernel walks a few more rows and drops the zeros) by
// the wave-per-column kernel; the slot's column list (filled and uploaded here) holds the long columns first, then the short ones.
void dropest_ctx::launch_emit(int dev_form, dropest::MatrixArgs a, MatrixResult &M, hipStream_t st) {
	using namespace dropest;
	const u32 ncols = u32(M.ncols);
	if (dev_form == 0) { hipLaunchKernelGGL(emit_matrix_kernel<0>, dim3(ncols), dim3(256), 0, st, a); return; }
	if (dev_form == 1) { hipLaunchKernelGGL(emit_matrix_kernel<1>, dim3(ncols), dim3(256), 0, st, a); return; }
	auto is_long = [&](u32 j) { return M.colptr[j + 1] - M.colptr[j] >= 256u; };
	M.col_list_host.resize(ncols);
	u32 n_long = 0;
	for (u32 j = 0; j < ncols; ++j) if (is_long(j)) M.col_list_host[n_long++] = j;
	u32 at = n_long;
	for (u32 j = 0; j < ncols; ++j) if (!is_long(j)) M.col_list_host[at++] = j;
	M.d_col_list.ensure(ncols);
	HIP_CHECK(hipMemcpyAsync(M.d_col_list.p, M.col_list_host.data(), size_t(ncols) * 4, hipMemcpyHostToDevice, st));
	if (n_long) { a.col_list = M.d_col_list.p; a.n_list = n_long; hipLaunchKernelGGL(emit_matrix_kernel<2>, dim3(n_long), dim3(256), 0, st, a); }
	if (ncols > n_long) {
		a.col_list = M.d_col_list.p + n_long; a.n_list = ncols - n_long;
		hipLaunchKernelGGL(emit_matrix_bytes_short_kernel, dim3(div_up(a.n_list, EMS_COLS)), dim3(256), 0, st, a);
	}
}

// Device-to-host copies of a matrix slot on stream `st` (after its emit launch).  Forms 1 / 2: the counts of the overflow lists travel
// with the arrays (listed entries are rare); the lists themselves are fetched by matrix_finish_overflow.
void dropest_ctx::matrix_copy_out(MatrixResult &M, uint64_t nnz, hipStream_t st) {
	if (M.narrow == 2) {
		HIP_CHECK(hipMemcpyAsync(M.h_drow8.p, M.d_drow8.p, nnz, hipMemcpyDeviceToHost, st));
		HIP_CHECK(hipMemcpyAsync(M.h_val8.p, M.d_val8.p, nnz, hipMemcpyDeviceToHost, st));
		HIP_CHECK(hipMemcpyAsync(M.vals.h_count(), M.vals.d_count(), 4, hipMemcpyDeviceToHost, st));
		HIP_CHECK(hipMemcpyAsync(M.rows.h_count(), M.rows.d_count(), 4, hipMemcpyDeviceToHost, st));
	} else if (M.narrow == 1) {
		HIP_CHECK(hipMemcpyAsync(M.h_row16.p, M.d_row16.p, nnz * 2, hipMemcpyDeviceToHost, st));
		HIP_CHECK(hipMemcpyAsync(M.h_val16.p, M.d_val16.p, nnz * 2, hipMemcpyDeviceToHost, st));
		HIP_CHECK(hipMemcpyAsync(M.vals.h_count(), M.vals.d_count(), 4, hipMemcpyDeviceToHost, st));
	} else {
		HIP_CHECK(hipMemcpyAsync(M.h_row.p, M.d_row.p, nnz * 4, hipMemcpyDeviceToHost, st));
		HIP_CHECK(hipMemcpyAsync(M.h_val.p, M.d_val.p, nnz * 4, hipMemcpyDeviceToHost, st));
	}
}

// After the copies of matrix_copy_out have been waited for: the overflow lists of a form 1 / 2 matrix (short or empty).
void dropest_ctx::matrix_finish_overflow(MatrixResult &M, hipStream_t st) {
	M.vals.n = M.rows.n = 0;
	if (!M.narrow || !M.nnz) return;
	auto finish = [&](MatrixResult::List &l, const char *what) {
		const u32 count = *l.h_count();
		if (count > l.cap) throw UnsupportedError(std::string("more than ") + std::to_string(l.cap) + " matrix entries with " + what + ": take the 32-bit form of the count matrix (dropest_count_matrix_csc)");
		l.n = count;
		if (!count) return;
		HIP_CHECK(hipMemcpyAsync(l.h_pos(), l.d_pos(), size_t(count) * 4, hipMemcpyDeviceToHost, st));
		HIP_CHECK(hipMemcpyAsync(l.h_val(), l.d_val(), size_t(count) * 4, hipMemcpyDeviceToHost, st));
		HIP_CHECK(stream_wait(st));
		// The list is filled in the order the atomics landed.  The 16-bit form promises it sorted by position (a handful of entries).  The
		// byte form does not: the small cells of cm_raw list 4e5 rows at C2 (25 ms of std::sort here, 0.9 ms of radix passes and their
		// waits on the device), and its decoder needs no order (dropest_matrix_bytes_widen).
		if (M.narrow == 2) return;
		std::vector<std::pair<u32, u32>> ov(count);
		for (u32 i = 0; i < count; ++i) ov[i] = {l.h_pos()[i], l.h_val()[i]};
		std::sort(ov.begin(), ov.end());
		for (u32 i = 0; i < count; ++i) { l.h_pos()[i] = ov[i].first; l.h_val()[i] = ov[i].second; }
	};
	finish(M.vals, M.narrow == 2 ? "a count beyond 254" : "a count beyond 65534");
	if (M.narrow == 2) finish(M.rows, "a row gap beyond 254");
}

// ---- 32-bit slots that cross PCIe as bytes (matrix_decode.h) ----
// dropest_count_matrix_csc hands out the dgCMatrix slots i / x as 32-bit arrays (ResultsPrinter.cpp:433-442).  As such they are 8 bytes
// per entry on a link of ~50 GB/s -- 6 ms for the 3.8e7 entries of C2, the longest single piece of a 10 ms pass.  So a large matrix is
// emitted in the byte form (2 bytes per entry), copied in chunks of whole columns with an event behind each, and widened into the slots by
// host threads while the next chunk is on the link.  Lists longer than their capacity (a matrix of very sparse columns): the slots are emitted
// directly instead, as before (wire_finish returns false).  DROPEST_MATRIX_DIRECT=1 switches the detour off.
bool dropest_ctx::wire_wanted(uint64_t nnz, int form, bool to_host) const {
	static const bool off = getenv("DROPEST_MATRIX_DIRECT") != nullptr;
	return form == 0 && to_host && !off && matrix_wire && nnz >= (1u << 18);
}

// The second half of every wire: `job` (sources, targets, `derived` and chunk_end set by the caller; the lists are slot M's) becomes M's
// job.  The byte arrays d_a / d_b (d_b and h_b null: one array) leave for h_a / h_b on `st` in the chunks of job->chunk_end over `colptr`.
void dropest_ctx::start_decode_job(MatrixResult &M, const std::shared_ptr<dropest::DecodeJob> &job, const u32 *colptr, const uint8_t *d_a, const uint8_t *d_b,
                                   uint8_t *h_a, uint8_t *h_b, hipStream_t st) {
	using namespace dropest;
	HIP_CHECK(hipGetDevice(&job->device));
	job->r_count = M.rows.h_count(); job->r_pos = M.rows.h_pos(); job->r_val = M.rows.h_val(); job->rcap = M.rows.cap;
	job->v_count = M.vals.h_count(); job->v_pos = M.vals.h_pos(); job->v_val = M.vals.h_val(); job->vcap = M.vals.cap;
	// Arrival flags (matrix_decode.h): [0] the lists, [1 + j] chunk j; the value of this emit is a number no earlier emit of the slot used.
	const size_t K = job->chunk_end.size();
	M.h_flags.ensure(K + 2);
	for (size_t j = 0; j < K + 2; ++j) M.h_flags.p[j] = 0;   // (the slot's previous job is complete: nobody reads or writes these now)
	M.wire_epoch = M.wire_epoch + 1 ? M.wire_epoch + 1 : 1;
	job->flags = M.h_flags.p; job->epoch = M.wire_epoch;
	// Every chunk leaves by a kernel that writes the pinned buffers itself (k_misc.h: a device-to-host hipMemcpyAsync costs ~20 us of
	// copy-engine set-up each, two dozen of them per matrix) and starts by raising the flag of what came before it on the stream.
	u32 c0 = 0;
	for (size_t j = 0; j < K; ++j) {
		const u32 c1 = job->chunk_end[j];
		const size_t k0 = colptr[c0], k1 = colptr[c1];
		hipLaunchKernelGGL(matrix_chunk_to_host_kernel, dim3(u32(std::max<size_t>(1, std::min<size_t>(128, (k1 - k0 + 4095) / 4096)))), dim3(256), 0, st, d_a, d_b, h_a, h_b,
		                   k0, k1, M.h_flags.p + j, M.wire_epoch);
		c0 = c1;
	}
	hipLaunchKernelGGL(matrix_flag_kernel, dim3(1), dim3(1), 0, st, M.h_flags.p + K, M.wire_epoch);
	HIP_CHECK(hipGetLastError());
	static const bool trace = getenv("DROPEST_WIRE_TRACE") != nullptr;
	job->trace = trace;
	static const uint64_t slice_entries = [] { const char *e = getenv("DROPEST_DECODE_SLICE"); return e && atoll(e) >= 1024 ? uint64_t(atoll(e)) : uint64_t(1) << 16; }();
	static const uint32_t test_delay = [] { const char *e = getenv("DROPEST_DECODE_TEST_DELAY_US"); return e ? uint32_t(std::max(0, atoi(e))) : 0u; }();
	job->test_delay_us = test_delay;
	job->prepare(slice_entries);
	M.job = job; M.wire = true;
	M.job_t0 = std::chrono::steady_clock::now();
	DecodePool::get().prefer_node_of(job->ro);
	DecodePool::get().submit(job);
}

void dropest_ctx::wire_copy_and_decode(MatrixResult &M, uint64_t nnz, hipStream_t st, const WireTarget *target) {
	using namespace dropest;
	if (!target) { M.h_row.ensure(nnz); M.h_val.ensure(nnz); }
	if (target) hipLaunchKernelGGL(matrix_lists_out_global_kernel, dim3(64), dim3(256), 0, st, M.rows.d.p, M.rows.cap, M.rows.h.p, M.vals.d.p, M.vals.cap, M.vals.h.p, target->d_descr, u32(M.ncols));
	else hipLaunchKernelGGL(matrix_lists_out_kernel, dim3(64), dim3(256), 0, st, M.rows.d.p, M.rows.cap, M.rows.h.p, M.vals.d.p, M.vals.cap, M.vals.h.p);
	HIP_CHECK(hipGetLastError());
	auto job = std::make_shared<DecodeJob>();
	job->m.rd = M.h_drow8.p; job->m.vb = M.h_val8.p; job->m.colptr = M.colptr.data(); job->m.ncols = M.ncols; job->m.nnz = nnz;
	job->ro = M.h_row.p; job->vo = M.h_val.p;
	if (target) {   // a shard's columns: bytes by the local colptr, slots at each column's global place
		job->m.colptr = target->begin; job->m.colend = target->end; job->m.bytebeg = M.colptr.data(); job->m.nnz = target->global_nnz;
		job->cut = M.colptr.data();
		job->ro = target->rows; job->vo = target->vals;
	}
	static const uint64_t n_chunks = [] { const char *e = getenv("DROPEST_WIRE_CHUNKS"); return uint64_t(e ? std::max(1, atoi(e)) : 12); }();
	cut_columns(M.colptr.data(), 0, size_t(M.ncols), std::max<uint64_t>(nnz / n_chunks + 1, uint64_t(1) << 19), job->chunk_end);
	M.wire_chunk_end = job->chunk_end;   // (a rider on this matrix moves its bytes in the same chunks: emit_rider)
	start_decode_job(M, job, M.colptr.data(), M.d_drow8.p, M.d_val8.p, M.h_drow8.p, M.h_val8.p, st);
}

// Sharded runs: the columns of a caller-given list of cells (local offsets col_start, nnz entries in all) leave the device as the byte form
// of a LOCAL matrix -- the emit of one context, the same chunked copies at the link's streaming rate -- and the pool's host threads widen
// them into the caller's slots at each column's GLOBAL place (the target).  The caller ends with wire_finish(mat[...]); false = the lists
// overflowed (very sparse columns): it then places the 32-bit form itself.
void dropest_ctx::ship_columns_to_slots(bool filtered_m, bool reads_output, const std::vector<u32> &col_cell, const std::vector<u32> &col_start, uint64_t nnz,
                                        const WireTarget &target, hipStream_t copy_st) {
	using namespace dropest;
	if (!filtered_m) invalidate_prefetch();   // (cm's columns use their own slot: cm_raw's may still be on their way, and stay so)
	MatrixResult &M = mat[filtered_m ? 0 : 1];
	M.settle();
	const u32 ncols = u32(col_cell.size());
	M.colptr.assign(col_start.begin(), col_start.end()); M.colptr.push_back(u32(nnz));
	M.nnz = nnz; M.ncols = ncols; M.narrow = 0; M.vals.n = M.rows.n = 0; M.wire = false;
	if (!ncols || !nnz) return;
	M.d_col_cell.ensure(ncols); M.d_col_start.ensure(ncols);
	MatrixArgs a = matrix_source(M, filtered_m, reads_output);
	matrix_outputs(M, nnz, 2, true, a);
	HIP_CHECK(hipMemcpyAsync(M.d_col_cell.p, col_cell.data(), size_t(ncols) * 4, hipMemcpyHostToDevice, stream));
	HIP_CHECK(hipMemcpyAsync(M.d_col_start.p, col_start.data(), size_t(ncols) * 4, hipMemcpyHostToDevice, stream));
	HIP_CHECK(hipMemsetAsync(M.vals.d_count(), 0, 4, stream));
	HIP_CHECK(hipMemsetAsync(M.rows.d_count(), 0, 4, stream));
	timed(filtered_m ? "emit_matrix:cm" : "emit_matrix:cm_raw", double(nnz) * 14, [&] { launch_emit(2, a, M, stream); });
	if (copy_st && copy_st != stream) {
		if (!ev_ship) HIP_CHECK(hipEventCreateWithFlags(&ev_ship, hipEventDisableTiming));
		HIP_CHECK(hipEventRecord(ev_ship, stream));
		HIP_CHECK(hipStreamWaitEvent(copy_st, ev_ship, 0));
	} else copy_st = stream;
	wire_copy_and_decode(M, nnz, copy_st, &target);
}

bool dropest_ctx::wire_finish(MatrixResult &M) {
	using dropest::DecodeJob;
	if (!M.job) return true;
	HostStage hs(this, "matrix:decode_wait");
	const auto w0 = std::chrono::steady_clock::now();
	M.job->work(true);   // the caller takes part: what is unclaimed, then what a straggler holds
	const int st = M.job->finish_rider();   // (= wait(); a rider's listed values are put in place here)
	if (M.job->trace) {
		const auto now = std::chrono::steady_clock::now();
		{   // where the buffers live (NUMA node of a few pages each) and where this thread runs
			auto node_of = [](const void *p, size_t bytes) {
				void *pages[8]; int status[8] = {-9, -9, -9, -9, -9, -9, -9, -9};
				for (int i = 0; i < 8; ++i) pages[i] = reinterpret_cast<void *>((reinterpret_cast<uintptr_t>(p) + bytes / 8 * size_t(i)) & ~uintptr_t(4095));
				(void)syscall(SYS_move_pages, 0, 8ul, pages, nullptr, status, 0);
				std::string out;
				for (int i = 0; i < 8; ++i) out += std::to_string(status[i]) + (i < 7 ? "," : "");
				return out;
			};
			fprintf(stderr, "[wire] nodes: rows %s | values %s | delta bytes %s | caller on cpu %d\n", node_of(M.h_row.p, M.nnz * 4).c_str(),
			        node_of(M.h_val.p, M.nnz * 4).c_str(), node_of(M.h_drow8.p, M.nnz).c_str(), sched_getcpu());
		}
		fprintf(stderr, "[wire] nnz %llu: submit -> done %.3f ms, waited %.3f ms, slowest slice %.3f ms of %zu slices in %zu chunks\n", (unsigned long long)M.nnz,
		        std::chrono::duration<double, std::milli>(now - M.job_t0).count(), std::chrono::duration<double, std::milli>(now - w0).count(),
		        double(M.job->slowest_slice_ns.load()) * 1e-6, M.job->slice_end.size(), M.job->chunk_end.size());
	}
	M.rows.n = M.job->n_r; M.vals.n = M.job->n_v;
	M.late_job = std::move(M.job);   // complete; a straggler may still be inside (settle() before the buffers are touched again)
	M.job.reset();
	if (st == DecodeJob::DONE) return true;
	if (st == DecodeJob::OVERFLOW) return false;
	throw DeviceError(st == DecodeJob::FAILED ? "count matrix: a copy of the byte form failed" : "count matrix: a listed entry of the byte form lies outside the matrix");
}

// cm_raw on a second stream: emit + device-to-host copy start now and run under whatever the caller does next (ordering
// the filtered cells, emitting cm); dropest_count_matrix_csc(filtered = 0) later only waits for the copy (and, for the 32-bit
// slots that travel as bytes, for the host threads that widen them).
void dropest_ctx::prefetch_raw_matrix(bool reads_output, int narrow, const dropest::CellRowPod *rows, const u32 *ids, u32 count) {
	if (raw_pf.valid && raw_pf.reads_output == reads_output && raw_pf.narrow == narrow) return;   // already under way (dropest_set_raw_matrix_prefetch)
	HostStage hs(this, "prefetch:cm_raw");
	invalidate_prefetch();
	if (narrow == 1 && !narrow_possible()) throw UnsupportedError("gene ids beyond 65535: the narrow matrix form is not available");
	MatrixResult &M = mat[1];
	uint64_t nnz = 0;
	if (rows) {   // straight from the rows fetch_real_cells just received (every one of them a column: n_genes >= min_genes_before_merge, nothing merged or excluded yet)
		raw_pf.col_cell.assign(ids, ids + count);
		M.colptr.resize(size_t(count) + 1);
		for (u32 i = 0; i < count; ++i) { M.colptr[i] = u32(nnz); nnz += rows[i].n_genes; }
		M.colptr[count] = checked_nnz(nnz);
	} else
		matrix_columns(false, raw_pf.col_cell, M.colptr, nnz);
	M.nnz = nnz; M.ncols = raw_pf.col_cell.size(); M.narrow = narrow; M.vals.n = M.rows.n = 0; M.wire = false;
	raw_pf.valid = true; raw_pf.reads_output = reads_output; raw_pf.narrow = narrow;
	if (nnz == 0) return;
	if (!stream2) {
		HIP_CHECK(hipStreamCreateWithFlags(&stream2, hipStreamNonBlocking));
		HIP_CHECK(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
		HIP_CHECK(hipEventCreateWithFlags(&ev_raw, hipEventDisableTiming));
	}
	const u32 ncols = u32(raw_pf.col_cell.size());
	M.d_col_cell.ensure(ncols); M.d_col_start.ensure(ncols);
	MatrixArgs a = matrix_source(M, false, reads_output);
	const bool wire = wire_wanted(nnz, narrow, true);
	const int dev_form = wire ? 2 : narrow;
	matrix_outputs(M, nnz, dev_form, true, a);
	HIP_CHECK(hipEventRecord(ev_fork, stream));                // everything enqueued so far (the tables) comes first
	HIP_CHECK(hipStreamWaitEvent(stream2, ev_fork, 0));
	HIP_CHECK(hipMemcpyAsync(M.d_col_cell.p, raw_pf.col_cell.data(), size_t(ncols) * 4, hipMemcpyHostToDevice, stream2));
	HIP_CHECK(hipMemcpyAsync(M.d_col_start.p, M.colptr.data(), size_t(ncols) * 4, hipMemcpyHostToDevice, stream2));
	if (!ev_raw_cols) HIP_CHECK(hipEventCreateWithFlags(&ev_raw_cols, hipEventDisableTiming));
	HIP_CHECK(hipEventRecord(ev_raw_cols, stream2));
	if (dev_form) HIP_CHECK(hipMemsetAsync(M.vals.d_count(), 0, 4, stream2));
	if (dev_form == 2) HIP_CHECK(hipMemsetAsync(M.rows.d_count(), 0, 4, stream2));
	launch_emit(dev_form, a, M, stream2);
	HIP_CHECK(hipGetLastError());
	if (wire) wire_copy_and_decode(M, nnz, stream2); else matrix_copy_out(M, nnz, stream2);
	HIP_CHECK(hipEventRecord(ev_raw, stream2));
	raw_pf.in_flight = true;
}

void dropest_ctx::emit_matrix(bool filtered_m, bool reads_output, bool to_host, int narrow, bool direct) {
	HostStage hs(this, filtered_m ? "matrix:cm" : "matrix:cm_raw");
	if (narrow == 1 && !narrow_possible()) throw UnsupportedError("gene ids beyond 65535: the narrow matrix form is not available");
	MatrixResult &M = mat[filtered_m ? 0 : 1];
	std::vector<u32> col_cell;
	uint64_t nnz = 0;
	if (!direct && !filtered_m && raw_pf.valid && to_host && raw_pf.reads_output == reads_output && raw_pf.narrow == narrow) {
		// A prefetched cm_raw of the same value kind and form IS what this call would produce: whatever changes the container
		// (merges, mutators, a new pass) discards the prefetch on its way in (invalidate_prefetch), so a valid one is current.
		// (Round 2 rebuilt and compared the column lists here: two walks over 2.5 M cells, 10 ms of a C3 pass.)
		bool ok = true;
		if (raw_pf.in_flight) {
			HIP_CHECK(event_wait(ev_raw)); raw_pf.in_flight = false;
			if (M.wire) ok = wire_finish(M); else matrix_finish_overflow(M, stream2);
		}
		if (ok) return;
		direct = true;   // the lists of the byte form overflowed: the slots come directly
	}
	if (!filtered_m) invalidate_prefetch();
	M.settle();
	tail_mark(filtered_m ? "emit_matrix(cm) entered" : "emit_matrix(cm_raw) entered");
	matrix_columns(filtered_m, col_cell, M.colptr, nnz);
	tail_mark("columns known");
	M.nnz = nnz; M.ncols = col_cell.size(); M.narrow = narrow; M.vals.n = M.rows.n = 0; M.wire = false;
	if (nnz == 0) return;
	const u32 ncols = u32(col_cell.size());
	const bool wire = !direct && wire_wanted(nnz, narrow, to_host);
	if (wire && filtered_m && emit_rider(reads_output, col_cell, nnz)) {   // cm's values ride on cm_raw's rows: half of cm's bytes stay off the link
		tail_mark("rider enqueued");
		HIP_CHECK(stream_wait(stream));
		const bool ok = wire_finish(M);
		tail_mark("matrix done");
		collect_timings();
		if (!ok) emit_matrix(filtered_m, reads_output, to_host, narrow, true);
		return;
	}
	const int dev_form = wire ? 2 : narrow;
	M.d_col_cell.ensure(ncols); M.d_col_start.ensure(ncols);
	MatrixArgs a = matrix_source(M, filtered_m, reads_output);
	matrix_outputs(M, nnz, dev_form, to_host, a);
	HIP_CHECK(hipMemcpyAsync(M.d_col_cell.p, col_cell.data(), size_t(ncols) * 4, hipMemcpyHostToDevice, stream));
	HIP_CHECK(hipMemcpyAsync(M.d_col_start.p, M.colptr.data(), size_t(ncols) * 4, hipMemcpyHostToDevice, stream));
	if (dev_form) HIP_CHECK(hipMemsetAsync(M.vals.d_count(), 0, 4, stream));
	if (dev_form == 2) HIP_CHECK(hipMemsetAsync(M.rows.d_count(), 0, 4, stream));
	timed(filtered_m ? "emit_matrix:cm" : "emit_matrix:cm_raw", double(nnz) * (dev_form == 2 ? 14 : dev_form ? 16 : 20), [&] { launch_emit(dev_form, a, M, stream); });
	tail_mark("emit enqueued");
	if (to_host) { if (wire) wire_copy_and_decode(M, nnz, stream); else matrix_copy_out(M, nnz, stream); }
	tail_mark("copies enqueued");
	HIP_CHECK(stream_wait(stream));   // col_cell (host vector) must outlive the H2D copy
	tail_mark("stream drained");
	bool ok = true;
	if (to_host) { if (wire) ok = wire_finish(M); else matrix_finish_overflow(M, stream); }
	tail_mark("matrix done");
	collect_timings();
	if (!ok) emit_matrix(filtered_m, reads_output, to_host, narrow, true);
}

// cm as a rider on cm_raw (k_misc.h: emit_values_on_rows_kernel, matrix_decode.h: widen_derived).  Taken when cm_raw of the
// same value kind is on its way (or there) in the byte form: one byte per entry of cm_raw -- its value in cm, 0 = not in cm -- crosses the link
// in cm_raw's chunks, and the host threads build cm's slots from cm_raw's row deltas.  mat[0].colptr / nnz are cm's own (the caller set them).
// false: not possible here (the caller emits cm's own byte form).
bool dropest_ctx::emit_rider(bool reads_output, const std::vector<u32> &col_cell, uint64_t nnz) {
	using namespace dropest;
	static const bool off = getenv("DROPEST_NO_RIDER") != nullptr;
	MatrixResult &M = mat[0], &R = mat[1];
	// Measured (NOTES_r06 section 5): at C3 (1.9e8 entries per matrix) the step is 0 to 6 ms shorter with the rider, box by box (0.18 of 0.69 GB off the link); at C2 (1.9e7
	// entries) the 0.35 ms of link time it saves are within the noise of its own dependencies (cm's columns wait for cm_raw's lists and
	// chunks): 9.53 against 9.32 ms over five pairs of runs.  Taken from 2^26 entries of cm_raw on; DROPEST_RIDER_MIN_NNZ moves the gate (tests: 0).
	const char *e_min = getenv("DROPEST_RIDER_MIN_NNZ");
	const uint64_t min_nnz = e_min ? uint64_t(std::max(0ll, atoll(e_min))) : (uint64_t(1) << 26);
	if (R.nnz < min_nnz) return false;
	if (off || !raw_pf.valid || !R.wire || R.narrow != 0 || raw_pf.reads_output != reads_output || !R.nnz || R.wire_chunk_end.empty() || !ev_raw_cols) return false;
	if (R.job == nullptr && R.late_job == nullptr) return false;   // (cm_raw's bytes have been let go)
	if (R.job && !R.job->running() && R.job->status.load() != DecodeJob::DONE) return false;   // cm_raw takes a wider form
	const u32 rcols = u32(R.ncols), ncols = u32(col_cell.size());
	if (raw_pf.col_cell.size() != rcols) return false;
	M.rider_out.assign(rcols, 0xFFFFFFFFu); M.rider_cnt.assign(rcols, 0u);
	for (u32 j = 0; j < ncols; ++j) {   // (cm_raw's columns ascend by cell id)
		auto it = std::lower_bound(raw_pf.col_cell.begin(), raw_pf.col_cell.end(), col_cell[j]);
		if (it == raw_pf.col_cell.end() || *it != col_cell[j]) return false;       // a filtered cell that is no column of cm_raw: not this way
		const size_t r = size_t(it - raw_pf.col_cell.begin());
		M.rider_out[r] = M.colptr[j]; M.rider_cnt[r] = M.colptr[j + 1] - M.colptr[j];
	}
	MatrixArgs a = matrix_source(R, true, reads_output);   // cm's values over cm_raw's columns
	matrix_outputs(M, R.nnz, 2, true, a);          // (value bytes and lists sized for cm_raw's entries; settles the slot's previous job)
	M.h_row.ensure(nnz); M.h_val.ensure(nnz);
	M.d_rider_out.ensure(rcols);
	HIP_CHECK(hipMemcpyAsync(M.d_rider_out.p, M.rider_out.data(), size_t(rcols) * 4, hipMemcpyHostToDevice, stream));
	HIP_CHECK(hipMemsetAsync(M.vals.d_count(), 0, 4, stream));
	HIP_CHECK(hipMemsetAsync(M.rows.d_count(), 0, 4, stream));
	HIP_CHECK(hipStreamWaitEvent(stream, ev_raw_cols, 0));   // cm_raw's column arrays (R.d_col_cell / R.d_col_start) are on the device
	timed("emit_matrix:cm", double(R.nnz) * 13, [&] {
		hipLaunchKernelGGL(emit_values_on_rows_kernel, dim3(std::min<u32>(div_up(rcols, 4u), 8192u)), dim3(256), 0, stream, a.col_cell, a.col_start, rcols, a.cell_cg_begin,
		                   a.cell_cg_count, a.cg_key, a.gene_mask, a.value, M.d_rider_out.p, M.d_val8.p, a.ovf_count, a.ovf_pos, a.ovf_val, a.ovf_cap);
	});
	hipLaunchKernelGGL(matrix_lists_out_kernel, dim3(64), dim3(256), 0, stream, M.rows.d.p, M.rows.cap, M.rows.h.p, M.vals.d.p, M.vals.cap, M.vals.h.p);   // (the row list: always empty, a rider has no rows of its own)
	HIP_CHECK(hipGetLastError());
	auto job = std::make_shared<DecodeJob>();
	job->m.rd = R.h_drow8.p; job->m.vb = M.h_val8.p; job->m.colptr = R.colptr.data(); job->m.ncols = rcols; job->m.nnz = nnz;
	job->ro = M.h_row.p; job->vo = M.h_val.p;
	job->derived = true;
	job->dv.base_ro = R.h_row.p; job->dv.out_begin = M.rider_out.data(); job->dv.out_count = M.rider_cnt.data();
	if (R.job && R.job->running()) { job->base_job = R.job; job->flags2 = R.h_flags.p; job->epoch2 = R.wire_epoch; }
	job->chunk_end = R.wire_chunk_end;
	M.narrow = 0;
	R.dependent = &M;
	start_decode_job(M, job, R.colptr.data(), M.d_val8.p, nullptr, M.h_val8.p, nullptr, stream);   // one array: the value bytes, in cm_raw's chunks
	if (profiling) stats["count:cm_rides_on_cm_raw"].launches += 1;
	return true;
}

// Sharded runs: the columns of a caller-given list of cells, emitted compactly into the device staging of matrix slot
// (filtered: cm values and zero-skipping; else cm_raw) -- the caller places them in the global matrix.
void dropest_ctx::emit_columns_device(bool filtered_m, bool reads_output, const std::vector<u32> &col_cell, const std::vector<u32> &col_start, uint64_t nnz, bool wait) {
	invalidate_prefetch();
	MatrixResult &M = mat[filtered_m ? 0 : 1];
	const u32 ncols = u32(col_cell.size());
	if (!ncols || !nnz) return;
	M.d_col_cell.ensure(ncols); M.d_col_start.ensure(ncols);
	M.d_row.ensure(nnz); M.d_val.ensure(nnz); M.narrow = 0; M.vals.n = 0;
	HIP_CHECK(hipMemcpyAsync(M.d_col_cell.p, col_cell.data(), size_t(ncols) * 4, hipMemcpyHostToDevice, stream));
	HIP_CHECK(hipMemcpyAsync(M.d_col_start.p, col_start.data(), size_t(ncols) * 4, hipMemcpyHostToDevice, stream));
	MatrixArgs a = matrix_source(M, filtered_m, reads_output);
	a.t_gene = M.d_row.p; a.t_val = M.d_val.p;
	timed(filtered_m ? "emit_matrix:cm" : "emit_matrix:cm_raw", double(nnz) * 20, [&] {
		hipLaunchKernelGGL(emit_matrix_kernel<0>, dim3(ncols), dim3(256), 0, stream, a);
	});
	if (wait) HIP_CHECK(stream_wait(stream));   // the host vectors must outlive their copies (wait = false: the caller keeps them until the stream has drained)
}

// ResultsPrinter::get_count_matrix_filtered(container, query_marks) (ResultsPrinter.cpp:333-361) for a query other than
// the container's own: columns = the filtered cells, values = UMIs (reads) of each gene whose mark matches, zero
// entries dropped (Cell::requested_umis_per_gene, Cell.cpp:54-68).
void dropest_ctx::emit_matrix_levels(u32 mask, bool reads_output) {
	HostStage hs(this, "matrix:levels");
	MatrixResult &M = mat[2];
	M.colptr.assign(1, 0); M.nnz = 0; M.ncols = 0;
	filtered_cells();
	std::vector<u32> col_cell;
	for (u32 ri : filtered_ridx) col_cell.push_back(real[ri].id);
	const u32 ncols = u32(col_cell.size());
	M.ncols = ncols;
	M.colptr.assign(size_t(ncols) + 1, 0);
	if (!ncols || !n_cg) return;
	DevBuf<u32> d_value, d_count;
	d_value.alloc(n_cg); d_count.alloc(ncols);
	hipLaunchKernelGGL(cg_requested_by_mask_kernel, dim3(div_up(n_cg, 256)), dim3(256), 0, stream, cg_mol_begin.p, n_cg, mol_mark.p, mol_reads.p,
	                   mask, reads_output ? 1 : 0, d_value.p);
	HIP_CHECK(hipGetLastError());
	// groups rewritten by a UMI merge on the host: their molecules live in the override map
	for (auto const &kv : umi_overrides) {
		const u32 cell = u32(kv.first >> layout.gene_bits);
		u32 cgb = 0, cgc = 0;
		HIP_CHECK(hipMemcpy(&cgb, cell_cg_begin.p + cell, 4, hipMemcpyDeviceToHost));
		HIP_CHECK(hipMemcpy(&cgc, cell_cg_count.p + cell, 4, hipMemcpyDeviceToHost));
		std::vector<u64> keys(cgc);
		HIP_CHECK(hipMemcpy(keys.data(), cg_key.p + cgb, size_t(cgc) * 8, hipMemcpyDeviceToHost));
		for (u32 j = 0; j < cgc; ++j) {
			if (keys[j] != kv.first) continue;
			u32 v = 0;
			for (const UmiOverride &o : kv.second) if ((mask >> (o.mark & 7u)) & 1u) v += reads_output ? o.reads : 1u;
			HIP_CHECK(hipMemcpy(d_value.p + cgb + j, &v, 4, hipMemcpyHostToDevice));
		}
	}
	M.d_col_cell.ensure(ncols); M.d_col_start.ensure(ncols);
	MatrixArgs a = matrix_source(M, true, reads_output);
	a.value = d_value.p; a.skip_zero = 1;   // the values of this query, not the container's own
	HIP_CHECK(hipMemcpyAsync(M.d_col_cell.p, col_cell.data(), size_t(ncols) * 4, hipMemcpyHostToDevice, stream));
	hipLaunchKernelGGL(count_nonzero_rows_kernel, dim3(div_up(ncols, 256)), dim3(256), 0, stream, a.col_cell, ncols, a.cell_cg_begin, a.cell_cg_count, a.cg_key, a.gene_mask,
	                   a.value, d_count.p);
	HIP_CHECK(hipGetLastError());
	std::vector<u32> cnt(ncols);
	fetch(cnt.data(), d_count.p, size_t(ncols) * 4);
	uint64_t nnz = 0;
	for (u32 c = 0; c < ncols; ++c) { M.colptr[c] = u32(nnz); nnz += cnt[c]; }
	M.colptr[ncols] = checked_nnz(nnz);
	M.nnz = nnz;
	if (!nnz) return;
	M.d_row.ensure(nnz); M.d_val.ensure(nnz); M.h_row.ensure(nnz); M.h_val.ensure(nnz);
	HIP_CHECK(hipMemcpyAsync(M.d_col_start.p, M.colptr.data(), size_t(ncols) * 4, hipMemcpyHostToDevice, stream));
	a.t_gene = M.d_row.p; a.t_val = M.d_val.p;
	hipLaunchKernelGGL(emit_matrix_kernel<0>, dim3(ncols), dim3(256), 0, stream, a);
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipMemcpyAsync(M.h_row.p, M.d_row.p, nnz * 4, hipMemcpyDeviceToHost, stream));
	HIP_CHECK(hipMemcpyAsync(M.h_val.p, M.d_val.p, nnz * 4, hipMemcpyDeviceToHost, stream));
	HIP_CHECK(stream_wait(stream));
}

// ================================================================================================
// C-ABI of the count matrices
// ================================================================================================
// The tail of the two widen entry points: the job runs on the pool with the calling thread taking part; when this returns the caller's
// arrays are its own again.  (The knobs are read at every call: tests run small slices with workers that nap between claiming a slice and
// walking it.)  name / bad_row / bad_value: the texts of the entry point's errors.
static void run_widen_job(const std::shared_ptr<dropest::DecodeJob> &job, const char *name, const char *bad_row, const char *bad_value) {
	using dropest::DecodeJob;
	(void)hipGetDevice(&job->device);
	(void)hipGetLastError();   // (no device: the walk needs none)
	const char *e_slice = getenv("DROPEST_DECODE_SLICE"), *e_delay = getenv("DROPEST_DECODE_TEST_DELAY_US");
	if (e_delay) job->test_delay_us = uint32_t(std::max(0, atoi(e_delay)));
	job->prepare(e_slice && atoll(e_slice) >= 64 ? uint64_t(atoll(e_slice)) : uint64_t(1) << 16);
	dropest::DecodePool::get().submit(job);
	job->work(true);
	const int st = job->finish_rider();   // (= wait() for a matrix that is no rider)
	job->quiesce();
	// every slice is counted exactly once, by whoever finished it first: a second count would have ended the job one slice early
	if (!job->derived && st == DecodeJob::DONE && job->slice_done.load() != uint32_t(job->slice_end.size()))
		throw DeviceError(std::string(name) + ": internal: " + std::to_string(job->slice_done.load()) + " slices counted, " + std::to_string(job->slice_end.size()) + " exist");
	if (st == DecodeJob::BAD_ROW) throw InvalidError(std::string(name) + ": " + bad_row);
	if (st == DecodeJob::BAD_VALUE) throw InvalidError(std::string(name) + ": " + bad_value);
	if (st != DecodeJob::DONE) throw InvalidError(std::string(name) + ": the decode failed");
}

extern "C" {

dropest_status dropest_count_matrix_csc(dropest_ctx *ctx, int filtered, int reads_output, uint64_t *ncols, uint64_t *nnz,
                                        const uint32_t **colptr, const uint32_t **rowidx, const uint32_t **values) {
	return guarded([&] {
		need_init(ctx);
		ctx->emit_matrix(filtered != 0, reads_output != 0);
		const dropest_ctx::MatrixResult &M = ctx->mat[filtered ? 0 : 1];
		*ncols = M.ncols; *nnz = M.nnz;
		*colptr = M.colptr.data(); *rowidx = M.h_row.p; *values = M.h_val.p;
	});
}

dropest_status dropest_prefetch_raw_matrix(dropest_ctx *ctx, int reads_output) {
	return guarded([&] {
		need_init(ctx);
		ctx->prefetch_raw_matrix(reads_output != 0, 0);
	});
}

dropest_status dropest_prefetch_raw_matrix_narrow(dropest_ctx *ctx, int reads_output) {
	return guarded([&] {
		need_init(ctx);
		ctx->prefetch_raw_matrix(reads_output != 0, 1);
	});
}

dropest_status dropest_prefetch_raw_matrix_bytes(dropest_ctx *ctx, int reads_output) {
	return guarded([&] {
		need_init(ctx);
		ctx->prefetch_raw_matrix(reads_output != 0, 2);
	});
}

dropest_status dropest_narrow_matrix_possible(dropest_ctx *ctx, int *possible) {
	return guarded([&] { need_init(ctx); if (!possible) throw InvalidError("null argument"); *possible = ctx->narrow_possible() ? 1 : 0; });
}

dropest_status dropest_count_matrix_csc_narrow(dropest_ctx *ctx, int filtered, int reads_output, uint64_t *ncols, uint64_t *nnz,
                                               const uint32_t **colptr, const uint16_t **rowidx, const uint16_t **values,
                                               uint64_t *n_overflow, const uint32_t **overflow_pos, const uint32_t **overflow_val) {
	return guarded([&] {
		need_init(ctx);
		if (!ncols || !nnz || !colptr || !rowidx || !values || !n_overflow || !overflow_pos || !overflow_val) throw InvalidError("null argument");
		ctx->emit_matrix(filtered != 0, reads_output != 0, true, 1);
		const dropest_ctx::MatrixResult &M = ctx->mat[filtered ? 0 : 1];
		*ncols = M.ncols; *nnz = M.nnz;
		*colptr = M.colptr.data(); *rowidx = M.h_row16.p; *values = M.h_val16.p;
		*n_overflow = M.vals.n; *overflow_pos = M.vals.h_pos(); *overflow_val = M.vals.h_val();
	});
}

dropest_status dropest_set_raw_matrix_prefetch(dropest_ctx *ctx, int form, int reads_output) {
	return guarded([&] {
		if (!ctx) throw InvalidError("null context");
		if (form < -1 || form > 2) throw InvalidError("form: -1 (off), 0 (32-bit), 1 (16-bit), 2 (bytes)");
		ctx->auto_pf_form = form; ctx->auto_pf_reads = reads_output != 0;
	});
}

dropest_status dropest_set_matrix_wire(dropest_ctx *ctx, int enabled) {
	return guarded([&] {
		if (!ctx) throw InvalidError("null context");
		ctx->invalidate_prefetch();
		ctx->matrix_wire = enabled != 0;
	});
}

dropest_status dropest_count_matrix_csc_bytes(dropest_ctx *ctx, int filtered, int reads_output, dropest_matrix_bytes *out) {
	return guarded([&] {
		need_init(ctx);
		if (!out) throw InvalidError("null argument");
		ctx->emit_matrix(filtered != 0, reads_output != 0, true, 2);
		const dropest_ctx::MatrixResult &M = ctx->mat[filtered ? 0 : 1];
		out->ncols = M.ncols; out->nnz = M.nnz; out->colptr = M.colptr.data();
		out->row_delta = M.h_drow8.p; out->value = M.h_val8.p;
		out->n_row_listed = M.rows.n; out->row_listed_pos = M.rows.h_pos(); out->row_listed_row = M.rows.h_val();
		out->n_value_listed = M.vals.n; out->value_listed_pos = M.vals.h_pos(); out->value_listed_value = M.vals.h_val();
	});
}

// dgCMatrix slots i / x from the byte form.  The listed entries come in no particular order: they are written to their places first, then
// every column is walked once (a column's first delta counts from row -1; a 255 takes what the first phase put there).  The walk is the one
// dropest_count_matrix_csc runs under its copies (matrix_decode.h), here with everything already on the host; the calling thread takes part.
dropest_status dropest_matrix_bytes_widen(const dropest_matrix_bytes *m, uint32_t *rowidx, uint32_t *values) {
	return guarded([&] {
		if (!m || (m->nnz && (!rowidx || !values))) throw InvalidError("null argument");
		if (!m->nnz) return;
		if (m->n_row_listed > 0xFFFFFFFFull || m->n_value_listed > 0xFFFFFFFFull) throw InvalidError("byte matrix: a list longer than the matrix");
		auto job = std::make_shared<dropest::DecodeJob>();
		job->m.rd = m->row_delta; job->m.vb = m->value; job->m.colptr = m->colptr; job->m.ncols = m->ncols; job->m.nnz = m->nnz;
		job->ro = rowidx; job->vo = values;
		const uint32_t nr = uint32_t(m->n_row_listed), nv = uint32_t(m->n_value_listed);
		job->r_count = &nr; job->r_pos = m->row_listed_pos; job->r_val = m->row_listed_row; job->rcap = nr;
		job->v_count = &nv; job->v_pos = m->value_listed_pos; job->v_val = m->value_listed_value; job->vcap = nv;
		job->check_marks = true;
		run_widen_job(job, "byte matrix", "a listed row does not stand on a 255", "a listed value does not stand on a 255");
	});
}

dropest_status dropest_matrix_rider_widen(const dropest_matrix_bytes *base, const uint32_t *base_rows, const uint8_t *value, const uint32_t *out_begin,
                                          const uint32_t *out_count, uint64_t rider_nnz, uint64_t n_listed, const uint32_t *listed_pos,
                                          const uint32_t *listed_value, uint32_t *rowidx, uint32_t *values) {
	return guarded([&] {
		if (!base || (base->nnz && (!base_rows || !value)) || (base->ncols && (!out_begin || !out_count)) || (rider_nnz && (!rowidx || !values)) ||
		    (n_listed && (!listed_pos || !listed_value))) throw InvalidError("null argument");
		if (n_listed > 0xFFFFFFFFull || rider_nnz > 0xFFFFFFF0ull) throw InvalidError("rider matrix: too many entries");
		if (!base->nnz || !rider_nnz) return;
		auto job = std::make_shared<dropest::DecodeJob>();
		job->m.rd = base->row_delta; job->m.vb = value; job->m.colptr = base->colptr; job->m.ncols = base->ncols; job->m.nnz = rider_nnz;
		job->ro = rowidx; job->vo = values;
		const uint32_t nv = uint32_t(n_listed);
		job->v_count = &nv; job->v_pos = listed_pos; job->v_val = listed_value; job->vcap = nv;
		job->derived = true;
		job->dv.base_ro = base_rows; job->dv.out_begin = out_begin; job->dv.out_count = out_count;
		run_widen_job(job, "rider matrix", "a column keeps another number of entries than announced", "a listed value lies outside the matrix");
	});
}

dropest_status dropest_count_matrix_csc_levels(dropest_ctx *ctx, const char *gene_match_levels, int reads_output, uint64_t *ncols,
                                               uint64_t *nnz, const uint32_t **colptr, const uint32_t **rowidx, const uint32_t **values) {
	return guarded([&] {
		need_init(ctx);
		if (!gene_match_levels) throw InvalidError("null gene_match_levels");
		ctx->emit_matrix_levels(query_mask_from_code(gene_match_levels), reads_output != 0);
		const dropest_ctx::MatrixResult &M = ctx->mat[2];
		*ncols = M.ncols; *nnz = M.nnz;
		*colptr = M.colptr.data(); *rowidx = M.h_row.p; *values = M.h_val.p;
	});
}

dropest_status dropest_count_matrix(dropest_ctx *ctx, int filtered, int reads_output, uint64_t *nnz, uint32_t *gene,
                                    uint32_t *col, uint32_t *val) {
	return guarded([&] {
		need_init(ctx);
		ctx->emit_matrix(filtered != 0, reads_output != 0);
		const dropest_ctx::MatrixResult &M = ctx->mat[filtered ? 0 : 1];
		*nnz = M.nnz;
		if (gene && col && val) {
			for (uint64_t c = 0; c < M.ncols; ++c)
				for (u32 k = M.colptr[c]; k < M.colptr[c + 1]; ++k) { gene[k] = M.h_row.p[k]; col[k] = u32(c); val[k] = M.h_val.p[k]; }
		}
	});
}

}  // extern "C"
