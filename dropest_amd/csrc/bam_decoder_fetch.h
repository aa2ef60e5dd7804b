// bam_decoder_fetch.h -- what the caller may ask of the last finished window of the device decoder: records byte by byte, the dense columns, the
// quality rows, and its own answers patched into the dense columns
#pragma once

__global__ __launch_bounds__(256) void bam_record_sizes_kernel(const uint8_t *__restrict__ data, const uint64_t *__restrict__ rec_off, const uint32_t *__restrict__ idx, uint32_t n,
                                                               uint32_t *__restrict__ size) {
	const uint32_t k = blockIdx.x * 256 + threadIdx.x;
	if (k < n) size[k] = 4u + b_le32(data + rec_off[idx[k]]);
}

// (The indices, sizes, offsets and the gathered bytes go through pinned memory that the kernels read and write themselves: the five copies this call
// used to make were 17 KB to 1 MB each -- sizes at which a hipMemcpyAsync out of or into pageable memory is staged, and took 8 ms whenever the
// staging grew: 3.3 -> 12.4 ms per file once the second window was 8 MB.)
extern "C" int dropest_bam_decoder_fetch_records(dropest_bam_decoder *d, const uint32_t *idx, uint32_t n, uint8_t *dst, uint64_t dst_cap, uint64_t *dst_off) {
	return bgzf_guarded([&] {
		if (!d || (n && (!idx || !dst || !dst_off))) throw InvalidError("null argument");
		if (!n) return;
		HIP_CHECK(hipSetDevice(d->device));
		bam_ready(d);
		for (uint32_t k = 0; k < n; ++k) if (idx[k] >= d->at.last_n_rec) throw RangeError("record index outside the window");
		BamGather &G = d->gather;
		G.h_idx.ensure(n); G.h_off.ensure(n); G.h_size.ensure(n);
		std::memcpy(G.h_idx.p, idx, size_t(n) * 4);
		hipLaunchKernelGGL(bam_record_sizes_kernel, dim3((n + 255) / 256), dim3(256), 0, d->stream, d->last().data(), d->rec.off.p, G.h_idx.p, n, G.h_size.p);
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipStreamSynchronize(d->stream));
		uint64_t total = 0;
		for (uint32_t k = 0; k < n; ++k) { dst_off[k] = total; G.h_off.p[k] = total; total += G.h_size.p[k]; }
		if (total > dst_cap) throw InvalidError("destination too small: " + std::to_string(total) + " bytes needed");
		G.h_bytes.ensure(total + total / 4 + 64);
		hipLaunchKernelGGL(bam_gather_records_kernel, dim3((n + 3) / 4), dim3(256), 0, d->stream, d->last().data(), d->rec.off.p, G.h_idx.p, G.h_off.p, n, G.h_bytes.p);
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipStreamSynchronize(d->stream));
		std::memcpy(dst, G.h_bytes.p, total);
	});
}

extern "C" int dropest_bam_decoder_columns_to_host(dropest_bam_decoder *d, uint64_t *cb, uint64_t *umi, uint32_t *gene, uint32_t *aux) {
	return bgzf_guarded([&] {
		if (!d) throw InvalidError("null argument");
		const uint64_t n = d->at.last_n_ok;
		if (!n) return;
		HIP_CHECK(hipSetDevice(d->device));
		bam_ready(d);
		if (cb) HIP_CHECK(hipMemcpyAsync(cb, d->dense.cb.p, n * 8, hipMemcpyDeviceToHost, d->stream));
		if (umi) HIP_CHECK(hipMemcpyAsync(umi, d->dense.umi.p, n * 8, hipMemcpyDeviceToHost, d->stream));
		if (gene) HIP_CHECK(hipMemcpyAsync(gene, d->dense.gene.p, n * 4, hipMemcpyDeviceToHost, d->stream));
		if (aux) HIP_CHECK(hipMemcpyAsync(aux, d->dense.aux.p, n * 4, hipMemcpyDeviceToHost, d->stream));
		HIP_CHECK(hipStreamSynchronize(d->stream));
	});
}

extern "C" int dropest_bam_decoder_quality_rows(dropest_bam_decoder *d, uint32_t ql, const uint8_t **rows) {
	return bgzf_guarded([&] {
		if (!d || !rows || !ql || ql > 255) throw InvalidError("bad argument");
		*rows = nullptr;
		const uint64_t n = d->at.last_n_ok;
		if (!n) return;
		HIP_CHECK(hipSetDevice(d->device));
		bam_ready(d);
		BamDenseColumns &C = d->dense;
		C.qual.ensure(n * ql + n * ql / 4); C.h_qual.ensure(n * ql);
		hipLaunchKernelGGL(bam_quality_rows_kernel, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, d->stream, d->last().data(), d->src.table ? d->src.table->text.p : (const uint8_t *)nullptr, C.qoff.p, uint32_t(n), ql, C.qual.p);
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipMemcpyAsync(C.h_qual.p, C.qual.p, n * ql, hipMemcpyDeviceToHost, d->stream));
		HIP_CHECK(hipStreamSynchronize(d->stream));
		*rows = C.h_qual.p;
	});
}

extern "C" int dropest_bam_decoder_patch(dropest_bam_decoder *d, const uint32_t *pos, const uint64_t *cb, const uint64_t *umi, const uint32_t *gene,
                                         const uint32_t *aux, uint32_t n) {
	return bgzf_guarded([&] {
		if (!d || (n && (!pos || !cb || !umi || !gene || !aux))) throw InvalidError("null argument");
		if (!n) return;
		HIP_CHECK(hipSetDevice(d->device));
		bam_ready(d);
		for (uint32_t k = 0; k < n; ++k) if (pos[k] >= d->at.last_n_ok) throw RangeError("row outside the dense columns");
		// (the caller's five arrays into one pinned buffer that the kernel reads itself: no staged copies)
		PinnedBuf<uint64_t> &P = d->gather.h_patch;
		P.ensure(size_t(n) * 4 + 8);      // words of 8 bytes: cb | umi | pos, gene, aux
		size_t at = 0;
		const char *const what = "the patches' staging";
		const auto *const q_cb = pinned_put(P, at, reinterpret_cast<const unsigned long long *>(cb), n, what), *const q_umi = pinned_put(P, at, reinterpret_cast<const unsigned long long *>(umi), n, what);
		const uint32_t *const q_pos = pinned_put(P, at, pos, n, what), *const q_gene = pinned_put(P, at, gene, n, what), *const q_aux = pinned_put(P, at, aux, n, what);
		hipLaunchKernelGGL(bam_patch_kernel, dim3((n + 255) / 256), dim3(256), 0, d->stream, q_pos, q_cb, q_umi, q_gene, q_aux, n, d->dense.args());
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipStreamSynchronize(d->stream));
	});
}

// -r: for records rec_idx[0 .. n) of the LAST window (NULL: its first n records) the row of the read-parameter table each was SERVED -- a row that
// fails the quality filter too, which the record took and is "low quality" for; 0xFFFFFFFF for every other record
extern "C" int dropest_bam_decoder_param_rows(dropest_bam_decoder *d, const uint32_t *rec_idx, uint32_t n, uint32_t *out_rows) {
	return bgzf_guarded([&] {
		if (!d || (n && !out_rows)) throw InvalidError("null argument");
		if (!d->src.table) throw InvalidError("no read-parameter table was given to this decoder");
		if (!n) return;
		const uint64_t n_rec = d->at.last_n_rec;
		if (!rec_idx && n > n_rec) throw RangeError("record index outside the window");
		for (uint32_t k = 0; rec_idx && k < n; ++k) if (rec_idx[k] >= n_rec) throw RangeError("record index outside the window");
		HIP_CHECK(hipSetDevice(d->device));
		bam_ready(d);
		PinnedBuf<uint32_t> &H = d->src.h_rp_row;
		H.ensure(n_rec);
		bam_copy(d->stream, uint32_t(n_rec), to_host(d->src.rp_row.p, H.p));
		HIP_CHECK(hipStreamSynchronize(d->stream));
		for (uint32_t k = 0; k < n; ++k) out_rows[k] = H.p[rec_idx ? rec_idx[k] : k];
	});
}
