// bam_read_params.h -- the read-parameter table of include/dropest_bgzf.h (dropest_read_params_*; the kernels: k_readparams.h).  An object of its
// own beside the decoders: a decoder is leased per file and per GPU, the table and its claims live as long as the caller's controller.
// Included by bgzf_api.hip in front of the decoder, which is handed one (dropest_bam_decoder_set_read_params, bam_decoder_dict.h).
// Every call works on the device's null stream and returns when its work is done; none may run while a window of a decoder that holds the
// table is in flight.
#pragma once

struct dropest_read_params {
	int device = 0;
	unsigned long long hash_mask = ~0ull;
	// what _add_text brought, until _build sends it: the text, every line's two ends in it, and the quality threshold of each call's lines
	std::vector<uint8_t> h_text;
	std::vector<unsigned long long> h_line_be;
	struct Lines { uint32_t first, n; int32_t min_phred; };
	std::vector<Lines> calls;
	DevBuf<uint8_t> text;
	DevBuf<unsigned long long> line_be, claim;
	DevBuf<unsigned long long> replay_claim;      // _replay_begin .. _replay_end: the claims of a second pass over the stream, `claim` untouched beside them
	bool replaying = false;
	unsigned long long text_len = 0;
	unsigned long long *claims() const { return replaying ? replay_claim.p : claim.p; }
	DevBuf<RpRow> rows;
	DevBuf<uint32_t> slots, canonical, counts;
	uint32_t n_rows = 0, mask = 63, h_counts[3] = {0, 0, 0};
	bool built = false;
	RpTable view() const { return RpTable{slots.p, mask, rows.p, text.p, claims(), hash_mask}; }
};

static dropest_read_params *rp_built(dropest_read_params *t) {
	if (!t) throw InvalidError("null argument");
	if (!t->built) throw InvalidError("the read-parameter table was not built (dropest_read_params_build)");
	HIP_CHECK(hipSetDevice(t->device));
	return t;
}

extern "C" int dropest_read_params_create(int device, int hash_bits, dropest_read_params **out) {
	return bgzf_guarded([&] {
		if (!out) throw InvalidError("null argument");
		int n_dev = 0;
		if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) throw DeviceError("no such GPU: the read-parameter table has no CPU implementation");
		auto *t = new dropest_read_params();
		t->device = device;
		if (hash_bits > 0 && hash_bits < 64) t->hash_mask = (1ull << hash_bits) - 1ull;
		*out = t;
	});
}

extern "C" int dropest_read_params_add_text(dropest_read_params *t, const uint8_t *text, uint64_t len, const uint64_t *line_off, uint64_t n_lines, int min_phred) {
	return bgzf_guarded([&] {
		if (!t || (len && !text) || (n_lines && !line_off)) throw InvalidError("null argument");
		if (t->built) throw InvalidError("the read-parameter table is built: no more text");
		if (uint64_t(t->h_line_be.size() / 2) + n_lines > 0xFFFFFFF0ull) throw UnsupportedError("more than 2^32 rows of read parameters");
		for (uint64_t k = 0; k < n_lines; ++k)
			if (line_off[k] > len || (k && line_off[k] < line_off[k - 1])) throw InvalidError("the line offsets must ascend inside the text");
		const unsigned long long base = t->h_text.size();
		t->calls.push_back({uint32_t(t->h_line_be.size() / 2), uint32_t(n_lines), int32_t(min_phred)});
		t->h_text.insert(t->h_text.end(), text, text + len);
		for (uint64_t k = 0; k < n_lines; ++k) { t->h_line_be.push_back(base + line_off[k]); t->h_line_be.push_back(base + (k + 1 < n_lines ? line_off[k + 1] : len)); }
	});
}

extern "C" int dropest_read_params_build(dropest_read_params *t) {
	return bgzf_guarded([&] {
		if (!t) throw InvalidError("null argument");
		if (t->built) throw InvalidError("the read-parameter table is built already");
		HIP_CHECK(hipSetDevice(t->device));
		const uint32_t n = uint32_t(t->h_line_be.size() / 2);
		if (n > (1u << 30)) throw UnsupportedError("more than 2^30 rows of read parameters");
		uint32_t cap = 64;                                // the power of two >= 2 x rows: at least as many empty slots as rows
		while (uint64_t(cap) < 2ull * n) cap <<= 1;
		t->text.alloc(t->h_text.size() + 16); t->line_be.alloc(size_t(n) * 2 + 2); t->rows.alloc(size_t(n) + 1); t->claim.alloc(size_t(n) + 1);
		t->canonical.alloc(size_t(n) + 1); t->slots.alloc(cap); t->counts.alloc(4);
		t->n_rows = n; t->mask = cap - 1; t->text_len = t->h_text.size();
		if (!t->h_text.empty()) HIP_CHECK(hipMemcpy(t->text.p, t->h_text.data(), t->h_text.size(), hipMemcpyHostToDevice));
		if (n) HIP_CHECK(hipMemcpy(t->line_be.p, t->h_line_be.data(), size_t(n) * 16, hipMemcpyHostToDevice));
		HIP_CHECK(hipMemset(t->slots.p, 0, size_t(cap) * 4));
		HIP_CHECK(hipMemset(t->counts.p, 0, 16));
		HIP_CHECK(hipMemset(t->claim.p, 0xFF, (size_t(n) + 1) * 8));
		for (const dropest_read_params::Lines &c : t->calls)
			if (c.n) hipLaunchKernelGGL(rp_rows_kernel, dim3((c.n + 255) / 256), dim3(256), 0, nullptr, t->text.p, t->line_be.p, c.first, c.n, c.min_phred, t->hash_mask, t->rows.p);
		if (n) {
			hipLaunchKernelGGL(rp_insert_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, t->view(), t->slots.p, n);
			hipLaunchKernelGGL(rp_canonical_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, t->view(), t->canonical.p, n, t->counts.p);
		}
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipMemcpy(t->h_counts, t->counts.p, 12, hipMemcpyDeviceToHost));
		HIP_CHECK(hipDeviceSynchronize());
		std::vector<uint8_t>().swap(t->h_text); std::vector<unsigned long long>().swap(t->h_line_be);      // (the caller keeps its own text)
		t->built = true;
	});
}

extern "C" int dropest_read_params_counts(dropest_read_params *t, uint64_t *rows, uint64_t *valid, uint64_t *malformed, uint64_t *repeated) {
	return bgzf_guarded([&] {
		rp_built(t);
		if (rows) *rows = t->n_rows;
		if (valid) *valid = t->h_counts[0];
		if (malformed) *malformed = t->h_counts[1];
		if (repeated) *repeated = t->h_counts[2];
	});
}

extern "C" int dropest_read_params_rows_to_host(dropest_read_params *t, uint64_t first, uint64_t n, dropest_read_params_row *out) {
	return bgzf_guarded([&] {
		static_assert(sizeof(dropest_read_params_row) == sizeof(RpRow) && sizeof(RpRow) == 80, "the C struct and the kernels' struct are one layout");
		rp_built(t);
		if (first > t->n_rows || n > t->n_rows - first) throw RangeError("rows outside the table");
		if (!n) return;
		if (!out) throw InvalidError("null argument");
		std::vector<uint32_t> canonical(n);
		HIP_CHECK(hipMemcpy(out, t->rows.p + first, size_t(n) * sizeof(RpRow), hipMemcpyDeviceToHost));
		HIP_CHECK(hipMemcpy(canonical.data(), t->canonical.p + first, size_t(n) * 4, hipMemcpyDeviceToHost));
		for (uint64_t k = 0; k < n; ++k) out[k].canonical = canonical[k];
	});
}

extern "C" int dropest_read_params_lookup(dropest_read_params *t, const uint8_t *name_pool, const uint64_t *name_off, uint64_t n, uint32_t *out_row) {
	return bgzf_guarded([&] {
		rp_built(t);
		if (!n) return;
		if (!name_off || !out_row || (name_off[n] && !name_pool)) throw InvalidError("null argument");
		if (n > 0xFFFFFFF0ull) throw UnsupportedError("more than 2^32 names in one look-up");
		for (uint64_t k = 0; k < n; ++k) if (name_off[k + 1] < name_off[k] || name_off[k + 1] - name_off[k] > 0xFFFFFFF0ull) throw InvalidError("the name offsets must ascend");
		DevBuf<uint8_t> pool; DevBuf<unsigned long long> off; DevBuf<uint32_t> row;
		pool.alloc(name_off[n] + 16); off.alloc(n + 1); row.alloc(n);
		if (name_off[n]) HIP_CHECK(hipMemcpy(pool.p, name_pool, name_off[n], hipMemcpyHostToDevice));
		HIP_CHECK(hipMemcpy(off.p, name_off, (n + 1) * 8, hipMemcpyHostToDevice));
		hipLaunchKernelGGL(rp_lookup_kernel, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, nullptr, t->view(), pool.p, off.p, uint32_t(n), row.p);
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipMemcpy(out_row, row.p, n * 4, hipMemcpyDeviceToHost));
	});
}

extern "C" int dropest_read_params_claims_to_host(dropest_read_params *t, uint64_t first, uint64_t n, uint64_t *out) {
	return bgzf_guarded([&] {
		rp_built(t);
		if (first > t->n_rows || n > t->n_rows - first) throw RangeError("rows outside the table");
		if (!n) return;
		if (!out) throw InvalidError("null argument");
		HIP_CHECK(hipDeviceSynchronize());
		HIP_CHECK(hipMemcpy(out, t->claims() + first, size_t(n) * 8, hipMemcpyDeviceToHost));
	});
}

extern "C" int dropest_read_params_reset_claims(dropest_read_params *t) {
	return bgzf_guarded([&] {
		rp_built(t);
		HIP_CHECK(hipDeviceSynchronize());
		HIP_CHECK(hipMemset(t->claims(), 0xFF, (size_t(t->n_rows) + 1) * 8));
		HIP_CHECK(hipDeviceSynchronize());
	});
}

// A second pass over the same stream (-F: the reference makes a new parser for write_filtered_bam_files, so every row serves afresh): from _begin to
// _end the table's claims are a fresh array, all ones, and the array that was current stays as it is beside it; _end puts it back.  Whatever reads
// or writes claims in between (a decoder's windows, _claims_to_host, _reset_claims) works on the fresh array.
extern "C" int dropest_read_params_replay_begin(dropest_read_params *t) {
	return bgzf_guarded([&] {
		rp_built(t);
		if (t->replaying) throw InvalidError("the read-parameter table is in a replay already (dropest_read_params_replay_end)");
		HIP_CHECK(hipDeviceSynchronize());
		t->replay_claim.ensure(size_t(t->n_rows) + 1);
		HIP_CHECK(hipMemset(t->replay_claim.p, 0xFF, (size_t(t->n_rows) + 1) * 8));
		HIP_CHECK(hipDeviceSynchronize());
		t->replaying = true;
	});
}

extern "C" int dropest_read_params_replay_end(dropest_read_params *t) {
	return bgzf_guarded([&] {
		rp_built(t);
		if (!t->replaying) throw InvalidError("the read-parameter table is not in a replay (dropest_read_params_replay_begin)");
		HIP_CHECK(hipDeviceSynchronize());
		t->replaying = false;
	});
}

extern "C" void dropest_read_params_destroy(dropest_read_params *t) {
	if (!t) return;
	(void)hipSetDevice(t->device);
	(void)hipDeviceSynchronize();
	delete t;
}
