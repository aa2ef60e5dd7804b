// bam_decoder_dict.h -- the host's dictionaries on their way to the device decoder: gene-name hashes and names, reference -> chromosome, with -g
// the annotation and its two tables (the state: BamDictionaries, bam_decoder.h)
#pragma once

// Host bytes to a device array without a staged copy: into the decoder's pinned staging (at `*at`, which moves on), then a kernel's loads.  The
// dictionaries' tables are 17 KB to a few hundred KB -- sizes at which hipMemcpyAsync out of pageable memory took 8-12 ms now and then (measured:
// "dictionaries to the device" 0.7 or 12 ms per file).  The caller waits for the stream before the staging is used again.
__global__ __launch_bounds__(256) void bam_bytes_from_host_kernel(const uint8_t *h, uint8_t *__restrict__ d, uint64_t n) {
	const uint64_t k = (uint64_t(blockIdx.x) * 256 + threadIdx.x) * 16;
	if (k + 16 <= n) { uint4 v; __builtin_memcpy(&v, h + k, 16); __builtin_memcpy(d + k, &v, 16); }
	else for (uint64_t i = k; i < n; ++i) d[i] = h[i];
}
static void bam_to_device(dropest_bam_decoder *d, void *dst, const void *src, size_t bytes, size_t &at) {
	if (!bytes) return;
	const uint8_t *const staged = pinned_put(d->dict.h_dict, at, static_cast<const uint8_t *>(src), bytes, "the dictionaries' staging", 16);
	hipLaunchKernelGGL(bam_bytes_from_host_kernel, dim3(uint32_t((bytes + 4095) / 4096)), dim3(256), 0, d->stream, staged, static_cast<uint8_t *>(dst), uint64_t(bytes));
	HIP_CHECK(hipGetLastError());
}

extern "C" int dropest_bam_decoder_set_annotation(dropest_bam_decoder *d, dropest_annotation *a, const int32_t *ann_chr_of_ref, uint32_t n_refs) {
	return bgzf_guarded([&] {
		if (!d || !a || (n_refs && !ann_chr_of_ref)) throw InvalidError("null argument");
		if (n_refs != uint32_t(d->cfg.n_refs)) throw InvalidError("one annotation chromosome per reference is expected");
		if (dropest_annotation_device(a) != d->device) throw InvalidError("the annotation lives on another GPU");
		HIP_CHECK(hipSetDevice(d->device));
		bam_ready(d);
		BamDictionaries &D = d->dict;
		D.annotation = a;
		D.n_ann_genes = dropest_annotation_genes(a);
		D.d_ann_chr.alloc(std::max<uint32_t>(n_refs, 1u));
		size_t at = 0;
		D.h_dict.ensure(size_t(n_refs) * 4 + 64);
		if (n_refs) bam_to_device(d, D.d_ann_chr.p, ann_chr_of_ref, size_t(n_refs) * 4, at);
		D.d_ann_id.alloc(std::max<uint32_t>(D.n_ann_genes, 1u));
		HIP_CHECK(hipMemsetAsync(D.d_ann_id.p, 0xFF, size_t(std::max<uint32_t>(D.n_ann_genes, 1u)) * 4, d->stream));   // no gene of the annotation is in the dictionary yet
		HIP_CHECK(hipStreamSynchronize(d->stream));
	});
}

extern "C" int dropest_bam_decoder_set_annotation_genes(dropest_bam_decoder *d, const int32_t *id_of_ann_gene, uint32_t n) {
	return bgzf_guarded([&] {
		if (!d || !d->dict.annotation || (n && !id_of_ann_gene)) throw InvalidError("no annotation was given to this decoder");
		if (n != d->dict.n_ann_genes) throw InvalidError("one entry per gene of the annotation is expected");
		HIP_CHECK(hipSetDevice(d->device));
		bam_ready(d);
		HIP_CHECK(hipStreamSynchronize(d->stream));
		if (n) { size_t at = 0; d->dict.h_dict.ensure(size_t(n) * 4 + 64); bam_to_device(d, d->dict.d_ann_id.p, id_of_ann_gene, size_t(n) * 4, at); HIP_CHECK(hipStreamSynchronize(d->stream)); }
	});
}

// The names of the genes in the dictionary, by index: name k = pool[off[k] .. off[k + 1]).  With them a record's gene is accepted on the device
// only if its bytes ARE the name the hash points at; a name that merely shares the FNV-1a value of another goes to the host (which interns it
// by its bytes, CellsDataContainer::intern_gene).  Call after dropest_bam_decoder_set_dictionaries, with every gene the dictionary holds.
extern "C" int dropest_bam_decoder_set_gene_names(dropest_bam_decoder *d, const uint32_t *off, const uint8_t *pool, uint32_t n_names) {
	return bgzf_guarded([&] {
		if (!d || (n_names && (!off || !pool))) throw InvalidError("null argument");
		HIP_CHECK(hipSetDevice(d->device));
		bam_ready(d);
		HIP_CHECK(hipStreamSynchronize(d->stream));
		BamDictionaries &D = d->dict;
		D.n_gene_names = 0;
		if (!n_names) return;
		D.g_name_off.ensure(size_t(n_names) + 1 + n_names / 4); D.g_name_pool.ensure(size_t(off[n_names]) + off[n_names] / 4 + 16);
		size_t at = 0;
		D.h_dict.ensure((size_t(n_names) + 1) * 4 + size_t(off[n_names]) + 128);
		bam_to_device(d, D.g_name_off.p, off, (size_t(n_names) + 1) * 4, at);
		if (off[n_names]) bam_to_device(d, D.g_name_pool.p, pool, off[n_names], at);
		HIP_CHECK(hipStreamSynchronize(d->stream));
		D.n_gene_names = n_names;
	});
}

extern "C" int dropest_bam_decoder_set_dictionaries(dropest_bam_decoder *d, const uint64_t *gene_hash, const uint32_t *gene_id, uint32_t n_genes,
                                                    const int32_t *chr_of_ref, uint32_t n_refs) {
	return bgzf_guarded([&] {
		if (!d || (n_genes && (!gene_hash || !gene_id)) || (n_refs && !chr_of_ref)) throw InvalidError("null argument");
		if (n_refs != uint32_t(d->cfg.n_refs)) throw InvalidError("the chromosome table does not have one entry per reference");
		HIP_CHECK(hipSetDevice(d->device));
		bam_ready(d);
		uint32_t cap = 1024;
		while (cap < n_genes * 2u + 16u) cap <<= 1;
		std::vector<unsigned long long> keys(cap, 0);
		std::vector<uint32_t> vals(cap, 0);
		for (uint32_t k = 0; k < n_genes; ++k) {
			uint32_t sl = bam_dict_slot(gene_hash[k], cap - 1);
			while (vals[sl] && keys[sl] != gene_hash[k]) sl = (sl + 1) & (cap - 1);
			if (!vals[sl]) { keys[sl] = gene_hash[k]; vals[sl] = gene_id[k] + 1; }      // (the first name with a hash keeps it, as the host's map does)
		}
		HIP_CHECK(hipStreamSynchronize(d->stream));
		BamDictionaries &D = d->dict;
		D.g_keys.ensure(cap); D.g_vals.ensure(cap);
		size_t at = 0;
		D.h_dict.ensure(size_t(cap) * 12 + size_t(n_refs) * 4 + 128);
		bam_to_device(d, D.g_keys.p, keys.data(), size_t(cap) * 8, at);
		bam_to_device(d, D.g_vals.p, vals.data(), size_t(cap) * 4, at);
		if (n_refs) bam_to_device(d, D.d_chr.p, chr_of_ref, size_t(n_refs) * 4, at);
		HIP_CHECK(hipStreamSynchronize(d->stream));
		D.g_mask = cap - 1;
	});
}

// -r: the records' barcodes, UMIs and UMI quality strings come from `table` (dropest_read_params_*, bam_read_params.h; built, on this GPU; it stays
// the caller's and outlives the decoder's use of it) by the read's name, each row serving the first record of the stream that asks for it.
// first_ordinal: the stream ordinal of the next window's first record -- above every ordinal that claimed a row of this table before (the records
// of the files read so far; 0 for the first file of a replay, dropest_read_params_replay_begin).  NULL turns the source off; so does a reset.  Not
// with -f (the tags win there).  A tagging decoder writes CR / UR / the UMI quality from the served row (bam_decoder_tag.h).
extern "C" int dropest_bam_decoder_set_read_params(dropest_bam_decoder *d, dropest_read_params *table, uint64_t first_ordinal) {
	return bgzf_guarded([&] {
		if (!d) throw InvalidError("null argument");
		if (!table) { d->src.table = nullptr; return; }
		if (!table->built) throw InvalidError("the read-parameter table was not built (dropest_read_params_build)");
		if (table->device != d->device) throw InvalidError("the read-parameter table lives on another GPU");
		if (d->cfg.filled_bam) throw InvalidError("read-parameter files are not looked at under -f (barcode and UMI come from the tags)");
		d->src.table = table; d->src.first_ordinal = first_ordinal; d->src.seen = 0;
	});
}

// -P: the gene of a record is its reference's name.  gene_of_ref[r] = the index of reference r's name in the caller's gene dictionary, -1 = not in
// it yet (a record on r comes back through need_*; call again once the dictionary has grown), -2 = the name is empty (no gene, mark 0).  The gene
// tag, the read type and an annotation are then not looked at.  NULL turns the source off; so does a reset.
extern "C" int dropest_bam_decoder_set_gene_of_reference(dropest_bam_decoder *d, const int32_t *gene_of_ref, uint32_t n_refs) {
	return bgzf_guarded([&] {
		if (!d) throw InvalidError("null argument");
		if (!gene_of_ref) { d->src.ref_gene = false; return; }
		if (n_refs != uint32_t(d->cfg.n_refs)) throw InvalidError("one gene per reference is expected");
		for (uint32_t r = 0; r < n_refs; ++r) if (gene_of_ref[r] < -2) throw InvalidError("a gene index below -2");
		HIP_CHECK(hipSetDevice(d->device));
		bam_ready(d);
		HIP_CHECK(hipStreamSynchronize(d->stream));
		d->src.gene_of_ref.ensure(std::max<uint32_t>(n_refs, 1u));
		if (n_refs) { size_t at = 0; d->dict.h_dict.ensure(size_t(n_refs) * 4 + 64); bam_to_device(d, d->src.gene_of_ref.p, gene_of_ref, size_t(n_refs) * 4, at); HIP_CHECK(hipStreamSynchronize(d->stream)); }
		d->src.ref_gene = true;
	});
}

// -P with tagged output: the references' names, name r = pool[off[r] .. off[r + 1]) (n + 1 offsets; host memory, copied), which the tag kernels
// write as the gene of a record on reference r.  A record whose reference id is not below n is flagged, not written (dropest_bam_decoder_tag_window
// then fails).  n = 0 drops the names; so does a reset.
extern "C" int dropest_bam_decoder_set_reference_names(dropest_bam_decoder *d, const uint32_t *off, const uint8_t *pool, uint32_t n_names) {
	return bgzf_guarded([&] {
		if (!d || (n_names && (!off || (off[n_names] && !pool)))) throw InvalidError("null argument");
		for (uint32_t r = 0; r < n_names; ++r) if (off[r] > off[r + 1]) throw InvalidError("the reference names' offsets must not decrease");
		HIP_CHECK(hipSetDevice(d->device));
		bam_ready(d);
		HIP_CHECK(hipStreamSynchronize(d->stream));
		BamSourceState &S = d->src;
		S.has_ref_names = false; S.n_ref_names = 0;
		if (!n_names) return;
		const uint32_t bytes = off[n_names];
		S.ref_off.ensure(size_t(n_names) + 1); S.ref_pool.ensure(size_t(bytes) + 16);
		size_t at = 0;
		d->dict.h_dict.ensure((size_t(n_names) + 1) * 4 + size_t(bytes) + 128);
		bam_to_device(d, S.ref_off.p, off, (size_t(n_names) + 1) * 4, at);
		if (bytes) bam_to_device(d, S.ref_pool.p, pool, bytes, at);
		HIP_CHECK(hipStreamSynchronize(d->stream));
		S.n_ref_names = n_names; S.has_ref_names = true;
	});
}
