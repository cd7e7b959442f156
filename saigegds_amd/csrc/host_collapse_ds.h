// host_collapse_ds.h -- the pseudo-variants of groups of resident dosage rows (kern_collapse_ds.h):
// sgx_ds_block_collapse appends them to the block, counts them as a load does and scans them as sgx_dsblock_scan does.
// The checks of a call's groups are those of sgx_collapse_2bit (host_collapse.h, tested on their own).
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.

extern "C" int sgx_ds_block_collapse(sgx_handle *h, sgx_dsblock *b, size_t n_groups, const int64_t *grp_ptr,
	const int32_t *var_idx, const uint8_t *flip, int32_t *n_valid, double *sum, int64_t *sum_trunc, double *out8,
	uint8_t *valid, void *out_rows)
{
	const char *who = "sgx_ds_block_collapse";
	int rc = dsblock_check(h, b, who);
	if (rc) return rc;
	if (h->owner) return fail(SGX_EINVAL, "%s: not on a twin", who);
	if (n_groups == 0) return SGX_OK;
	if (!grp_ptr || !var_idx || !flip || !n_valid || !sum || !sum_trunc || !out8 || !valid)
		return fail(SGX_EINVAL, "%s: NULL buffer", who);
	if (b->M == 0) return fail(SGX_EINVAL, "%s: nothing loaded", who);
	const size_t M = b->M;
	if (n_groups > b->cap - M)
		return fail(SGX_EINVAL, "%s: %zu rows and %zu groups, the block holds up to %zu", who, M, n_groups, b->cap);
	size_t at;
	rc = collapse_fail(who, collapse_ptr_check(n_groups, grp_ptr, &at), at, M);
	if (rc) return rc;
	const size_t nnz = (size_t)grp_ptr[n_groups];
	rc = collapse_fail(who, collapse_idx_check(nnz, var_idx, M, &at), at, M);
	if (!rc) rc = begin_call(h);
	if (rc) return rc;

	// the groups to the device, then a workgroup per (group, slab); beyond 2^20 workgroups they loop
	TabLayout tl;
	const auto s_ptr = tl.add(n_groups + 1, grp_ptr);
	const auto s_idx = tl.add(nnz, var_idx);
	const auto s_flip = tl.add(nnz, flip);
	rc = grow(b->tabs, tl.bytes());
	if (!rc) rc = tabs_upload(b->tabs, h->stream, s_ptr, s_idx, s_flip);
	if (rc) return rc;
	HIPCHK(hipEventRecord(h->evk[0], h->stream));           // stats.ms_kernel of this call: the collapse kernel alone
	with_ds_rows(b->dtype, b->rows.p, [&](auto *rows, auto t) {
		using T = decltype(t);
		const size_t total = n_groups * (((size_t)b->N + COLLAPSE_DS_SLAB(T) - 1) / COLLAPSE_DS_SLAB(T));
		hipLaunchKernelGGL((collapse_ds_kernel<T>), dim3((unsigned)std::min(total, (size_t)1 << 20)), dim3(COLLAPSE_DS_BLOCK), 0,
			h->stream, const_cast<T *>(rows), b->N, M, n_groups, tl.at(b->tabs, s_ptr), tl.at(b->tabs, s_idx), tl.at(b->tabs, s_flip));
	});
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(h->evk[1], h->stream));
	h->evk_set = true;                                       // (read by the sync of the scan below, whose FP64 form sets none)
	// the new rows are rows of the block from here on: the load's counts, the scan's table (both wait for the stream)
	rc = dsblock_counts(h, b, M, n_groups, n_valid, sum, sum_trunc);
	if (!rc) rc = dsblock_scan_rows(h, b, M, n_groups, out8, valid);
	if (rc) return rc;
	if (out_rows) HIPCHK(hipMemcpy(out_rows, b->rows + M * b->row_bytes, n_groups * b->row_bytes, hipMemcpyDeviceToHost));
	return SGX_OK;
}
