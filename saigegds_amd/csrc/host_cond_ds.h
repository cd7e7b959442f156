// host_cond_ds.h -- the conditional scan ("Conditional analysis") on the dosage rows of a resident
// sgx_dsblock: sgx_ds_block_cond_set installs a set of conditioning variants that are rows of a loaded block (their S
// and Phi by sgx_ds_block_skat's own functions, the dense matrix B of kern_cond.h built from the rows where they lie)
// into the handle state sgx_cond_set fills, sgx_ds_block_cond makes score, variance and the covariances with the set
// for every resident row (kern_cond_ds.h, then the slab sum and the finish of sgx_cond_2bit: cond_run).
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.

extern "C" int sgx_ds_block_cond_set(sgx_handle *h, const sgx_dsblock *b, size_t n_cond, const int32_t *var_idx,
	const uint8_t *flip, const double *mean, double *score_c, double *cov_cc)
{
	int rc = dsblock_check(h, b, "sgx_ds_block_cond_set");
	if (rc) return rc;
	if (h->owner) return fail(SGX_EINVAL, "sgx_ds_block_cond_set: not on a twin");
	if (n_cond > SGX_COND_MAX)
		return fail(SGX_EINVAL, "sgx_ds_block_cond_set: %zu conditioning variants, at most %d are supported", n_cond, SGX_COND_MAX);
	if (n_cond) {
		if (!var_idx || !flip || !mean || !score_c || !cov_cc) return fail(SGX_EINVAL, "sgx_ds_block_cond_set: NULL buffer");
		if (b->M == 0) return fail(SGX_EINVAL, "sgx_ds_block_cond_set: nothing loaded");
		rc = block_idx_check("sgx_ds_block_cond_set", var_idx, n_cond, b->M);
	}
	if (!rc) rc = sgx_sync(h);                  // nothing queued reads the set that is replaced
	if (rc) return rc;
	h->n_cond = 0;
	if (n_cond == 0) return SGX_OK;

	// S_C and Phi_CC: sgx_ds_block_skat on the set as one unit
	const int64_t unit_ptr[2] = {0, (int64_t)n_cond};
	std::vector<double> dense;
	rc = skat_ds_block_host(h, b, 1, unit_ptr, var_idx, flip, mean, score_c, cov_cc, dense);
	if (rc) return rc;

	const int C = (int)n_cond;
	return cond_install(h, C, dense, [&](int PB, dim3 grid) -> int {
		TabLayout tl;
		const auto s_mean = tl.add(n_cond, mean);
		const auto s_idx = tl.add(n_cond, var_idx);
		const auto s_flip = tl.add(n_cond, flip);
		int rc = grow(h->stage_pk, tl.bytes());
		if (!rc) rc = tabs_upload(h->stage_pk, h->stream, s_mean, s_idx, s_flip);
		if (rc) return rc;
		with_ds_rows(b->dtype, b->rows.p, [&](auto *rows, auto t) {
			hipLaunchKernelGGL((cond_build_ds_kernel<decltype(t)>), grid, dim3(256), 0, h->stream, rows, tl.at(h->stage_pk, s_idx),
				tl.at(h->stage_pk, s_flip), tl.at(h->stage_pk, s_mean), C, h->md.F, h->md.P, b->N, PB, h->cond_B);
		});
		return SGX_OK;
	});
}

extern "C" int sgx_ds_block_cond(sgx_handle *h, const sgx_dsblock *b, const uint8_t *flip, const double *mean,
	double *score, double *var, double *cov)
{
	int rc = dsblock_check(h, b, "sgx_ds_block_cond");
	if (rc) return rc;
	if (h->owner) return fail(SGX_EINVAL, "sgx_ds_block_cond: not on a twin");
	if (!flip || !mean || !score || !var || !cov) return fail(SGX_EINVAL, "sgx_ds_block_cond: NULL buffer");
	if (b->M == 0) return fail(SGX_EINVAL, "sgx_ds_block_cond: nothing loaded");
	if (h->n_cond == 0) return fail(SGX_EINVAL, "sgx_ds_block_cond: no conditioning set (sgx_ds_block_cond_set)");
	rc = begin_call(h);
	if (rc) return rc;

	// tables and results on the device: means, score, var, cov, then the flips
	const size_t M = b->M, C = (size_t)h->n_cond;
	const int N = b->N, P = h->md.P;
	TabLayout tl;
	const auto s_mean = tl.add(M, mean);
	const auto s_s = tl.add<double>(M), s_v = tl.add<double>(M), s_c = tl.add<double>(M * C);
	const auto s_flip = tl.add(M, flip);
	rc = grow(h->stage_pk, tl.bytes());
	if (!rc) rc = tabs_upload(h->stage_pk, h->stream, s_mean, s_flip);
	if (rc) return rc;
	double *d_s = tl.at(h->stage_pk, s_s), *d_v = tl.at(h->stage_pk, s_v), *d_c = tl.at(h->stage_pk, s_c);
	rc = cond_run(h, h, M, COND_DS_SLAB_CH, [&](auto nct, dim3 grid, size_t off, size_t m) {
		with_ds_rows(b->dtype, b->rows.p, [&](auto *rows, auto t) {
			hipLaunchKernelGGL((cond_rect_ds_kernel<decltype(t), decltype(nct)::value>), grid, dim3(256), 0, h->stream,
				rows + off * (size_t)N, N, m, tl.at(h->stage_pk, s_flip) + off, tl.at(h->stage_pk, s_mean) + off, h->md.F, P, h->cond_B,
				COND_DS_SLAB_CH, h->cond_part);
		});
	}, d_s, d_v, d_c);
	if (rc) return rc;
	HIPCHK(hipMemcpyAsync(score, d_s, M * sizeof(double), hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipMemcpyAsync(var, d_v, M * sizeof(double), hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipMemcpyAsync(cov, d_c, M * C * sizeof(double), hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipStreamSynchronize(h->stream));
	return SGX_OK;
}
