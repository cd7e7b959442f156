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
		for (size_t c = 0; c < n_cond; c++)
			if (var_idx[c] < 0 || (size_t)var_idx[c] >= b->M)
				return fail(SGX_EINVAL, "sgx_ds_block_cond_set: variant index %d outside the block's %zu rows", var_idx[c], b->M);
	}
	rc = sgx_sync(h);                           // nothing queued reads the set that is replaced
	if (rc) return rc;
	h->n_cond = 0;
	if (n_cond == 0) return SGX_OK;

	// S_C and Phi_CC: sgx_ds_block_skat on the set as one unit
	const int64_t unit_ptr[2] = {0, (int64_t)n_cond};
	std::vector<double> dense;
	rc = skat_ds_block_host(h, b, 1, unit_ptr, var_idx, flip, mean, score_c, cov_cc, dense);
	if (rc) return rc;

	// their c' and e sums, then B = (F[:, 0:2K+1] | mu2 o G_c | zeros)
	const int N = b->N, K = h->md.K, P = h->md.P, C = (int)n_cond, PB = 16 * ((2 * K + 1 + C + 15) / 16);
	std::vector<double> ce((size_t)C * 2 * K);
	for (int c = 0; c < C; c++)
		for (int a = 0; a < 2 * K; a++) ce[(size_t)c * 2 * K + a] = dense[(size_t)c * (2 * K + 1) + a];
	rc = grow(h->cond_ce, (size_t)SGX_COND_MAX * 2 * KMAX);
	if (rc) return rc;
	rc = grow(h->cond_B, (size_t)N * PB);
	if (rc) return rc;
	const size_t o_idx = (size_t)C * sizeof(double), o_flip = o_idx + (size_t)C * sizeof(int);      // means first
	rc = grow(h->stage_pk, o_flip + (size_t)C);
	if (rc) return rc;
	static_assert(sizeof(int) == sizeof(int32_t), "var_idx");
	HIPCHK(hipMemcpyAsync(h->stage_pk, mean, (size_t)C * sizeof(double), hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipMemcpyAsync(h->stage_pk + o_idx, var_idx, (size_t)C * sizeof(int), hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipMemcpyAsync(h->stage_pk + o_flip, flip, (size_t)C, hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipMemcpyAsync(h->cond_ce, ce.data(), ce.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
	const double *d_mean = reinterpret_cast<const double *>(h->stage_pk.p);
	const int *d_idx = reinterpret_cast<const int *>(h->stage_pk + o_idx);
	const size_t nel = (size_t)N * PB;
	const dim3 grid((unsigned)((nel + 255) / 256));
	if (b->dtype == SGX_DS_U8)
		hipLaunchKernelGGL((cond_build_ds_kernel<uint8_t>), grid, dim3(256), 0, h->stream,
			(const uint8_t *)b->rows, d_idx, h->stage_pk + o_flip, d_mean, C, h->md.F, P, N, PB, h->cond_B);
	else
		hipLaunchKernelGGL((cond_build_ds_kernel<double>), grid, dim3(256), 0, h->stream,
			(const double *)b->rows.p, d_idx, h->stage_pk + o_flip, d_mean, C, h->md.F, P, N, PB, h->cond_B);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(h->stream));
	h->n_cond = C;
	return SGX_OK;
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
	rc = sync_lane(h);
	if (rc) return rc;
	h->last_issued = h;

	// tables and results on the device: means, score, var, cov, then the flips
	const size_t M = b->M, C = (size_t)h->n_cond;
	const int N = b->N, P = h->md.P;
	const size_t o_flip = M * (3 + C) * sizeof(double);
	rc = grow(h->stage_pk, o_flip + M);
	if (rc) return rc;
	double *d_mean = reinterpret_cast<double *>(h->stage_pk.p), *d_s = d_mean + M, *d_v = d_s + M, *d_c = d_v + M;
	const uint8_t *d_flip = h->stage_pk + o_flip;
	HIPCHK(hipMemcpyAsync(d_mean, mean, M * sizeof(double), hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipMemcpyAsync(h->stage_pk + o_flip, flip, M, hipMemcpyHostToDevice, h->stream));
	rc = cond_run(h, h, M, COND_DS_SLAB_CH, [&](auto nct, dim3 grid, size_t off, size_t m) {
		constexpr int NCT = decltype(nct)::value;
		if (b->dtype == SGX_DS_U8)
			hipLaunchKernelGGL((cond_rect_ds_kernel<uint8_t, NCT>), grid, dim3(256), 0, h->stream,
				(const uint8_t *)b->rows + off * (size_t)N, N, m, d_flip + off, d_mean + off, h->md.F, P, h->cond_B, COND_DS_SLAB_CH,
				h->cond_part);
		else
			hipLaunchKernelGGL((cond_rect_ds_kernel<double, NCT>), grid, dim3(256), 0, h->stream,
				(const double *)b->rows.p + off * (size_t)N, N, m, d_flip + off, d_mean + off, h->md.F, P, h->cond_B, COND_DS_SLAB_CH,
				h->cond_part);
	}, d_s, d_v, d_c);
	if (rc) return rc;
	HIPCHK(hipMemcpyAsync(score, d_s, M * sizeof(double), hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipMemcpyAsync(var, d_v, M * sizeof(double), hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipMemcpyAsync(cov, d_c, M * C * sizeof(double), hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipStreamSynchronize(h->stream));
	return SGX_OK;
}
