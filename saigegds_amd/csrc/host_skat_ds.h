// host_skat_ds.h -- the SKAT set test's score vector and covariance matrix per unit from the dosage rows
// of a resident sgx_dsblock: kern_skat_ds.h makes the Gram tiles and the dense sums from the rows where they lie, the
// plan, the slab sum and the step to S and Phi are those of sgx_skat_2bit (host_skat.h).
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.

static const int SKAT_DS_SLAB = 4096;       // samples per sample slab (a multiple of 64): cut by N alone

// sgx_ds_block_skat; `dense` keeps the entries' dense sums [entry][2K+1] for a caller that wants them
// (sgx_ds_block_cond_set).
static int skat_ds_block_host(sgx_handle *h, const sgx_dsblock *b, size_t n_units, const int64_t *unit_ptr,
	const int32_t *var_idx, const uint8_t *flip, const double *mean, double *score, double *cov, std::vector<double> &dense)
{
	int rc = dsblock_check(h, b, "sgx_ds_block_skat");
	if (rc) return rc;
	if (n_units == 0) return SGX_OK;
	if (!unit_ptr || !var_idx || !flip || !mean || !score || !cov)
		return fail(SGX_EINVAL, "sgx_ds_block_skat: NULL buffer");
	if (b->M == 0) return fail(SGX_EINVAL, "sgx_ds_block_skat: nothing loaded");
	rc = skat_units_check("sgx_ds_block_skat", n_units, unit_ptr, var_idx, b->M);
	if (rc) return rc;
	const int64_t nnz = unit_ptr[n_units];
	if (nnz == 0) return SGX_OK;
	rc = sync_lane(h);
	if (rc) return rc;
	h->last_issued = h;
	const int N = b->N, P = h->md.P, C = 2 * h->md.K + 1;

	SkatPlan pl;
	skat_plan(pl, n_units, unit_ptr, C, (N + SKAT_DS_SLAB - 1) / SKAT_DS_SLAB);
	const size_t T = pl.tiles.size();

	// device copies of the tables: entries, means, tiles, flips
	sgx_dsblock *bm = const_cast<sgx_dsblock *>(b);
	const size_t o_mean = ((size_t)nnz * sizeof(int) + 15) & ~(size_t)15;
	const size_t o_til = o_mean + (size_t)nnz * sizeof(double);
	const size_t o_flip = o_til + T * sizeof(SkatTile);
	rc = grow(bm->tabs, o_flip + (size_t)nnz);
	if (rc) return rc;
	static_assert(sizeof(int) == sizeof(int32_t), "var_idx");
	HIPCHK(hipMemcpyAsync(b->tabs, var_idx, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipMemcpyAsync(b->tabs + o_mean, mean, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipMemcpyAsync(b->tabs + o_til, pl.tiles.data(), T * sizeof(SkatTile), hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipMemcpyAsync(b->tabs + o_flip, flip, (size_t)nnz, hipMemcpyHostToDevice, h->stream));

	const int *d_idx = reinterpret_cast<const int *>(b->tabs.p);
	const double *d_mean = reinterpret_cast<const double *>(b->tabs + o_mean);
	const SkatTile *d_til = reinterpret_cast<const SkatTile *>(b->tabs + o_til);
	const uint8_t *d_flip = b->tabs + o_flip;
	rc = skat_run(h, pl, n_units, unit_ptr, C, [&](size_t t0, size_t nt) {
		const dim3 grid((unsigned)nt, (unsigned)pl.nslab);
		if (b->dtype == SGX_DS_U8)
			hipLaunchKernelGGL((skat_gram_ds_kernel<uint8_t>), grid, dim3(64), 0, h->stream,
				(const uint8_t *)b->rows, N, d_idx, d_flip, d_mean, h->md.F, P, d_til + t0, nt, SKAT_DS_SLAB, h->skat_part);
		else
			hipLaunchKernelGGL((skat_gram_ds_kernel<double>), grid, dim3(64), 0, h->stream,
				(const double *)b->rows.p, N, d_idx, d_flip, d_mean, h->md.F, P, d_til + t0, nt, SKAT_DS_SLAB, h->skat_part);
	}, dense, cov);
	if (rc) return rc;
	skat_finish(h->md, n_units, unit_ptr, dense, score, cov);
	return SGX_OK;
}

extern "C" int sgx_ds_block_skat(sgx_handle *h, const sgx_dsblock *b, size_t n_units, const int64_t *unit_ptr,
	const int32_t *var_idx, const uint8_t *flip, const double *mean, double *score, double *cov)
{
	std::vector<double> dense;
	return skat_ds_block_host(h, b, n_units, unit_ptr, var_idx, flip, mean, score, cov, dense);
}
