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
	rc = begin_call(h);
	if (rc) return rc;
	const int N = b->N, P = h->md.P, C = 2 * h->md.K + 1;

	SkatPlan pl;
	skat_plan(pl, n_units, unit_ptr, C, (N + SKAT_DS_SLAB - 1) / SKAT_DS_SLAB);

	// device copies of the tables: entries, means, tiles, flips
	TabLayout tl;
	const auto s_idx = tl.add(nnz, var_idx);
	const auto s_mean = tl.add(nnz, mean);
	const auto s_til = tl.add(pl.tiles.size(), pl.tiles.data());
	const auto s_flip = tl.add(nnz, flip);
	rc = grow(const_cast<sgx_dsblock *>(b)->tabs, tl.bytes());
	if (!rc) rc = tabs_upload(b->tabs, h->stream, s_idx, s_mean, s_til, s_flip);
	if (rc) return rc;

	rc = skat_run(h, pl, n_units, unit_ptr, C, [&](size_t t0, size_t nt) {
		with_ds_rows(b->dtype, b->rows.p, [&](auto *rows, auto t) {
			hipLaunchKernelGGL((skat_gram_ds_kernel<decltype(t)>), dim3((unsigned)nt, (unsigned)pl.nslab), dim3(64), 0, h->stream,
				rows, N, tl.at(b->tabs, s_idx), tl.at(b->tabs, s_flip), tl.at(b->tabs, s_mean), h->md.F, P,
				tl.at(b->tabs, s_til) + t0, nt, SKAT_DS_SLAB, h->skat_part);
		});
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
