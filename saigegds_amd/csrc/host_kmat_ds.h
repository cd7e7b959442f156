// host_kmat_ds.h -- SKAT and the conditional scan on an explicit GRM from the dosage rows of a resident sgx_dsblock
// (DESIGN.md 8i): sgx_ds_block_skat_kmat, sgx_ds_block_cond_kmat_set and sgx_ds_block_cond_kmat are the flows of
// sgx_skat_kmat_2bit, sgx_cond_kmat_set and sgx_cond_kmat_2bit (skk_units, ckm_install, ckm_chunk) with the block's rows
// as the column source: kern_kmat_ds.h fills A and the sums from the rows where they lie.  Nothing crosses PCIe but
// the entries' tables, the weights and the results.
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.

// The tables of n dosage entries in h->stage_pk: means [n], row indices [n], flips [n].  An entry whose mean is not
// finite is flagged in `bad` and gets a column of zeros (SKK_DS_ZERO), like a 2-bit entry with a non-finite table.
// var_idx == nullptr: the rows 0 .. n_idx - 1 (a chunk's own numbering) instead of one index per entry.
static int kds_tables(const char *who, sgx_handle *h, size_t n, const int32_t *var_idx, size_t n_idx, const uint8_t *flip,
	const double *mean, std::vector<uint8_t> &bad, const sgx_dsblock *b, SkkSrc &src)
{
	std::vector<double> mean_ok(mean, mean + n);
	std::vector<uint8_t> flip_ok(n);
	bad.assign(n, 0);
	for (size_t e = 0; e < n; e++) {
		bad[e] = !std::isfinite(mean[e]);
		flip_ok[e] = bad[e] ? SKK_DS_ZERO : (flip[e] != 0);
		if (bad[e]) mean_ok[e] = 0;
	}
	std::vector<int32_t> iota;
	if (!var_idx) {
		iota.resize(n_idx);
		for (size_t j = 0; j < n_idx; j++) iota[j] = (int32_t)j;
		var_idx = iota.data();
	}
	TabLayout tl;
	const auto s_mean = tl.add(n, mean_ok.data());
	const auto s_idx = tl.add(n_idx, var_idx);
	const auto s_flip = tl.add(n, flip_ok.data());
	int rc = dev_room(h->stage_pk, tl.bytes(), "the entries' tables", who);
	if (!rc) rc = tabs_upload(h->stage_pk, h->stream, s_mean, s_idx, s_flip);
	if (rc) return rc;
	HIPCHK(hipStreamSynchronize(h->stream));     // mean_ok, flip_ok and iota are locals
	src = SkkSrc();
	src.idx = tl.at(h->stage_pk, s_idx);
	src.ds = b->rows.p; src.ds_dtype = b->dtype == SGX_DS_U8 ? SGX_DS_U8 : SGX_DS_F64;
	src.flip = tl.at(h->stage_pk, s_flip);
	src.mean = tl.at(h->stage_pk, s_mean);
	return SGX_OK;
}

extern "C" int sgx_ds_block_skat_kmat(sgx_handle *h, sgx_kmat *km, const sgx_dsblock *b, size_t n_units,
	const int64_t *unit_ptr, const int32_t *var_idx, const uint8_t *flip, const double *mean, const double *w,
	const double *tau, int maxiter, double tol, double *score, double *cov, int32_t *iters)
{
	const char *who = "sgx_ds_block_skat_kmat";
	if (!h || !km || !b) return fail(SGX_EINVAL, "%s: NULL handle", who);
	if (!unit_ptr || !var_idx || !flip || !mean || !w || !tau || !score || !cov) return fail(SGX_EINVAL, "%s: NULL buffer", who);
	if (h->owner) return fail(SGX_EINVAL, "%s: not on a twin", who);
	int rc = dsblock_check(h, b, who);
	if (!rc) rc = skk_km_check(who, h, km);
	if (!rc) rc = skk_sigma_args(who, h->md.N, w, tau, maxiter);
	if (rc) return rc;
	if (b->M == 0) return fail(SGX_EINVAL, "%s: nothing loaded", who);
	if (n_units == 0) return SGX_OK;
	rc = skat_units_check(who, n_units, unit_ptr, var_idx, b->M);
	if (rc) return rc;
	const int64_t nnz = unit_ptr[n_units];
	if (nnz == 0) return SGX_OK;
	rc = begin_call(h);
	if (rc) return rc;
	auto t_col = std::chrono::steady_clock::now();
	h->skk_ms[0] = h->skk_ms[1] = h->skk_ms[2] = 0;
	int64_t m_max = 0;
	for (size_t u = 0; u < n_units; u++) m_max = std::max(m_max, unit_ptr[u + 1] - unit_ptr[u]);
	std::vector<uint8_t> bad;
	SkkSrc src;
	rc = skk_unit_room(who, h, (size_t)m_max);
	if (!rc) rc = kds_tables(who, h, (size_t)nnz, var_idx, (size_t)nnz, flip, mean, bad, b, src);
	if (rc) return rc;
	return skk_units(who, h, km, src, n_units, unit_ptr, bad, (size_t)m_max, w, tau, maxiter, tol, t_col, score, cov, iters);
}

extern "C" int sgx_ds_block_cond_kmat_set(sgx_handle *h, sgx_kmat *km, const sgx_dsblock *b, size_t n_cond,
	const int32_t *var_idx, const uint8_t *flip, const double *mean, const double *w, const double *tau, int maxiter,
	double tol, double *score_c, double *cov_cc, int32_t *iters_c)
{
	const char *who = "sgx_ds_block_cond_kmat_set";
	bool clear;
	int rc = ckm_set_args(who, h, km, n_cond, &clear);
	if (rc || clear) return rc;
	if (!b) return fail(SGX_EINVAL, "%s: NULL handle", who);
	if (!var_idx || !flip || !mean || !w || !tau || !score_c || !cov_cc) return fail(SGX_EINVAL, "%s: NULL buffer", who);
	rc = dsblock_check(h, b, who);
	if (!rc) rc = skk_km_check(who, h, km);
	if (!rc) rc = skk_sigma_args(who, h->md.N, w, tau, maxiter);
	if (rc) return rc;
	if (b->M == 0) return fail(SGX_EINVAL, "%s: nothing loaded", who);
	rc = block_idx_check(who, var_idx, n_cond, b->M);
	if (!rc) rc = sgx_sync(h);                   // nothing queued reads the set that is replaced
	if (!rc) rc = set_dev(h);
	if (rc) return rc;
	h->last_issued = h;
	auto t_col = std::chrono::steady_clock::now();
	h->skk_ms[0] = h->skk_ms[1] = h->skk_ms[2] = 0;
	rc = ckm_sum_room(who, h, n_cond);
	if (rc) return rc;
	h->ckm_n = 0;                                // from here on the old set is gone
	h->ckm_km = nullptr;
	SkkSrc src;
	rc = kds_tables(who, h, n_cond, var_idx, n_cond, flip, mean, h->ckm_bad, b, src);
	if (rc) return rc;
	return ckm_install(who, h, km, src, (int)n_cond, w, tau, maxiter, tol, t_col, score_c, cov_cc, iters_c);
}

extern "C" int sgx_ds_block_cond_kmat(sgx_handle *h, sgx_kmat *km, const sgx_dsblock *b, const uint8_t *flip,
	const double *mean, double *score, double *var, double *cov, int32_t *iters)
{
	const char *who = "sgx_ds_block_cond_kmat";
	int rc = ckm_scan_args(who, h, km);
	if (rc) return rc;
	if (!b) return fail(SGX_EINVAL, "%s: NULL handle", who);
	if (!flip || !mean || !score || !var || !cov) return fail(SGX_EINVAL, "%s: NULL buffer", who);
	rc = dsblock_check(h, b, who);
	if (!rc) rc = skk_km_check(who, h, km);
	if (rc) return rc;
	if (b->M == 0) return fail(SGX_EINVAL, "%s: nothing loaded", who);
	rc = begin_call(h);
	if (rc) return rc;
	h->skk_ms[0] = h->skk_ms[1] = h->skk_ms[2] = 0;
	auto t_col = std::chrono::steady_clock::now();

	const size_t M = b->M, C = (size_t)h->ckm_n;
	const size_t mc_max = std::min<size_t>(M, SGX_GRM_MAX_RHS);
	CkmScan cs;
	rc = ckm_sum_room(who, h, M);
	if (rc) return rc;
	std::vector<uint8_t> bad;
	SkkSrc all;
	rc = kds_tables(who, h, M, nullptr, mc_max, flip, mean, bad, b, all);         // a chunk's rows are 0 .. m - 1 of its own
	if (!rc) rc = ckm_scan_begin(who, h, km, mc_max, cs);
	if (rc) return rc;
	h->skk_ms[0] += skk_ms_since(t_col);
	for (size_t g0 = 0; g0 < M; g0 += SGX_GRM_MAX_RHS) {
		const int m = (int)std::min<size_t>(SGX_GRM_MAX_RHS, M - g0);
		SkkSrc src = all;
		src.ds = b->rows + g0 * b->row_bytes;
		src.flip += g0; src.mean += g0;
		rc = ckm_chunk(who, h, km, src, m, &bad[g0], cs, score + g0, var + g0, cov + g0 * C, iters ? iters + g0 : nullptr);
		if (rc) return rc;
	}
	return SGX_OK;
}
