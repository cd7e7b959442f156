// host_cond.h -- the conditional scan ("Conditional analysis"): sgx_cond_set installs a set of
// conditioning variants (their S and Phi by sgx_skat_2bit's own functions, the dense matrix B of kern_cond.h on the
// device), sgx_cond_2bit_dev makes score, variance and the covariances with the set for rows in device memory,
// sgx_cond_2bit is its wrapper for rows in host memory.
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.

static const size_t COND_PART_BYTES = (size_t)256 << 20;    // per-slab partial sums of one launch

static int cond_ncol(const sgx_handle *p) { return 2 * p->md.K + 1 + p->n_cond; }

// Installs a set of C conditioning variants whose S and Phi the caller has made with SKAT's functions on the set as one
// unit: from their dense sums [c][2K+1] the c' and e sums (cond_ce), then B = (F[:, 0:2K+1] | mu2 o G_c | zeros) by
// build(PB, grid), which queues the entry's build kernel (and the tables it reads) into h->cond_B on the handle's stream.
template <class Build>
static int cond_install(sgx_handle *h, int C, const std::vector<double> &dense, Build build)
{
	const int N = h->md.N, K = h->md.K, PB = 16 * ((2 * K + 1 + C + 15) / 16);
	std::vector<double> ce((size_t)C * 2 * K);
	for (int c = 0; c < C; c++)
		for (int a = 0; a < 2 * K; a++) ce[(size_t)c * 2 * K + a] = dense[(size_t)c * (2 * K + 1) + a];
	int rc = grow(h->cond_ce, (size_t)SGX_COND_MAX * 2 * KMAX);
	if (!rc) rc = grow(h->cond_B, (size_t)N * PB);
	if (rc) return rc;
	HIPCHK(hipMemcpyAsync(h->cond_ce, ce.data(), ce.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
	const size_t nel = (size_t)N * PB;
	rc = build(PB, dim3((unsigned)((nel + 255) / 256)));
	if (rc) return rc;
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(h->stream));
	h->n_cond = C;
	return SGX_OK;
}

extern "C" int sgx_cond_set(sgx_handle *h, const uint8_t *packed_c, size_t bpv, size_t n_cond,
	const double *lut_c, double *score_c, double *cov_cc)
{
	if (!h) return fail(SGX_EINVAL, "sgx_cond_set: NULL handle");
	if (h->owner) return fail(SGX_EINVAL, "sgx_cond_set: not on a twin");
	if (n_cond > SGX_COND_MAX)
		return fail(SGX_EINVAL, "sgx_cond_set: %zu conditioning variants, at most %d are supported", n_cond, SGX_COND_MAX);
	if (n_cond && (!packed_c || !lut_c || !score_c || !cov_cc)) return fail(SGX_EINVAL, "sgx_cond_set: NULL buffer");
	const int N = h->md.N;
	int rc = n_cond ? bpv_check(bpv, N) : SGX_OK;
	if (!rc) rc = sgx_sync(h);                  // nothing queued reads the set that is replaced
	if (rc) return rc;
	h->n_cond = 0;
	if (n_cond == 0) return SGX_OK;

	// S_C and Phi_CC: sgx_skat_2bit on the set as one unit
	const int64_t unit_ptr[2] = {0, (int64_t)n_cond};
	int32_t var_idx[SGX_COND_MAX];
	for (size_t c = 0; c < n_cond; c++) var_idx[c] = (int32_t)c;
	std::vector<double> dense;
	rc = skat_2bit_host(h, packed_c, bpv, n_cond, 1, unit_ptr, var_idx, lut_c, score_c, cov_cc, dense);
	if (rc) return rc;

	const int C = (int)n_cond;
	return cond_install(h, C, dense, [&](int PB, dim3 grid) -> int {
		const size_t dbpv = (size_t)((N + 15) >> 4) * 4;
		TabLayout tl;
		tl.add<uint8_t>((size_t)C * dbpv);
		const auto s_lut = tl.add((size_t)C * 4, lut_c);
		int rc = grow(h->stage_pk, tl.bytes());
		if (!rc) rc = copy_rows_h2d(h->stage_pk, dbpv, packed_c, bpv, (size_t)C, h->stream);
		if (!rc) rc = tabs_upload(h->stage_pk, h->stream, s_lut);
		if (rc) return rc;
		hipLaunchKernelGGL(cond_build_kernel, grid, dim3(256), 0, h->stream,
			h->stage_pk, dbpv, tl.at(h->stage_pk, s_lut), C, h->md.F, h->md.P, N, PB, h->cond_B);
		return SGX_OK;
	});
}

// M rows -> score / var / cov in device memory, queued on lane->stream: the rows in launches whose per-slab sums fit
// COND_PART_BYTES (what a row gets does not depend on the cut), each followed by the slab sum and the finish.
// rect(nct, grid, off, m) queues the rectangular kernel of rows [off, off + m) with nct column tiles
// (std::integral_constant) into lane->cond_part; slab_ch: the chunks of 256 samples of its sample slabs.  p: the primary
// handle, which holds the set.
template <class Rect>
static int cond_run(sgx_handle *p, sgx_handle *lane, size_t M, int slab_ch, Rect rect, double *score, double *var, double *cov)
{
	const int N = p->md.N, C = p->n_cond, NCT = (cond_ncol(p) + 15) / 16, WD = 16 * NCT + 1;
	const int nslab = ((N + 255) / 256 + slab_ch - 1) / slab_ch;
	size_t mchunk = COND_PART_BYTES / ((size_t)nslab * WD * sizeof(double));
	mchunk = std::min(M, std::max<size_t>(COND_WG_ROWS, mchunk / COND_WG_ROWS * COND_WG_ROWS));
	int rc = ensure_buf(lane, lane->cond_part, mchunk * nslab * WD);
	if (rc) return rc;
	rc = ensure_buf(lane, lane->cond_fin, mchunk * WD);
	if (rc) return rc;
	hipStream_t st = lane->stream;
	using std::integral_constant;
	for (size_t off = 0; off < M; off += mchunk) {
		const size_t m = std::min(mchunk, M - off);
		const dim3 grid((unsigned)((m + COND_WG_ROWS - 1) / COND_WG_ROWS), (unsigned)nslab);
		switch (NCT) {
		case 1: rect(integral_constant<int, 1>{}, grid, off, m); break;
		case 2: rect(integral_constant<int, 2>{}, grid, off, m); break;
		case 3: rect(integral_constant<int, 3>{}, grid, off, m); break;
		default: rect(integral_constant<int, 4>{}, grid, off, m); break;
		}
		HIPCHK(hipGetLastError());
		const size_t nel = m * WD;
		hipLaunchKernelGGL(skat_reduce_kernel, dim3((unsigned)((nel + 255) / 256)), dim3(256), 0, st,
			lane->cond_part, nel, nslab, lane->cond_fin);
		HIPCHK(hipGetLastError());
		hipLaunchKernelGGL(cond_finish_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st,
			lane->cond_fin, m, WD, p->md, C, p->cond_ce, score + off, var + off, cov + off * C);
		HIPCHK(hipGetLastError());
	}
	return SGX_OK;
}

// 2-bit rows in device memory through cond_run.
static int cond_rows_dev(sgx_handle *p, sgx_handle *lane, const uint8_t *rows, size_t bpv, size_t M,
	const double *lut, double *score, double *var, double *cov)
{
	return cond_run(p, lane, M, COND_SLAB_CH, [&](auto nct, dim3 grid, size_t off, size_t m) {
		hipLaunchKernelGGL(cond_rect_kernel<decltype(nct)::value>, grid, dim3(256), 0, lane->stream, rows + off * bpv, bpv,
			p->md.N, m, lut + 4 * off, p->md.F, p->md.P, p->cond_B, COND_SLAB_CH, lane->cond_part);
	}, score, var, cov);
}

extern "C" int sgx_cond_2bit_dev(sgx_handle *h, const uint8_t *packed_dev, size_t bpv, size_t M,
	const double *lut_dev, double *score_dev, double *var_dev, double *cov_dev)
{
	if (!h) return fail(SGX_EINVAL, "sgx_cond_2bit_dev: NULL handle");
	if (h->owner) return fail(SGX_EINVAL, "sgx_cond_2bit_dev: not on a twin");
	if (M == 0) return SGX_OK;
	if (!packed_dev || !lut_dev || !score_dev || !var_dev || !cov_dev)
		return fail(SGX_EINVAL, "sgx_cond_2bit_dev: NULL buffer");
	if (h->n_cond == 0) return fail(SGX_EINVAL, "sgx_cond_2bit_dev: no conditioning set (sgx_cond_set)");
	int rc = dev_rows_check("sgx_cond_2bit_dev", packed_dev, bpv, h->md.N);
	if (!rc) rc = set_dev(h);
	if (rc) return rc;
	sgx_handle *lane = h->last_issued ? h->last_issued : h;      // behind the most recent call: a scan of the same rows
	return cond_rows_dev(h, lane, packed_dev, bpv, M, lut_dev, score_dev, var_dev, cov_dev);
}

extern "C" int sgx_cond_2bit(sgx_handle *h, const uint8_t *packed, size_t bpv, size_t M,
	const double *lut, double *score, double *var, double *cov)
{
	if (!h) return fail(SGX_EINVAL, "sgx_cond_2bit: NULL handle");
	if (h->owner) return fail(SGX_EINVAL, "sgx_cond_2bit: not on a twin");
	if (M == 0) return SGX_OK;
	if (!packed || !lut || !score || !var || !cov) return fail(SGX_EINVAL, "sgx_cond_2bit: NULL buffer");
	if (h->n_cond == 0) return fail(SGX_EINVAL, "sgx_cond_2bit: no conditioning set (sgx_cond_set)");
	int rc = bpv_check(bpv, h->md.N);
	if (!rc) rc = begin_call(h);
	if (rc) return rc;
	return rows_2bit_host(h, packed, bpv, M, lut, {{score, 1}, {var, 1}, {cov, (size_t)h->n_cond}},
		[&](const uint8_t *rows, size_t dbpv, size_t m, const double *d_lut, double *const *d_out) {
			return cond_rows_dev(h, h, rows, dbpv, m, d_lut, d_out[0], d_out[1], d_out[2]);
		});
}
