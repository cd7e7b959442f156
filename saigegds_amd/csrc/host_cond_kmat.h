// host_cond_kmat.h -- the conditional scan on an explicit GRM: S_j, Phi^K_jj and Phi^K_jC of every scanned
// row under the fitted model itself, Phi^K = 1/2 (C + C') - D E^-1 D' as sgx_skat_kmat_2bit defines it on the unit
// (c_1 .. c_C, j), with the set's solves made once.  sgx_cond_kmat_set installs the set (its columns, solves and
// products by the functions of host_skat_kmat.h), sgx_cond_kmat_2bit takes rows in host memory: per chunk of at most
// SGX_GRM_MAX_RHS rows the columns, one solve, and ckm_panel_kernel (kern_cond_kmat.h).  Both are a flow with the
// column source (SkkSrc) as its only variable: ckm_install and ckm_scan / ckm_chunk, which the entries on a resident
// dosage block (host_kmat_ds.h) share.
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.

// device room for the column sums of a chunk of at most SGX_GRM_MAX_RHS of m rows
static int ckm_sum_room(const char *who, sgx_handle *h, size_t m)
{
	const int N = h->md.N, C1 = h->md.K + 1;
	const int ndw = (N + 15) >> 4, ncslab = (ndw + SKK_CSLAB_DW - 1) / SKK_CSLAB_DW;
	const size_t mc = std::min<size_t>(m, SGX_GRM_MAX_RHS);
	int rc = dev_room(h->skk_cpart, mc * ncslab * C1, "the column sums", who);
	if (!rc) rc = dev_room(h->skk_cs, mc * C1, "the column sums", who);
	return rc;
}

// ... and for m 2-bit rows themselves (the first slot of h->stage_pk) with a chunk's index list and the tables behind them
static int ckm_room(const char *who, sgx_handle *h, size_t m, size_t dbpv, TabSlot<int> &s_idx, TabSlot<double> &s_lut)
{
	TabLayout tl;
	tl.add<uint8_t>(m * dbpv);
	s_idx = tl.add<int>(std::min<size_t>(m, SGX_GRM_MAX_RHS));
	s_lut = tl.add<double>(m * 4);
	int rc = dev_room(h->stage_pk, tl.bytes(), "the rows", who);
	if (!rc) rc = ckm_sum_room(who, h, m);
	return rc;
}

// the checks of a set's arguments that do not depend on where its rows are; *clear: n_cond == 0, the set was cleared
static int ckm_set_args(const char *who, sgx_handle *h, sgx_kmat *km, size_t n_cond, bool *clear)
{
	*clear = false;
	if (!h) return fail(SGX_EINVAL, "%s: NULL handle", who);
	if (h->owner) return fail(SGX_EINVAL, "%s: not on a twin", who);
	if (n_cond > SGX_COND_MAX)
		return fail(SGX_EINVAL, "%s: %zu conditioning variants, at most %d are supported", who, n_cond, SGX_COND_MAX);
	if (n_cond == 0) {
		const int rc = sgx_sync(h);
		if (rc) return rc;
		h->ckm_n = 0;
		h->ckm_km = nullptr;
		*clear = true;
		return SGX_OK;
	}
	if (!km) return fail(SGX_EINVAL, "%s: NULL handle", who);
	return SGX_OK;
}

// Installs the set of C entries of `src` (on the device, queued on the handle's stream; the old set is gone): its
// vectors [A_C | Y_C | Z | X], the solves, E = X'Z and its inverse, C = A_C'Y_C, D_C = A_C'Z and Phi^K_CC.
// h->ckm_bad [C] is filled by the caller: entries whose column is zeros and whose results are non-finite.
static int ckm_install(const char *who, sgx_handle *h, sgx_kmat *km, const SkkSrc &src, int C, const double *w, const double *tau,
	int maxiter, double tol, std::chrono::steady_clock::time_point t_col, double *score_c, double *cov_cc, int32_t *iters_c)
{
	const int N = h->md.N, K = h->md.K;
	const size_t lda = (size_t)((N + 15) >> 4) * 16;
	hipStream_t st = h->stream;
	int rc = dev_room(h->ckm_set, (size_t)(2 * C + 2 * K) * lda, "the set's vectors", who);
	if (rc) return rc;
	double *A_C = h->ckm_set, *Y_C = A_C + (size_t)C * lda, *Z = Y_C + (size_t)C * lda, *Xc = Z + (size_t)K * lda;
	hipLaunchKernelGGL(skk_xcols_kernel, dim3((unsigned)((lda + 255) / 256), (unsigned)K), dim3(256), 0, st, h->md.X, N, K, Xc, lda);
	HIPCHK(hipMemsetAsync(Y_C, 0, (size_t)(C + K) * lda * sizeof(double), st));      // Y_C and Z: the solves fill N of lda
	HIPCHK(hipGetLastError());
	rc = skk_columns(h, src, C, A_C, lda, score_c);
	if (rc) return rc;
	h->skk_ms[0] += skk_ms_since(t_col);

	// the weights on the operator's device copy; Z = Sigma^-1 X, Y_C = Sigma^-1 A_C
	auto t_sol = std::chrono::steady_clock::now();
	HIPCHK(hipMemcpyAsync(km->pw.w, w, (size_t)N * sizeof(double), hipMemcpyHostToDevice, km->stream));
	std::vector<int> it_z((size_t)K), it_c((size_t)C);
	rc = kmat_pcg_dev(who, km, km->pw.w, tau, Xc, lda, K, maxiter, tol, Z, it_z.data());
	if (!rc) rc = kmat_pcg_dev(who, km, km->pw.w, tau, A_C, lda, C, maxiter, tol, Y_C, it_c.data());
	if (rc) return rc;
	if (iters_c) for (int c = 0; c < C; c++) iters_c[c] = it_c[c];
	h->skk_ms[1] += skk_ms_since(t_sol);

	// E = X'Z and its inverse, C = A_C'Y_C, D_C = A_C'Z, Phi^K_CC
	auto t_con = std::chrono::steady_clock::now();
	std::vector<double> E((size_t)K * K), Cm((size_t)C * C);
	h->ckm_D.assign((size_t)C * K, 0.0);
	h->ckm_q.assign((size_t)C * K, 0.0);
	rc = skk_product(h, Xc, 0, K, Z, 0, K, lda, E.data(), (size_t)K);
	if (!rc) rc = skk_product(h, A_C, 0, C, Y_C, 0, C, lda, Cm.data(), (size_t)C);
	if (!rc) rc = skk_product(h, A_C, 0, C, Z, 0, K, lda, h->ckm_D.data(), (size_t)K);
	if (rc) return rc;
	h->ckm_eok = skk_inverse(K, E, h->ckm_Einv);
	const double *D = h->ckm_D.data(), *q = h->ckm_q.data();
	for (int c = 0; c < C; c++) skk_q(K, h->ckm_Einv, h->ckm_eok, D + (size_t)c * K, h->ckm_q.data() + (size_t)c * K);
	for (int j = 0; j < C; j++)
		for (int l = j; l < C; l++) {
			double v = skk_phi_entry(K, Cm[(size_t)j * C + l], Cm[(size_t)l * C + j], D + (size_t)j * K, D + (size_t)l * K,
				q + (size_t)j * K, q + (size_t)l * K);
			if (h->ckm_bad[j] || h->ckm_bad[l]) v = NAN;
			cov_cc[(size_t)j * C + l] = v;
			cov_cc[(size_t)l * C + j] = v;
		}
	for (int c = 0; c < C; c++) if (h->ckm_bad[c]) score_c[c] = NAN;
	h->skk_ms[2] += skk_ms_since(t_con);

	h->ckm_w.assign(w, w + N);
	h->ckm_tau[0] = tau[0]; h->ckm_tau[1] = tau[1];
	h->ckm_maxiter = maxiter; h->ckm_tol = tol;
	h->ckm_km = km;
	h->ckm_n = C;
	return SGX_OK;
}

extern "C" int sgx_cond_kmat_set(sgx_handle *h, sgx_kmat *km, const uint8_t *packed_c, size_t bpv, size_t n_cond,
	const double *lut_c, const double *w, const double *tau, int maxiter, double tol, double *score_c, double *cov_cc,
	int32_t *iters_c)
{
	const char *who = "sgx_cond_kmat_set";
	bool clear;
	int rc = ckm_set_args(who, h, km, n_cond, &clear);
	if (rc || clear) return rc;
	if (!packed_c || !lut_c || !w || !tau || !score_c || !cov_cc) return fail(SGX_EINVAL, "%s: NULL buffer", who);
	const int N = h->md.N, C = (int)n_cond;
	rc = skk_km_check(who, h, km);
	if (rc) return rc;
	rc = bpv_check(bpv, N);
	if (!rc) rc = skk_sigma_args(who, N, w, tau, maxiter);
	if (!rc) rc = sgx_sync(h);                   // nothing queued reads the set that is replaced
	if (!rc) rc = set_dev(h);
	if (rc) return rc;
	h->last_issued = h;
	hipStream_t st = h->stream;
	auto t_col = std::chrono::steady_clock::now();
	h->skk_ms[0] = h->skk_ms[1] = h->skk_ms[2] = 0;

	const size_t dbpv = (size_t)((N + 15) >> 4) * 4;
	TabSlot<int> s_idx; TabSlot<double> s_lut;
	rc = ckm_room(who, h, (size_t)C, dbpv, s_idx, s_lut);
	if (rc) return rc;
	h->ckm_n = 0;                               // from here on the old set is gone
	h->ckm_km = nullptr;
	std::vector<double> lut_ok;
	skk_tables(lut_c, (size_t)C, lut_ok, h->ckm_bad);
	int32_t iota[SGX_COND_MAX];
	for (int c = 0; c < C; c++) iota[c] = c;
	rc = copy_rows_h2d(h->stage_pk, dbpv, packed_c, bpv, (size_t)C, st);
	if (!rc) rc = tab_copy(h->stage_pk, s_idx, iota, (size_t)C, st);
	if (!rc) rc = tab_copy(h->stage_pk, s_lut, lut_ok.data(), (size_t)C * 4, st);
	if (rc) return rc;
	SkkSrc src;
	src.idx = TabLayout::at(h->stage_pk, s_idx);
	src.rows = h->stage_pk; src.dbpv = dbpv;
	src.lut = TabLayout::at(h->stage_pk, s_lut);
	return ckm_install(who, h, km, src, C, w, tau, maxiter, tol, t_col, score_c, cov_cc, iters_c);
}

// the checks of a scan's arguments that do not depend on where its rows are
static int ckm_scan_args(const char *who, sgx_handle *h, sgx_kmat *km)
{
	if (!h || !km) return fail(SGX_EINVAL, "%s: NULL handle", who);
	if (h->owner) return fail(SGX_EINVAL, "%s: not on a twin", who);
	if (h->ckm_n == 0) return fail(SGX_EINVAL, "%s: no conditioning set (sgx_cond_kmat_set)", who);
	if (km != h->ckm_km) return fail(SGX_EINVAL, "%s: not the matrix the set was installed with", who);
	return SGX_OK;
}

// A scan against the installed set, in chunks of at most SGX_GRM_MAX_RHS rows
struct CkmScan {
	int C = 0, K = 0, NPT = 0, NT = 0, nslab = 0;
	size_t lda = 0;
	std::vector<double> fin, dj, qj;
	std::vector<int> it;
};

// device room and host scratch of a scan whose chunks hold at most mc_max rows; the set's weights go to the operator
static int ckm_scan_begin(const char *who, sgx_handle *h, sgx_kmat *km, size_t mc_max, CkmScan &cs)
{
	const int N = h->md.N;
	cs.C = h->ckm_n; cs.K = h->md.K;
	cs.lda = (size_t)((N + 15) >> 4) * 16;
	cs.nslab = ((int)cs.lda + SKK_SLAB - 1) / SKK_SLAB;
	cs.NPT = (cs.C + cs.K + 15) / 16; cs.NT = cs.NPT + 2;
	const size_t nrt_max = (mc_max + 15) / 16;
	int rc = dev_room(h->skk_A, mc_max * cs.lda, "a chunk's columns", who);
	if (!rc) rc = dev_room(h->skk_Y, mc_max * cs.lda, "a chunk's solves", who);
	if (!rc) rc = dev_room(h->skat_part, (size_t)cs.nslab * nrt_max * cs.NT * 256, "the slab partials", who);
	if (!rc) rc = dev_room(h->skat_fin, nrt_max * cs.NT * 256, "the tiles", who);
	if (rc) return rc;
	cs.fin.resize(nrt_max * cs.NT * 256);
	cs.dj.resize((size_t)cs.K); cs.qj.resize((size_t)cs.K);
	cs.it.assign((size_t)SGX_GRM_MAX_RHS, 0);
	HIPCHK(hipMemcpyAsync(km->pw.w, h->ckm_w.data(), (size_t)N * sizeof(double), hipMemcpyHostToDevice, km->stream));
	HIPCHK(hipMemsetAsync(h->skk_Y, 0, mc_max * cs.lda * sizeof(double), h->stream));      // the solves fill N of lda
	return SGX_OK;
}

// one chunk: the first m <= SGX_GRM_MAX_RHS entries of `src` with their flags bad [m] -> results [m]
static int ckm_chunk(const char *who, sgx_handle *h, sgx_kmat *km, const SkkSrc &src, int m, const uint8_t *bad, CkmScan &cs,
	double *score, double *var, double *cov, int32_t *iters)
{
	const int N = h->md.N, K = cs.K, C = cs.C, NPT = cs.NPT, NT = cs.NT, nslab = cs.nslab;
	const size_t lda = cs.lda;
	hipStream_t st = h->stream;
	const double *D_C = h->ckm_D.data(), *q_C = h->ckm_q.data();
	auto t_col = std::chrono::steady_clock::now();
	int rc = skk_columns(h, src, m, h->skk_A, lda, score);
	if (rc) return rc;
	h->skk_ms[0] += skk_ms_since(t_col);

	auto t_sol = std::chrono::steady_clock::now();
	rc = kmat_pcg_dev(who, km, km->pw.w, h->ckm_tau, h->skk_A, lda, m, h->ckm_maxiter, h->ckm_tol, h->skk_Y, cs.it.data());
	if (rc) return rc;
	h->skk_ms[1] += skk_ms_since(t_sol);

	auto t_con = std::chrono::steady_clock::now();
	const int nrt = (m + 15) / 16;
	const dim3 grid((unsigned)((nrt + CKM_WG_TILES - 1) / CKM_WG_TILES), (unsigned)nslab);
	if (NPT == 1)
		hipLaunchKernelGGL(ckm_panel_kernel<1>, grid, dim3(256), 0, st, h->ckm_set, C, K, h->skk_A, h->skk_Y, lda, N, m, h->skat_part);
	else
		hipLaunchKernelGGL(ckm_panel_kernel<2>, grid, dim3(256), 0, st, h->ckm_set, C, K, h->skk_A, h->skk_Y, lda, N, m, h->skat_part);
	const size_t nel = (size_t)nrt * NT * 256;
	hipLaunchKernelGGL(skat_reduce_kernel, dim3((unsigned)((nel + 255) / 256)), dim3(256), 0, st, h->skat_part, nel, nslab, h->skat_fin);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(cs.fin.data(), h->skat_fin, nel * sizeof(double), hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	// the host's last step: row j is the last entry of the unit (c_1 .. c_C, j)
	double *dj = cs.dj.data(), *qj = cs.qj.data();
	for (int j = 0; j < m; j++) {
		const double *tl = &cs.fin[(size_t)(j >> 4) * NT * 256];
		const int jl = j & 15;
		auto panel = [&](int p) { return tl[(size_t)(p >> 4) * 256 + jl * 16 + (p & 15)]; };      // a_j' (panel vector p)
		for (int a = 0; a < K; a++) dj[a] = panel(C + a);
		skk_q(K, h->ckm_Einv, h->ckm_eok, dj, qj);
		const double cjj = tl[(size_t)(NPT + 1) * 256 + jl * 16 + jl];
		const bool bj = bad[j] != 0;
		var[j] = bj ? NAN : skk_phi_entry(K, cjj, cjj, dj, dj, qj, qj);
		for (int c = 0; c < C; c++) {
			const double c_cj = tl[(size_t)NPT * 256 + c * 16 + jl], c_jc = panel(c);
			const double v = skk_phi_entry(K, c_cj, c_jc, D_C + (size_t)c * K, dj, q_C + (size_t)c * K, qj);
			cov[j * (size_t)C + c] = (bj || h->ckm_bad[c]) ? NAN : v;
		}
		if (bj) score[j] = NAN;
		if (iters) iters[j] = cs.it[j];
	}
	h->skk_ms[2] += skk_ms_since(t_con);
	return SGX_OK;
}

extern "C" int sgx_cond_kmat_2bit(sgx_handle *h, sgx_kmat *km, const uint8_t *packed, size_t bpv, size_t M,
	const double *lut, double *score, double *var, double *cov, int32_t *iters)
{
	const char *who = "sgx_cond_kmat_2bit";
	int rc = ckm_scan_args(who, h, km);
	if (rc) return rc;
	if (M == 0) return SGX_OK;
	if (!packed || !lut || !score || !var || !cov) return fail(SGX_EINVAL, "%s: NULL buffer", who);
	const int N = h->md.N, C = h->ckm_n;
	rc = skk_km_check(who, h, km);
	if (rc) return rc;
	rc = bpv_check(bpv, N);
	if (!rc) rc = begin_call(h);
	if (rc) return rc;
	hipStream_t st = h->stream;
	h->skk_ms[0] = h->skk_ms[1] = h->skk_ms[2] = 0;
	auto t_col = std::chrono::steady_clock::now();

	const size_t dbpv = (size_t)((N + 15) >> 4) * 4;
	const size_t rchunk = scan_chunk(h, dbpv, M);
	const size_t mc_max = std::min<size_t>(rchunk, SGX_GRM_MAX_RHS);
	TabSlot<int> s_idx; TabSlot<double> s_lut;
	CkmScan cs;
	rc = ckm_room(who, h, rchunk, dbpv, s_idx, s_lut);
	if (rc) return rc;
	std::vector<double> lut_ok;
	std::vector<uint8_t> bad;
	skk_tables(lut, M, lut_ok, bad);
	int32_t iota[SGX_GRM_MAX_RHS];
	for (int j = 0; j < SGX_GRM_MAX_RHS; j++) iota[j] = j;
	rc = ckm_scan_begin(who, h, km, mc_max, cs);
	if (!rc) rc = tab_copy(h->stage_pk, s_idx, iota, mc_max, st);
	if (rc) return rc;
	h->skk_ms[0] += skk_ms_since(t_col);

	SkkSrc src;
	src.idx = TabLayout::at(h->stage_pk, s_idx);
	src.dbpv = dbpv;
	for (size_t off = 0; off < M; off += rchunk) {
		t_col = std::chrono::steady_clock::now();
		const size_t mr = std::min(rchunk, M - off);
		rc = copy_rows_h2d(h->stage_pk, dbpv, packed + off * bpv, bpv, mr, st);
		if (!rc) rc = tab_copy(h->stage_pk, s_lut, lut_ok.data() + 4 * off, 4 * mr, st);
		if (rc) return rc;
		h->skk_ms[0] += skk_ms_since(t_col);
		for (size_t j0 = 0; j0 < mr; j0 += SGX_GRM_MAX_RHS) {
			const int m = (int)std::min<size_t>(SGX_GRM_MAX_RHS, mr - j0);
			const size_t g0 = off + j0;
			src.rows = h->stage_pk + j0 * dbpv;
			src.lut = TabLayout::at(h->stage_pk, s_lut) + 4 * j0;
			rc = ckm_chunk(who, h, km, src, m, &bad[g0], cs, score + g0, var + g0, cov + g0 * (size_t)C, iters ? iters + g0 : nullptr);
			if (rc) return rc;
		}
	}
	return SGX_OK;
}
