// host_skat_kmat.h -- SKAT on an explicit GRM: per unit the score statistics of sgx_skat_2bit and their
// covariance under the fitted model, Phi^K = 1/2 (C + C') - D E^-1 D' with C = A' Y, D = A' Z, E = X' Z, Y = Sigma^-1 A,
// Z = Sigma^-1 X.  kern_skat_kmat.h makes A, X and the products; the solves are pcg_core (host_pcg.h) on the resident
// vectors, through the operator's product, in chunks of at most SGX_GRM_MAX_RHS columns.
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.

// the explicit-matrix solve on resident vectors: B_dev, X_dev at [k][ldb], w_dev [n]; synchronous
static int kmat_pcg_dev(const char *fn, sgx_kmat *m, const double *w_dev, const double *tau, const double *B_dev, size_t ldb,
	int k, int maxiter, double tol, double *X_dev, int *iters)
{
	HIPCHK(hipSetDevice(m->device));
	const hipError_t e = pcg_reserve(&m->pw, k);
	if (e != hipSuccess) {
		(void)hipGetLastError();
		return fail(mem_code(e), "%s: the workspace of %d columns: %s", fn, k, hipGetErrorString(e));
	}
	int rc = pcg_core(&m->pw, m->diag, w_dev, tau, B_dev, ldb, k, maxiter, tol, iters, kmat_product(m), nullptr);
	if (rc) return rc;
	const size_t nb = (size_t)m->n * sizeof(double);
	HIPCHK(hipMemcpy2DAsync(X_dev, ldb * sizeof(double), m->pw.X, nb, nb, (size_t)k, hipMemcpyDeviceToDevice, m->stream));
	HIPCHK(hipStreamSynchronize(m->stream));
	return SGX_OK;
}

extern "C" int sgx_kmat_pcg_multi_dev(sgx_kmat *m, const double *w_dev, const double *tau, const double *B_dev, size_t ldb,
	int k, int maxiter, double tol, double *X_dev, int *iters)
{
	if (!w_dev || !tau || !iters) return fail(SGX_EINVAL, "sgx_kmat_pcg_multi_dev: NULL argument");
	int rc = pcg_multi_args("sgx_kmat_pcg_multi_dev", m, m ? m->n : 0, B_dev, ldb, k, X_dev);
	if (rc) return rc;
	return kmat_pcg_dev("sgx_kmat_pcg_multi_dev", m, w_dev, tau, B_dev, ldb, k, maxiter, tol, X_dev, iters);
}

// out[r][c] = (vector row0 + r of L)' (vector col0 + c of R) for r < nr, c < nc (row-major, ldo apart): the tiles,
// as many per launch as SKAT_PART_BYTES holds slab partials of, then the slabs added in slab order
static int skk_product(sgx_handle *h, const double *L, int row0, int nr, const double *R, int col0, int nc, size_t ld,
	double *out, size_t ldo)
{
	const int N = h->md.N;
	const int nslab = (((N + 15) & ~15) + SKK_SLAB - 1) / SKK_SLAB;
	std::vector<SkkTile> tiles;
	for (int r = 0; r < nr; r += 16)
		for (int c = 0; c < nc; c += 16) tiles.push_back(SkkTile{row0 + r, col0 + c, std::min(16, nr - r), std::min(16, nc - c)});
	const size_t T = tiles.size();
	if (T == 0) return SGX_OK;
	const size_t tchunk = std::min(T, std::max<size_t>(1, SKAT_PART_BYTES / ((size_t)nslab * 256 * sizeof(double))));
	const char *who = "sgx_skat_kmat_2bit";      // whichever entry the product is for: the text has named this one so far
	int rc = dev_room(h->skat_part, tchunk * (size_t)nslab * 256, "the slab partials", who);
	if (!rc) rc = dev_room(h->skat_fin, tchunk * 256, "the tiles", who);
	if (!rc) rc = dev_room(h->skk_tiles, tchunk, "the tile list", who);
	if (rc) return rc;
	std::vector<double> fin(tchunk * 256);
	for (size_t t0 = 0; t0 < T; t0 += tchunk) {
		const size_t nt = std::min(tchunk, T - t0);
		HIPCHK(hipMemcpyAsync(h->skk_tiles, &tiles[t0], nt * sizeof(SkkTile), hipMemcpyHostToDevice, h->stream));
		hipLaunchKernelGGL(skk_gram_kernel, dim3((unsigned)nt, (unsigned)nslab), dim3(64), 0, h->stream, L, ld, R, ld, N,
			h->skk_tiles, nt, h->skat_part);
		hipLaunchKernelGGL(skat_reduce_kernel, dim3((unsigned)nt), dim3(256), 0, h->stream, h->skat_part, nt * 256, nslab, h->skat_fin);
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpyAsync(fin.data(), h->skat_fin, nt * 256 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
		HIPCHK(hipStreamSynchronize(h->stream));     // (also: the tile list is free for the next chunk)
		for (size_t k = 0; k < nt; k++) {
			const SkkTile &t = tiles[t0 + k];
			for (int i = 0; i < t.nrow; i++)
				for (int j = 0; j < t.ncol; j++)
					out[(size_t)(t.row0 - row0 + i) * ldo + (t.col0 - col0 + j)] = fin[k * 256 + i * 16 + j];
		}
	}
	return SGX_OK;
}

// inv = the inverse of the symmetric part of E [K][K] by Gauss-Jordan with partial pivoting, symmetrised; false: singular
static bool skk_inverse(int K, const std::vector<double> &E, std::vector<double> &inv)
{
	std::vector<double> a((size_t)K * 2 * K, 0.0);
	for (int i = 0; i < K; i++) {
		for (int j = 0; j < K; j++) a[(size_t)i * 2 * K + j] = 0.5 * (E[(size_t)i * K + j] + E[(size_t)j * K + i]);
		a[(size_t)i * 2 * K + K + i] = 1;
	}
	for (int c = 0; c < K; c++) {
		int p = c;
		for (int i = c + 1; i < K; i++) if (std::fabs(a[(size_t)i * 2 * K + c]) > std::fabs(a[(size_t)p * 2 * K + c])) p = i;
		const double piv = a[(size_t)p * 2 * K + c];
		if (!(std::fabs(piv) > 0) || !std::isfinite(piv)) return false;
		if (p != c) for (int j = 0; j < 2 * K; j++) std::swap(a[(size_t)p * 2 * K + j], a[(size_t)c * 2 * K + j]);
		for (int j = 0; j < 2 * K; j++) a[(size_t)c * 2 * K + j] /= piv;
		for (int i = 0; i < K; i++) {
			if (i == c) continue;
			const double f = a[(size_t)i * 2 * K + c];
			if (f != 0) for (int j = 0; j < 2 * K; j++) a[(size_t)i * 2 * K + j] -= f * a[(size_t)c * 2 * K + j];
		}
	}
	inv.assign((size_t)K * K, 0.0);
	for (int i = 0; i < K; i++)
		for (int j = 0; j < K; j++) inv[(size_t)i * K + j] = 0.5 * (a[(size_t)i * 2 * K + K + j] + a[(size_t)j * 2 * K + K + i]);
	return true;
}

// The host's last step, Phi^K = 1/2 (C + C') - D E^-1 D', entry by entry (shared with host_cond_kmat.h).
// q = E^-1 d for one row d [K] of D (NaN where E was singular)
static void skk_q(int K, const std::vector<double> &Einv, bool e_ok, const double *d, double *q)
{
	for (int a = 0; a < K; a++) {
		double x = 0;
		for (int b = 0; b < K; b++) x += (e_ok ? Einv[(size_t)a * K + b] : NAN) * d[b];
		q[a] = x;
	}
}

// entry (j, l): c_jl, c_lj of C, rows d_j, d_l of D and their q
static double skk_phi_entry(int K, double c_jl, double c_lj, const double *dj, const double *dl, const double *qj, const double *ql)
{
	double djl = 0, dlj = 0;      // both orders, so that the entry does not depend on which of the two comes first
	for (int a = 0; a < K; a++) {
		djl += dj[a] * ql[a];
		dlj += dl[a] * qj[a];
	}
	return 0.5 * (c_jl + c_lj) - 0.5 * (djl + dlj);
}

// the rules for w [N], tau [2] and maxiter of the entries that solve with Sigma = tau[0] diag(1/w) + tau[1] K
static int skk_sigma_args(const char *who, int N, const double *w, const double *tau, int maxiter)
{
	if (!(tau[0] > 0) || !(tau[1] >= 0) || !std::isfinite(tau[0]) || !std::isfinite(tau[1]))
		return fail(SGX_EINVAL, "%s: tau = (%g, %g), need tau[0] > 0 and tau[1] >= 0", who, tau[0], tau[1]);
	for (int i = 0; i < N; i++)
		if (!(w[i] > 0) || !std::isfinite(w[i])) return fail(SGX_EINVAL, "%s: w[%d] = %g is not a positive finite weight", who, i, w[i]);
	if (maxiter < 0) return fail(SGX_EINVAL, "%s: maxiter = %d", who, maxiter);
	return SGX_OK;
}

static double skk_ms_since(const std::chrono::steady_clock::time_point &t0)
{
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// Where the columns of a call's entries come from -- the only thing in which the 2-bit entries and the entries on a
// resident dosage block (host_kmat_ds.h) differ.  Entry e of the source is row idx[e] of its rows, with its table
// lut[e][4] (2-bit rows on the device, dbpv bytes apart) or its flip[e] / mean[e] (dosage rows, N elements apart:
// kern_kmat_ds.h; flip[e] & SKK_DS_ZERO: a column of zeros).  All pointers are device pointers.
struct SkkSrc {
	const int *idx = nullptr;
	const uint8_t *rows = nullptr; size_t dbpv = 0; const double *lut = nullptr;             // 2-bit rows
	const void *ds = nullptr; int ds_dtype = 0; const uint8_t *flip = nullptr; const double *mean = nullptr;   // dosage rows
	// the source of the entries from e on
	SkkSrc from(size_t e) const
	{
		SkkSrc s = *this;
		s.idx += e;
		if (ds) { s.flip += e; s.mean += e; } else s.lut += 4 * e;
		return s;
	}
};

template <typename T, int NS>
static void skk_launch_colsum_ds(sgx_handle *h, const SkkSrc &src, int ncslab, int m)
{
	hipLaunchKernelGGL((skk_colsum_ds_kernel<T, NS>), dim3((unsigned)ncslab, (unsigned)m), dim3(256), 0, h->stream,
		(const T *)src.ds, h->md.N, src.idx, src.flip, src.mean, h->md.F, h->md.P, h->md.K, h->skk_cpart);
}

// the accumulators a thread of skk_colsum_ds_kernel holds: the smallest of 4, 9, 17 that takes the K + 1 sums
template <typename T>
static void skk_colsum_ds(sgx_handle *h, const SkkSrc &src, int ncslab, int m)
{
	const int C1 = h->md.K + 1;
	if (C1 <= 4) skk_launch_colsum_ds<T, 4>(h, src, ncslab, m);
	else if (C1 <= 9) skk_launch_colsum_ds<T, 9>(h, src, ncslab, m);
	else skk_launch_colsum_ds<T, 17>(h, src, ncslab, m);
}
static_assert(KMAX + 1 <= 17, "skk_colsum_ds: K + 1 sums");

// the first m entries of `src` -> their adj columns A [m][lda] and score statistics: the column sums per slab
// (skk_cpart), the slabs added (skk_cs), the columns, and S = s - S_a . c' on the host.  Synchronous.
static int skk_columns(sgx_handle *h, const SkkSrc &src, int m, double *A, size_t lda, double *score)
{
	const int N = h->md.N, K = h->md.K, P = h->md.P, C1 = K + 1;
	const int ndw = (N + 15) >> 4, ncslab = (ndw + SKK_CSLAB_DW - 1) / SKK_CSLAB_DW;
	const unsigned gl = (unsigned)((lda + 255) / 256);
	hipStream_t st = h->stream;
	if (!src.ds)
		hipLaunchKernelGGL(skk_colsum_kernel, dim3((unsigned)ncslab, (unsigned)m), dim3(256), 0, st, src.rows, src.dbpv, N,
			src.idx, src.lut, h->md.F, P, K, h->skk_cpart);
	else with_ds_rows(src.ds_dtype, src.ds, [&](auto *, auto t) { skk_colsum_ds<decltype(t)>(h, src, ncslab, m); });
	hipLaunchKernelGGL(skk_colfin_kernel, dim3((unsigned)(((size_t)m * C1 + 255) / 256)), dim3(256), 0, st, h->skk_cpart,
		(size_t)m * C1, ncslab, C1, h->skk_cs);
	if (!src.ds)
		hipLaunchKernelGGL(skk_adj_kernel, dim3(gl, (unsigned)m), dim3(256), 0, st, src.rows, src.dbpv, N, src.idx, src.lut,
			h->md.X, K, h->skk_cs, A, lda);
	else
		with_ds_rows(src.ds_dtype, src.ds, [&](auto *rows, auto t) {
			hipLaunchKernelGGL((skk_adj_ds_kernel<decltype(t)>), dim3(gl, (unsigned)m), dim3(256), 0, st, rows, N,
				src.idx, src.flip, src.mean, h->md.X, K, h->skk_cs, A, lda);
		});
	HIPCHK(hipGetLastError());
	std::vector<double> cs((size_t)m * C1);
	HIPCHK(hipMemcpyAsync(cs.data(), h->skk_cs, cs.size() * sizeof(double), hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	for (int j = 0; j < m; j++) {
		const double *cj = &cs[(size_t)j * C1];
		double sa = 0;
		for (int a = 0; a < K; a++) sa += h->md.S_a[a] * cj[a];
		const double S = cj[K] - sa;
		score[j] = h->md.quant ? S / h->md.tau0 : S;
	}
	return SGX_OK;
}

// what the arguments of the entries on an explicit GRM have in common: matrix and handle on one device, of one size
static int skk_km_check(const char *who, const sgx_handle *h, const sgx_kmat *km)
{
	if (km->device != h->device) return fail(SGX_EINVAL, "%s: the matrix is on device %d, the handle on device %d", who, km->device, h->device);
	if (km->n != h->md.N) return fail(SGX_EINVAL, "%s: the matrix has %d samples, the model has %d", who, km->n, h->md.N);
	return SGX_OK;
}

// device room of the unit loop: units of at most m_max entries
static int skk_unit_room(const char *who, sgx_handle *h, size_t m_max)
{
	const int N = h->md.N, K = h->md.K, C1 = K + 1;
	const int ndw = (N + 15) >> 4, ncslab = (ndw + SKK_CSLAB_DW - 1) / SKK_CSLAB_DW;
	const size_t lda = (size_t)ndw * 16;
	int rc = dev_room(h->skk_XZ, (size_t)2 * K * lda, "the covariate columns", who);
	if (!rc) rc = dev_room(h->skk_A, m_max * lda, "a unit's columns", who);
	if (!rc) rc = dev_room(h->skk_Y, m_max * lda, "a unit's solves", who);
	if (!rc) rc = dev_room(h->skk_cpart, m_max * ncslab * C1, "the column sums", who);
	if (!rc) rc = dev_room(h->skk_cs, m_max * C1, "the column sums", who);
	return rc;
}

// The flow of a SKAT call on an explicit GRM once its source is on the device (queued on the handle's stream): the
// covariate columns, Z = Sigma^-1 X and E = X'Z once, then per unit the columns, the solves in chunks of
// SGX_GRM_MAX_RHS, the products and the host's last step.  bad [entries]: entries whose column is zeros and whose
// results are non-finite at the end; t_col: when the call began (skk_ms[0]).
static int skk_units(const char *who, sgx_handle *h, sgx_kmat *km, const SkkSrc &src, size_t n_units, const int64_t *unit_ptr,
	const std::vector<uint8_t> &bad, size_t m_max, const double *w, const double *tau, int maxiter, double tol,
	std::chrono::steady_clock::time_point t_col, double *score, double *cov, int32_t *iters)
{
	const int N = h->md.N, K = h->md.K;
	const size_t lda = (size_t)((N + 15) >> 4) * 16;
	hipStream_t st = h->stream;
	double *Xc = h->skk_XZ, *Z = h->skk_XZ + (size_t)K * lda;
	const unsigned gl = (unsigned)((lda + 255) / 256);
	hipLaunchKernelGGL(skk_xcols_kernel, dim3(gl, (unsigned)K), dim3(256), 0, st, h->md.X, N, K, Xc, lda);
	HIPCHK(hipMemsetAsync(Z, 0, (size_t)K * lda * sizeof(double), st));
	HIPCHK(hipMemsetAsync(h->skk_Y, 0, m_max * lda * sizeof(double), st));
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(st));
	h->skk_ms[0] += skk_ms_since(t_col);

	// the weights on the operator's device copy; Z = Sigma^-1 X and E = X' Z once per call
	auto t_sol = std::chrono::steady_clock::now();
	HIPCHK(hipMemcpyAsync(km->pw.w, w, (size_t)N * sizeof(double), hipMemcpyHostToDevice, km->stream));
	std::vector<int> it_z((size_t)K), it_u;
	int rc = kmat_pcg_dev(who, km, km->pw.w, tau, Xc, lda, K, maxiter, tol, Z, it_z.data());
	if (rc) return rc;
	h->skk_ms[1] += skk_ms_since(t_sol);
	auto t_con = std::chrono::steady_clock::now();
	std::vector<double> E((size_t)K * K), Einv;
	rc = skk_product(h, Xc, 0, K, Z, 0, K, lda, E.data(), (size_t)K);
	if (rc) return rc;
	const bool e_ok = skk_inverse(K, E, Einv);
	h->skk_ms[2] += skk_ms_since(t_con);

	std::vector<double> Cm, Dm, q;
	size_t off = 0;
	for (size_t u = 0; u < n_units; u++) {
		const int64_t e0 = unit_ptr[u];
		const int m = (int)(unit_ptr[u + 1] - e0);
		if (m == 0) continue;
		double *phi = cov + off;
		off += (size_t)m * m;

		t_col = std::chrono::steady_clock::now();
		rc = skk_columns(h, src.from((size_t)e0), m, h->skk_A, lda, score + e0);
		if (rc) return rc;
		h->skk_ms[0] += skk_ms_since(t_col);

		t_sol = std::chrono::steady_clock::now();
		it_u.assign((size_t)m, 0);
		for (int j0 = 0; j0 < m; j0 += SGX_GRM_MAX_RHS) {
			const int k = std::min(SGX_GRM_MAX_RHS, m - j0);
			rc = kmat_pcg_dev(who, km, km->pw.w, tau, h->skk_A + (size_t)j0 * lda, lda, k, maxiter, tol,
				h->skk_Y + (size_t)j0 * lda, &it_u[j0]);
			if (rc) return rc;
		}
		if (iters) for (int j = 0; j < m; j++) iters[e0 + j] = it_u[j];
		h->skk_ms[1] += skk_ms_since(t_sol);

		t_con = std::chrono::steady_clock::now();
		Cm.assign((size_t)m * m, 0.0);
		Dm.assign((size_t)m * K, 0.0);
		rc = skk_product(h, h->skk_A, 0, m, h->skk_Y, 0, m, lda, Cm.data(), (size_t)m);
		if (!rc) rc = skk_product(h, h->skk_A, 0, m, Z, 0, K, lda, Dm.data(), (size_t)K);
		if (rc) return rc;
		// Phi^K = 1/2 (C + C') - D E^-1 D': the upper triangle, mirrored
		q.assign((size_t)m * K, 0.0);
		for (int j = 0; j < m; j++) skk_q(K, Einv, e_ok, &Dm[(size_t)j * K], &q[(size_t)j * K]);
		for (int j = 0; j < m; j++)
			for (int l = j; l < m; l++) {
				double v = skk_phi_entry(K, Cm[(size_t)j * m + l], Cm[(size_t)l * m + j], &Dm[(size_t)j * K], &Dm[(size_t)l * K],
					&q[(size_t)j * K], &q[(size_t)l * K]);
				if (bad[e0 + j] || bad[e0 + l]) v = NAN;
				phi[(size_t)j * m + l] = v;
				phi[(size_t)l * m + j] = v;
			}
		for (int j = 0; j < m; j++) if (bad[e0 + j]) score[e0 + j] = NAN;
		h->skk_ms[2] += skk_ms_since(t_con);
	}
	return SGX_OK;
}

// tables with the non-finite ones replaced by zeros (a column of zeros takes no step of the solve) and flagged
static void skk_tables(const double *lut, size_t m, std::vector<double> &lut_ok, std::vector<uint8_t> &bad)
{
	lut_ok.assign(lut, lut + m * 4);
	bad.assign(m, 0);
	for (size_t e = 0; e < m; e++) {
		for (int c = 0; c < 4; c++) if (!std::isfinite(lut[4 * e + c])) bad[e] = 1;
		if (bad[e]) for (int c = 0; c < 4; c++) lut_ok[4 * e + c] = 0;
	}
}

extern "C" int sgx_skat_kmat_2bit(sgx_handle *h, sgx_kmat *km, const uint8_t *packed, size_t bpv, size_t n_variants,
	size_t n_units, const int64_t *unit_ptr, const int32_t *var_idx, const double *lut, const double *w,
	const double *tau, int maxiter, double tol, double *score, double *cov, int32_t *iters)
{
	const char *who = "sgx_skat_kmat_2bit";
	if (!h || !km) return fail(SGX_EINVAL, "%s: NULL handle", who);
	if (!packed || !unit_ptr || !var_idx || !lut || !w || !tau || !score || !cov) return fail(SGX_EINVAL, "%s: NULL buffer", who);
	const int N = h->md.N;
	int rc = skk_km_check(who, h, km);
	if (rc) return rc;
	rc = bpv_check(bpv, N);
	if (!rc) rc = skk_sigma_args(who, N, w, tau, maxiter);
	if (rc) return rc;
	if (n_units == 0) return SGX_OK;
	rc = skat_units_check(who, n_units, unit_ptr, var_idx, n_variants);
	if (rc) return rc;
	const int64_t nnz = unit_ptr[n_units];
	if (nnz == 0) return SGX_OK;
	rc = begin_call(h);
	if (rc) return rc;
	hipStream_t st = h->stream;
	auto t_col = std::chrono::steady_clock::now();
	h->skk_ms[0] = h->skk_ms[1] = h->skk_ms[2] = 0;

	// an entry with a non-finite table stays out of the sums and the solve (a table of zeros: a right-hand side of
	// zeros takes no step) and gets its non-finite results at the end
	std::vector<double> lut_ok;
	std::vector<uint8_t> bad;
	skk_tables(lut, (size_t)nnz, lut_ok, bad);
	int64_t m_max = 0;
	for (size_t u = 0; u < n_units; u++) m_max = std::max(m_max, unit_ptr[u + 1] - unit_ptr[u]);

	// device copies: the rows (dword stride) in the host-row pipeline's chunks, then entries and tables
	const int ndw = (N + 15) >> 4;
	const size_t dbpv = (size_t)ndw * 4;
	TabLayout tl;
	tl.add<uint8_t>(n_variants * dbpv);
	const auto s_idx = tl.add(nnz, var_idx);
	const auto s_lut = tl.add(nnz * 4, lut_ok.data());
	rc = dev_room(h->stage_pk, tl.bytes(), "the rows", who);
	if (!rc) rc = skk_unit_room(who, h, (size_t)m_max);
	if (rc) return rc;
	rc = rows_2bit_upload(h, h->stage_pk, dbpv, packed, bpv, n_variants, st);
	if (rc) return rc;
	rc = tabs_upload(h->stage_pk, st, s_idx, s_lut);
	if (rc) return rc;
	SkkSrc src;
	src.idx = tl.at(h->stage_pk, s_idx);
	src.rows = h->stage_pk; src.dbpv = dbpv;
	src.lut = tl.at(h->stage_pk, s_lut);
	return skk_units(who, h, km, src, n_units, unit_ptr, bad, (size_t)m_max, w, tau, maxiter, tol, t_col, score, cov, iters);
}

// milliseconds of the last sgx_skat_kmat_2bit / sgx_ds_block_skat_kmat call on this handle, as the host saw them: ms[0] rows, tables and columns,
// ms[1] the solves, ms[2] the products and the host's last step
extern "C" int sgx_skat_kmat_ms(sgx_handle *h, double *ms)
{
	if (!h || !ms) return fail(SGX_EINVAL, "sgx_skat_kmat_ms: NULL argument");
	for (int i = 0; i < 3; i++) ms[i] = h->skk_ms[i];
	return SGX_OK;
}
