// host_skato.h -- sgx_skato_spectra: the eigenvalues of the SKAT-O matrices of a batch of units (DESIGN.md 8k,
// kern_eig.h).  The matrices A_u go to the device once; the problems are sorted into size classes, one launch each,
// so that many small problems do not pay the LDS and the threads of a large one.
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.

// size classes: the largest m, the threads of a workgroup.  Up to EIG_LDS_M the working matrix is in LDS.
struct EigClass { int max_m, threads; };
static const EigClass EIG_CLASSES[] = {{16, 64}, {32, 128}, {64, 256}, {EIG_LDS_M, 512}, {SGX_SKATO_MAX_M, 1024}};
static const size_t EIG_SCR_BYTES = (size_t)256 << 20;      // scratch of one launch of the class above EIG_LDS_M
static_assert(EIG_LDS_M < SGX_SKATO_MAX_M, "classes ascending");
static_assert((size_t)(eig_aux(EIG_LDS_M) + EIG_LDS_M * eig_ld(EIG_LDS_M)) * sizeof(double) <= 160 * 1024, "LDS of a CU");

extern "C" int sgx_skato_spectra(sgx_handle *h, size_t n, const int32_t *m_of, const double *mats, size_t n_rho,
	const double *rho, double *eig, int32_t *sweeps)
{
	const char *who = "sgx_skato_spectra";
	if (!h) return fail(SGX_EINVAL, "%s: NULL handle", who);
	if (h->owner) return fail(SGX_EINVAL, "%s: not on a twin", who);
	if (!rho || n_rho == 0 || n_rho > 4096) return fail(SGX_EINVAL, "%s: the rho grid needs 1 .. 4096 values", who);
	for (size_t k = 0; k < n_rho; k++)
		if (!(rho[k] >= 0 && rho[k] <= 1) || (k && !(rho[k] > rho[k - 1])))
			return fail(SGX_EINVAL, "%s: rho must be strictly increasing within [0, 1]", who);
	if (n == 0) return SGX_OK;
	if (!m_of || !mats || !eig || !sweeps) return fail(SGX_EINVAL, "%s: NULL buffer", who);
	if (n > (size_t)INT32_MAX / (n_rho + 1)) return fail(SGX_EINVAL, "%s: too many problems", who);
	const int nmat = (int)n_rho + 1;
	std::vector<long long> a_off(n), e_off(n);
	size_t na = 0, ne = 0;
	for (size_t u = 0; u < n; u++) {
		if (m_of[u] < 0 || m_of[u] > SGX_SKATO_MAX_M)
			return fail(SGX_EINVAL, "%s: problem %zu has m=%d, at most %d is supported", who, u, m_of[u], SGX_SKATO_MAX_M);
		const size_t m = (size_t)m_of[u];
		a_off[u] = (long long)na; e_off[u] = (long long)ne;
		na += m * m; ne += (size_t)nmat * m;
	}
	int rc = sync_lane(h);
	if (rc) return rc;
	h->last_issued = h;
	for (size_t i = 0; i < n * (size_t)nmat; i++) sweeps[i] = 0;
	if (na == 0) return SGX_OK;

	// (a = sqrt(1 - rho), rho) per grid value; a value above 0.999 enters as 0.999 when the grid has more than one
	std::vector<double> ab(2 * n_rho);
	// the problems by class, in the call's order
	const int ncls = (int)(sizeof EIG_CLASSES / sizeof EIG_CLASSES[0]);
	std::vector<int> plist;
	size_t cls_at[sizeof EIG_CLASSES / sizeof EIG_CLASSES[0] + 1];
	for (int c = 0; c < ncls; c++) {
		cls_at[c] = plist.size();
		const int lo = c ? EIG_CLASSES[c - 1].max_m : 0;
		for (size_t u = 0; u < n; u++)
			if (m_of[u] > lo && m_of[u] <= EIG_CLASSES[c].max_m) plist.push_back((int)u);
	}
	cls_at[ncls] = plist.size();

	// device copies: offsets, sizes, class lists, (a, b)
	const size_t o_eoff = n * sizeof(long long), o_ab = 2 * o_eoff, o_m = o_ab + 2 * n_rho * sizeof(double);
	const size_t o_pl = o_m + n * sizeof(int), need = o_pl + plist.size() * sizeof(int);
	rc = grow(h->eig_meta, need);
	if (!rc) rc = grow(h->eig_A, na);
	if (!rc) rc = grow(h->eig_out, ne);
	if (!rc) rc = grow(h->eig_sw, n * (size_t)nmat);
	if (rc) return rc;
	const long long *d_aoff = reinterpret_cast<const long long *>(h->eig_meta.p);
	const long long *d_eoff = reinterpret_cast<const long long *>(h->eig_meta + o_eoff);
	const double *d_ab = reinterpret_cast<const double *>(h->eig_meta + o_ab);
	const int *d_m = reinterpret_cast<const int *>(h->eig_meta + o_m), *d_pl = reinterpret_cast<const int *>(h->eig_meta + o_pl);
	for (size_t k = 0; k < n_rho; k++) {
		const double rk = (n_rho > 1 && rho[k] > 0.999) ? 0.999 : rho[k];
		ab[2 * k] = sqrt(1 - rk);
		ab[2 * k + 1] = rk;                                   // (b depends on m: the kernel makes it)
	}
	HIPCHK(hipMemcpyAsync(h->eig_meta.p, a_off.data(), o_eoff, hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipMemcpyAsync(h->eig_meta + o_eoff, e_off.data(), o_eoff, hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipMemcpyAsync(h->eig_meta + o_ab, ab.data(), 2 * n_rho * sizeof(double), hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipMemcpyAsync(h->eig_meta + o_m, m_of, n * sizeof(int), hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipMemcpyAsync(h->eig_meta + o_pl, plist.data(), plist.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
	HIPCHK(hipMemcpyAsync(h->eig_A.p, mats, na * sizeof(double), hipMemcpyHostToDevice, h->stream));

	for (int c = 0; c < ncls; c++) {
		const size_t np = cls_at[c + 1] - cls_at[c];
		if (np == 0) continue;
		const int M = EIG_CLASSES[c].max_m;
		const dim3 blk((unsigned)EIG_CLASSES[c].threads);
		if (M <= EIG_LDS_M) {
			const size_t lds = (size_t)(eig_aux(M) + M * eig_ld(M)) * sizeof(double);
			if (lds > 64 * 1024 && !h->eig_attr_set) {
				HIPCHK(hipFuncSetAttribute((const void *)eig_jacobi_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
				h->eig_attr_set = true;
			}
			hipLaunchKernelGGL(eig_jacobi_kernel<true>, dim3((unsigned)(np * nmat)), blk, lds, h->stream,
				h->eig_A.p, d_aoff, d_m, d_eoff, d_pl + cls_at[c], nmat, d_ab, (double *)nullptr, (size_t)0, h->eig_out.p, h->eig_sw.p);
			HIPCHK(hipGetLastError());
		} else {
			const size_t slice = (size_t)M * eig_ld(M);
			const size_t pchunk = std::max<size_t>(1, EIG_SCR_BYTES / (slice * sizeof(double)) / (size_t)nmat);
			rc = grow(h->eig_scr, std::min(np, pchunk) * nmat * slice);
			if (rc) return rc;
			for (size_t p0 = 0; p0 < np; p0 += pchunk) {
				const size_t pn = std::min(pchunk, np - p0);
				hipLaunchKernelGGL(eig_jacobi_kernel<false>, dim3((unsigned)(pn * nmat)), blk, (size_t)eig_aux(M) * sizeof(double), h->stream,
					h->eig_A.p, d_aoff, d_m, d_eoff, d_pl + cls_at[c] + p0, nmat, d_ab, h->eig_scr.p, slice, h->eig_out.p, h->eig_sw.p);
				HIPCHK(hipGetLastError());
			}
		}
	}
	HIPCHK(hipMemcpyAsync(eig, h->eig_out.p, ne * sizeof(double), hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipMemcpyAsync(sweeps, h->eig_sw.p, n * (size_t)nmat * sizeof(int), hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipStreamSynchronize(h->stream));
	for (size_t u = 0; u < n; u++)                            // (no workgroup wrote these)
		if (m_of[u] == 0) for (int k = 0; k < nmat; k++) sweeps[u * nmat + k] = 0;
	return SGX_OK;
}
