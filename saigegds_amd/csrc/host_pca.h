// host_pca.h -- top principal components of the GRM of a sgx_grm handle: block subspace iteration with Rayleigh-Ritz
// around the operator's product (host_grm.h) on the tall-skinny kernels of kern_tsblock.h.
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.

// With PCA_HOST_ONLY the two dense routines alone, without HIP: tests/pca_check.cpp builds them with the host compiler.

#ifdef PCA_HOST_ONLY
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#define GRM_MAX_RHS 64
#else
static_assert(TS_SLAB == SGX_TS_SLAB, "kern_tsblock.h and saigehip.h disagree on the slab of ts_gram");
#endif

// ---- the small dense steps, on the host in double: plain loops in a fixed order, so their bits hang on the input only

// C [L][L] (symmetric, the upper triangle is read) = R'R -> Ti = R^-1, upper triangular [L][L], so that Q Ti has the
// Gram matrix I.  false: a pivot <= L 2^-52 max_j C_jj, the columns are dependent to working precision.
static bool pca_chol_rinv(int L, const double *C, double *R, double *Ti)
{
	double dmax = 0;
	for (int j = 0; j < L; j++) dmax = std::max(dmax, C[j * L + j]);
	const double thr = (double)L * 0x1p-52 * dmax;
	for (int k = 0; k < L * L; k++) R[k] = Ti[k] = 0;
	for (int j = 0; j < L; j++)
		for (int i = 0; i <= j; i++) {
			double s = C[i * L + j];
			for (int k = 0; k < i; k++) s -= R[k * L + i] * R[k * L + j];
			if (i < j) { R[i * L + j] = s / R[i * L + i]; continue; }
			if (!(s > thr)) return false;          // (a NaN fails too)
			R[j * L + j] = std::sqrt(s);
		}
	for (int j = 0; j < L; j++) {
		Ti[j * L + j] = 1 / R[j * L + j];
		for (int i = j - 1; i >= 0; i--) {
			double s = 0;
			for (int k = i; k < j; k++) s += Ti[i * L + k] * R[k * L + j];
			Ti[i * L + j] = -s / R[j * L + j];
		}
	}
	return true;
}

// H [L][L] symmetric (destroyed) = V diag(theta) V', theta descending (equal values in the order Jacobi left them),
// V [L][L] with eigenvector c in column c.  Cyclic Jacobi, pairs (p, q) in row order, until a sweep finds every
// off-diagonal entry negligible beside the diagonal's (at most PCA_JACOBI_SWEEPS sweeps).
#define PCA_JACOBI_SWEEPS 60
static void pca_jacobi(int L, double *H, double *V, double *theta)
{
	for (int k = 0; k < L * L; k++) V[k] = 0;
	for (int j = 0; j < L; j++) V[j * L + j] = 1;
	for (int sweep = 0; sweep < PCA_JACOBI_SWEEPS; sweep++) {
		bool rotated = false;
		for (int p = 0; p < L - 1; p++)
			for (int q = p + 1; q < L; q++) {
				const double hpq = H[p * L + q];
				if (std::fabs(hpq) <= 0x1p-60 * std::sqrt(std::fabs(H[p * L + p] * H[q * L + q])) || hpq == 0) {
					H[p * L + q] = H[q * L + p] = 0;
					continue;
				}
				rotated = true;
				const double tau = (H[q * L + q] - H[p * L + p]) / (2 * hpq);
				const double t = (tau >= 0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1 + tau * tau));
				const double c = 1 / std::sqrt(1 + t * t), s = t * c;
				for (int k = 0; k < L; k++) {          // columns p, q
					const double a = H[k * L + p], b = H[k * L + q];
					H[k * L + p] = c * a - s * b; H[k * L + q] = s * a + c * b;
				}
				for (int k = 0; k < L; k++) {          // rows p, q
					const double a = H[p * L + k], b = H[q * L + k];
					H[p * L + k] = c * a - s * b; H[q * L + k] = s * a + c * b;
				}
				H[p * L + q] = H[q * L + p] = 0;
				for (int k = 0; k < L; k++) {
					const double a = V[k * L + p], b = V[k * L + q];
					V[k * L + p] = c * a - s * b; V[k * L + q] = s * a + c * b;
				}
			}
		if (!rotated) break;
	}
	int ord[GRM_MAX_RHS];
	for (int j = 0; j < L; j++) ord[j] = j;
	std::stable_sort(ord, ord + L, [&](int a, int b) { return H[a * L + a] > H[b * L + b]; });
	std::vector<double> Vs((size_t)L * L);
	for (int c = 0; c < L; c++) {
		theta[c] = H[ord[c] * L + ord[c]];
		for (int k = 0; k < L; k++) Vs[k * L + c] = V[k * L + ord[c]];
	}
	memcpy(V, Vs.data(), (size_t)L * L * sizeof(double));
}

#ifndef PCA_HOST_ONLY
// ---- the block kernels on the handle's stream and scratch; blocks are device arrays of n rows

// C (host, [La][Lb]) = A'B; synchronous
static int ts_gram_run(sgx_grm *g, int n, const double *A, size_t lda, int La, const double *B, size_t ldb, int Lb, double *C)
{
	hipStream_t st = g->stream;
	const int nslab = (n + TS_SLAB - 1) / TS_SLAB;
	HIPCHK(g->ts_part.reserve((size_t)nslab * GRM_MAX_RHS * GRM_MAX_RHS));
	HIPCHK(g->ts_C.reserve(GRM_MAX_RHS * GRM_MAX_RHS));
	hipLaunchKernelGGL(ts_gram_kernel, dim3((unsigned)nslab), dim3(256), 0, st, A, lda, La, B, ldb, Lb, n, g->ts_part);
	hipLaunchKernelGGL(ts_gram_reduce_kernel, dim3((unsigned)((La * Lb + 255) / 256)), dim3(256), 0, st, g->ts_part, nslab,
		La, Lb, g->ts_C);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(C, g->ts_C, (size_t)La * Lb * sizeof(double), hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	return SGX_OK;
}

// Out = A T, T on the host [La][Lc]; asynchronous (T is taken before the return)
static int ts_apply_run(sgx_grm *g, int n, const double *A, size_t lda, int La, const double *T, int Lc, double *Out, size_t ldo)
{
	hipStream_t st = g->stream;
	HIPCHK(g->ts_T.reserve(GRM_MAX_RHS * GRM_MAX_RHS));
	HIPCHK(hipMemcpyAsync(g->ts_T, T, (size_t)La * Lc * sizeof(double), hipMemcpyHostToDevice, st));
	HIPCHK(hipStreamSynchronize(st));          // (T may be the caller's local)
	hipLaunchKernelGGL(ts_apply_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)((Lc + TS_AC - 1) / TS_AC)), dim3(256), 0, st,
		A, lda, La, g->ts_T, Lc, n, Out, ldo);
	HIPCHK(hipGetLastError());
	return SGX_OK;
}

// ---- the kernels alone, on host blocks of any row count n (the tests' way in): A [La][lda], B [Lb][ldb] -> C [La][Lb];
// A [La][lda], T [La][Lc] -> Out [Lc][ldo].  The whole arrays go to the device, padding included.
static int ts_test_args(const char *fn, sgx_grm *g, int n, size_t ld, int L)
{
	if (!g) return fail(SGX_EINVAL, "%s: NULL handle", fn);
	if (n < 1) return fail(SGX_EINVAL, "%s: n=%d < 1", fn, n);
	if (L < 1 || L > SGX_GRM_MAX_RHS) return fail(SGX_EINVAL, "%s: %d columns outside 1..%d", fn, L, SGX_GRM_MAX_RHS);
	if (ld < (size_t)n) return fail(SGX_EINVAL, "%s: ld=%zu < n=%d", fn, ld, n);
	return SGX_OK;
}

extern "C" int sgx_grm_ts_gram(sgx_grm *g, int32_t n, const double *A, size_t lda, int La, const double *B, size_t ldb, int Lb,
	double *C)
{
	if (!A || !B || !C) return fail(SGX_EINVAL, "sgx_grm_ts_gram: NULL argument");
	int rc = ts_test_args("sgx_grm_ts_gram", g, n, lda, La);
	if (!rc) rc = ts_test_args("sgx_grm_ts_gram", g, n, ldb, Lb);
	if (rc) return rc;
	HIPCHK(hipSetDevice(g->device));
	DevBuf<double> dA, dB;                     // the call's own: it waits for the stream before they go
	HIPCHK(dA.alloc((size_t)La * lda));
	HIPCHK(hipMemcpyAsync(dA, A, (size_t)La * lda * sizeof(double), hipMemcpyHostToDevice, g->stream));
	const bool same = A == B && lda == ldb && La == Lb;
	if (!same) {
		HIPCHK(dB.alloc((size_t)Lb * ldb));
		HIPCHK(hipMemcpyAsync(dB, B, (size_t)Lb * ldb * sizeof(double), hipMemcpyHostToDevice, g->stream));
	}
	rc = ts_gram_run(g, n, dA.p, lda, La, same ? dA.p : dB.p, ldb, Lb, C);
	(void)hipStreamSynchronize(g->stream);
	return rc;
}

extern "C" int sgx_grm_ts_apply(sgx_grm *g, int32_t n, const double *A, size_t lda, int La, const double *T, int Lc,
	double *Out, size_t ldo)
{
	if (!A || !T || !Out) return fail(SGX_EINVAL, "sgx_grm_ts_apply: NULL argument");
	int rc = ts_test_args("sgx_grm_ts_apply", g, n, lda, La);
	if (!rc) rc = ts_test_args("sgx_grm_ts_apply", g, n, ldo, Lc);
	if (rc) return rc;
	HIPCHK(hipSetDevice(g->device));
	DevBuf<double> dA, dO;
	HIPCHK(dA.alloc((size_t)La * lda));
	HIPCHK(dO.alloc((size_t)Lc * ldo));
	HIPCHK(hipMemcpyAsync(dA, A, (size_t)La * lda * sizeof(double), hipMemcpyHostToDevice, g->stream));
	// (Out's padding comes back as it went in: rows >= n are not the kernel's to write)
	HIPCHK(hipMemcpyAsync(dO, Out, (size_t)Lc * ldo * sizeof(double), hipMemcpyHostToDevice, g->stream));
	rc = ts_apply_run(g, n, dA, lda, La, T, Lc, dO, ldo);
	if (!rc && hipMemcpyAsync(Out, dO, (size_t)Lc * ldo * sizeof(double), hipMemcpyDeviceToHost, g->stream) != hipSuccess)
		rc = fail(SGX_EHIP, "sgx_grm_ts_apply: copy to the host failed");
	(void)hipStreamSynchronize(g->stream);
	return rc;
}

// ---- the solver

// Q (L columns, ld = N) -> orthonormal columns of the same span, in place: CholeskyQR twice through tmp.
// SGX_ERANK: the columns are dependent to working precision.
static int pca_orthonormalise(sgx_grm *g, int L, double *Q, double *tmp, double *C, double *R, double *Ti)
{
	const int N = g->N;
	double *src = Q, *dst = tmp;
	for (int pass = 0; pass < 2; pass++) {
		int rc = ts_gram_run(g, N, src, (size_t)N, L, src, (size_t)N, L, C);
		if (rc) return rc;
		if (!pca_chol_rinv(L, C, R, Ti))
			return fail(SGX_ERANK, "sgx_grm_pca: the block of %d vectors lost rank: the markers span fewer directions", L);
		if ((rc = ts_apply_run(g, N, src, (size_t)N, L, Ti, L, dst, (size_t)N))) return rc;
		std::swap(src, dst);
	}
	return SGX_OK;
}

extern "C" int sgx_grm_pca(sgx_grm *g, int n_pc, int n_block, const double *Q0, size_t ld0, int max_iter, double tol,
	double *eigval, double *resid, double *vec, size_t ldv, double *loading, size_t ldl, sgx_grm_pca_stats *stats)
{
	if (!g || !Q0 || !eigval || !resid || !vec) return fail(SGX_EINVAL, "sgx_grm_pca: NULL argument");
	if (n_pc < 1 || n_block < n_pc || n_block > SGX_GRM_MAX_RHS || n_block > g->N)
		return fail(SGX_EINVAL, "sgx_grm_pca: n_pc=%d, n_block=%d: need 1 <= n_pc <= n_block <= min(%d, N=%d)", n_pc, n_block,
			SGX_GRM_MAX_RHS, g->N);
	if (ld0 < (size_t)g->N || ldv < (size_t)g->N) return fail(SGX_EINVAL, "sgx_grm_pca: ld0=%zu or ldv=%zu < N=%d", ld0, ldv, g->N);
	if (loading && ldl < g->M) return fail(SGX_EINVAL, "sgx_grm_pca: ldl=%zu < M=%zu", ldl, g->M);
	if (!std::isfinite(tol) || tol < 0) return fail(SGX_EINVAL, "sgx_grm_pca: tol is not a finite number >= 0");
	if (max_iter < 1) return fail(SGX_EINVAL, "sgx_grm_pca: max_iter=%d < 1", max_iter);
	HIPCHK(hipSetDevice(g->device));
	hipStream_t st = g->stream;
	const int L = n_block, N = g->N;
	const size_t Nz = (size_t)N, M = g->M;
	HIPCHK(hipStreamSynchronize(st));
	for (DevBuf<double> *b : {&g->pca_X0, &g->pca_X1, &g->pca_Y, &g->pca_W}) HIPCHK(b->reserve((size_t)L * Nz));
	if (loading) HIPCHK(g->md_out.reserve((size_t)n_pc * M));
	double *X0 = g->pca_X0, *X1 = g->pca_X1, *Y = g->pca_Y, *W = g->pca_W;
	HIPCHK(hipMemcpy2DAsync(X0, Nz * sizeof(double), Q0, ld0 * sizeof(double), Nz * sizeof(double), (size_t)L,
		hipMemcpyHostToDevice, st));
	std::vector<double> C((size_t)L * L), R((size_t)L * L), T((size_t)L * L), H((size_t)L * L), V((size_t)L * L);
	std::vector<double> theta(L), r(L);
	sgx_grm_pca_stats sx{};
	const auto t_begin = std::chrono::steady_clock::now();
	int rc;
	for (int it = 1;; it++) {
		if ((rc = pca_orthonormalise(g, L, X0, X1, C.data(), R.data(), T.data()))) return rc;
		// Y = K Q
		HIPCHK(hipStreamSynchronize(st));
		const auto t0 = std::chrono::steady_clock::now();
		if ((rc = grm_matvec_dev(g, X0, Nz, pcg_cols_iota(L), Y, Nz))) return rc;
		HIPCHK(hipStreamSynchronize(st));
		sx.ms_products += gd_ms_since(t0);
		// H = Q'Y, symmetrised; H = V Theta V'
		if ((rc = ts_gram_run(g, N, X0, Nz, L, Y, Nz, L, C.data()))) return rc;
		for (int a = 0; a < L; a++)
			for (int b = 0; b < L; b++) H[a * L + b] = (C[a * L + b] + C[b * L + a]) / 2;
		pca_jacobi(L, H.data(), V.data(), theta.data());
		// U = Q V -> X1, W = Y V -> W, R = W - theta U -> Y, r_c = |R_c|
		if ((rc = ts_apply_run(g, N, X0, Nz, L, V.data(), L, X1, Nz))) return rc;
		if ((rc = ts_apply_run(g, N, Y, Nz, L, V.data(), L, W, Nz))) return rc;
		GrmScal th{};
		for (int c = 0; c < L; c++) th.v[c] = theta[c];
		hipLaunchKernelGGL(ts_axpy_cols_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)L), dim3(256), 0, st, W, Nz, X1, Nz, th,
			N, Y, Nz);
		HIPCHK(hipGetLastError());
		if ((rc = ts_gram_run(g, N, Y, Nz, L, Y, Nz, L, C.data()))) return rc;
		for (int c = 0; c < L; c++) r[c] = std::sqrt(C[c * L + c]);
		sx.iters = it;
		sx.n_converged = 0;
		bool all = true;
		for (int c = 0; c < n_pc; c++) {
			const bool ok = r[c] <= tol * theta[0];
			if (ok && all) sx.n_converged = c + 1;
			all = all && ok;
		}
		if (all || it >= max_iter) break;
		std::swap(X0, W);                      // the next block is W
	}
	// outputs: U is in X1
	std::vector<double> sign(n_pc, 1.0);
	HIPCHK(hipMemcpy2DAsync(vec, ldv * sizeof(double), X1, Nz * sizeof(double), Nz * sizeof(double), (size_t)n_pc,
		hipMemcpyDeviceToHost, st));
	if (loading) {
		if ((rc = grm_marker_dots_run(g, X1, Nz, n_pc, g->md_out, M))) return rc;
		HIPCHK(hipMemcpy2DAsync(loading, ldl * sizeof(double), g->md_out, M * sizeof(double), M * sizeof(double), (size_t)n_pc,
			hipMemcpyDeviceToHost, st));
	}
	HIPCHK(hipStreamSynchronize(st));
	for (int c = 0; c < n_pc; c++) {
		double *u = vec + (size_t)c * ldv;
		size_t best = 0;
		for (size_t i = 1; i < Nz; i++)
			if (std::fabs(u[i]) > std::fabs(u[best])) best = i;
		if (u[best] < 0) {
			sign[c] = -1;
			for (size_t i = 0; i < Nz; i++) u[i] = -u[i];
		}
		eigval[c] = theta[c];
		resid[c] = r[c];
		if (loading) {
			double *l = loading + (size_t)c * ldl;
			const double sc = theta[c] > 0 ? sign[c] / std::sqrt((double)M * theta[c]) : 0.0;
			for (size_t v = 0; v < M; v++) l[v] = theta[c] > 0 ? l[v] * sc : 0.0;
		}
	}
	const double ms_all = gd_ms_since(t_begin);
	sx.ms_block = ms_all - sx.ms_products;
	if (stats) *stats = sx;
	return SGX_OK;
}
#endif   // PCA_HOST_ONLY
