// host_king.h -- KING-robust kinship of a sgx_grm handle (kern_king.h): the counts of a rectangle of
// pairs and the list of related pairs.
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.

#define KG_RECT 2048          /* sgx_grm_king_counts works in pieces of at most KG_RECT x KG_RECT pairs (80 MiB) */

extern "C" int sgx_grm_king_counts(sgx_grm *g, int32_t i0, int32_t ni, int32_t j0, int32_t nj, int32_t *out, size_t ld)
{
	if (!g || !out) return fail(SGX_EINVAL, "sgx_grm_king_counts: NULL argument");
	if (i0 < 0 || ni < 0 || j0 < 0 || nj < 0 || (int64_t)i0 + ni > g->N || (int64_t)j0 + nj > g->N)
		return fail(SGX_EINVAL, "sgx_grm_king_counts: rows %d..+%d, columns %d..+%d outside [0, %d)", i0, ni, j0, nj, g->N);
	if (ld < (size_t)nj) return fail(SGX_EINVAL, "sgx_grm_king_counts: ld=%zu < nj=%d", ld, nj);
	if (ni == 0 || nj == 0) return SGX_OK;
	HIPCHK(hipSetDevice(g->device));
	hipStream_t st = g->stream;
	for (int a = 0; a < ni; a += KG_RECT)
		for (int b = 0; b < nj; b += KG_RECT) {
			const int pi = std::min(KG_RECT, ni - a), pj = std::min(KG_RECT, nj - b);
			const size_t plane = (size_t)pi * pj;
			HIPCHK(g->kg_out.reserve(5 * plane));
			hipLaunchKernelGGL(king_counts_kernel, dim3((unsigned)((pj + KG_T - 1) / KG_T), (unsigned)((pi + KG_T - 1) / KG_T)),
				dim3(256), 0, st, g->Gt, g->bpvM, g->N, g->M, i0 + a, pi, j0 + b, pj, g->kg_out);
			HIPCHK(hipGetLastError());
			for (int q = 0; q < 5; q++)
				HIPCHK(hipMemcpy2DAsync(out + ((size_t)q * ni + a) * ld + b, ld * sizeof(int32_t), g->kg_out + q * plane,
					(size_t)pj * sizeof(int32_t), (size_t)pj * sizeof(int32_t), (size_t)pi, hipMemcpyDeviceToHost, st));
			HIPCHK(hipStreamSynchronize(st));              // (the next piece reuses kg_out)
		}
	return SGX_OK;
}

extern "C" int sgx_grm_king_pairs(sgx_grm *g, double cutoff, size_t cap, int32_t *i_out, int32_t *j_out, double *kin_out,
	double *ibs0_out, int32_t *counts_out, size_t *n_out, sgx_grm_king_stats *stats)
{
	if (!g || !n_out || (cap > 0 && (!i_out || !j_out || !kin_out || !ibs0_out)))
		return fail(SGX_EINVAL, "sgx_grm_king_pairs: NULL argument");
	if (!std::isfinite(cutoff)) return fail(SGX_EINVAL, "sgx_grm_king_pairs: the cutoff is not finite");
	HIPCHK(hipSetDevice(g->device));
	hipStream_t st = g->stream;
	const size_t N = (size_t)g->N, nb = (N + KG_T - 1) / KG_T;
	sgx_grm_king_stats sx{};
	sx.tiles = (int64_t)(nb * (nb + 1) / 2);
	// (room for the pairs that can exist at most, not for whatever the caller's cap allows)
	const size_t dcap = std::max<size_t>(1, std::min(cap, N * (N - 1) / 2));
	HIPCHK(g->kg_cnt.reserve(1));
	HIPCHK(g->kg_i.reserve(dcap));
	HIPCHK(g->kg_j.reserve(dcap));
	HIPCHK(g->kg_kin.reserve(dcap));
	HIPCHK(g->kg_ibs.reserve(dcap));
	HIPCHK(g->kg_c5.reserve(5 * dcap));
	if (!g->kg_ev1) { if (!g->kg_ev0) HIPCHK(g->kg_ev0.create()); HIPCHK(g->kg_ev1.create()); }
	HIPCHK(hipMemsetAsync(g->kg_cnt, 0, sizeof(unsigned long long), st));
	HIPCHK(hipEventRecord(g->kg_ev0, st));
	hipLaunchKernelGGL(king_pairs_kernel, dim3((unsigned)nb, (unsigned)nb), dim3(256), 0, st, g->Gt, g->bpvM, g->N, g->M,
		cutoff, g->kg_i, g->kg_j, g->kg_kin, g->kg_ibs, g->kg_c5, g->kg_cnt, std::min(cap, dcap));
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(g->kg_ev1, st));
	unsigned long long n_pair = 0;
	HIPCHK(hipMemcpyAsync(&n_pair, g->kg_cnt, sizeof n_pair, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, g->kg_ev0, g->kg_ev1));
	sx.ms_kernel = ms;
	sx.pairs = (int64_t)n_pair;
	*n_out = (size_t)n_pair;
	if (n_pair > cap) {
		if (stats) *stats = sx;
		return fail(SGX_ENOSPACE, "sgx_grm_king_pairs: %llu pairs, room for %zu", n_pair, cap);
	}

	// ---- to the host, sorted by (i, j)
	auto t0 = std::chrono::steady_clock::now();
	const size_t n = (size_t)n_pair;
	std::vector<int> hi(n), hj(n), hc(5 * n);
	std::vector<double> hk(n), hb(n);
	if (n) {
		HIPCHK(hipMemcpyAsync(hi.data(), g->kg_i, n * sizeof(int), hipMemcpyDeviceToHost, st));
		HIPCHK(hipMemcpyAsync(hj.data(), g->kg_j, n * sizeof(int), hipMemcpyDeviceToHost, st));
		HIPCHK(hipMemcpyAsync(hk.data(), g->kg_kin, n * sizeof(double), hipMemcpyDeviceToHost, st));
		HIPCHK(hipMemcpyAsync(hb.data(), g->kg_ibs, n * sizeof(double), hipMemcpyDeviceToHost, st));
		HIPCHK(hipMemcpyAsync(hc.data(), g->kg_c5, 5 * n * sizeof(int), hipMemcpyDeviceToHost, st));
		HIPCHK(hipStreamSynchronize(st));
	}
	std::vector<size_t> ord(n);
	for (size_t k = 0; k < n; k++) ord[k] = k;
	std::sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return hi[a] != hi[b] ? hi[a] < hi[b] : hj[a] < hj[b]; });
	for (size_t k = 0; k < n; k++) {
		const size_t s = ord[k];
		i_out[k] = hi[s]; j_out[k] = hj[s]; kin_out[k] = hk[s]; ibs0_out[k] = hb[s];
		if (counts_out) memcpy(counts_out + 5 * k, hc.data() + 5 * s, 5 * sizeof(int));
	}
	sx.ms_sort = gd_ms_since(t0);
	if (stats) *stats = sx;
	return SGX_OK;
}
