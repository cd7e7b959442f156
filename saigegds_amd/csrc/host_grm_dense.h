// host_grm_dense.h -- the explicit GRM of a sgx_grm handle (kern_grm_dense.h): dense rectangles and
// the thresholded sparse matrix.
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.

#include <chrono>

#define GD_RECT 2048          /* sgx_grm_dense works in pieces of at most GD_RECT x GD_RECT entries          */
#define GD_BATCH 16384        /* flagged sub-tiles per FP64 launch of sgx_grm_sparse                         */

static double gd_ms_since(std::chrono::steady_clock::time_point t0)
{
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

static int gd_nslab(const sgx_grm *g)
{
	const size_t ndw = (g->M + 15) >> 4;
	return (int)((ndw + GD_SLAB_DW - 1) / GD_SLAB_DW);
}

// one piece of a rectangle: its tile grid in FP64, gathered into g->gd_out [ni][nj], copied to the host
static int gd_rect(sgx_grm *g, int i0, int ni, int j0, int nj, double *out, size_t ld)
{
	hipStream_t st = g->stream;
	const int ti0 = i0 / 16, nti = (i0 + ni - 1) / 16 - ti0 + 1;
	const int tj0 = j0 / 16, ntj = (j0 + nj - 1) / 16 - tj0 + 1;
	const size_t n_tiles = (size_t)nti * ntj;
	const int nslab = gd_nslab(g);
	HIPCHK(g->gd_part.reserve((size_t)nslab * n_tiles * 256));
	HIPCHK(g->gd_out.reserve((size_t)ni * nj));
	if (!g->gd_ev1) { if (!g->gd_ev0) HIPCHK(g->gd_ev0.create()); HIPCHK(g->gd_ev1.create()); }
	HIPCHK(hipEventRecord(g->gd_ev0, st));
	hipLaunchKernelGGL(grm_dense_tile_kernel, dim3((unsigned)n_tiles, (unsigned)nslab), dim3(WAVE), 0, st, g->Gt, g->bpvM,
		g->N, g->M, g->inv, g->l0, (const GdTile *)nullptr, ti0, nti, tj0, ntj, n_tiles, g->gd_part);
	hipLaunchKernelGGL(grm_dense_gather_kernel, dim3((unsigned)(((size_t)ni * nj + 255) / 256)), dim3(256), 0, st,
		g->gd_part, n_tiles, nslab, ti0, nti, tj0, ntj, i0, ni, j0, nj, g->M, g->gd_out);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(g->gd_ev1, st));
	HIPCHK(hipMemcpy2DAsync(out, ld * sizeof(double), g->gd_out, (size_t)nj * sizeof(double), (size_t)nj * sizeof(double),
		(size_t)ni, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, g->gd_ev0, g->gd_ev1));
	g->gd_ms_kernel += ms;
	return SGX_OK;
}

extern "C" int sgx_grm_dense_kernel_ms(sgx_grm *g, double *ms_out)
{
	if (!g || !ms_out) return fail(SGX_EINVAL, "sgx_grm_dense_kernel_ms: NULL argument");
	*ms_out = g->gd_ms_kernel;
	return SGX_OK;
}

extern "C" int sgx_grm_dense(sgx_grm *g, int32_t i0, int32_t ni, int32_t j0, int32_t nj, double *out, size_t ld)
{
	if (!g || !out) return fail(SGX_EINVAL, "sgx_grm_dense: NULL argument");
	if (i0 < 0 || ni < 0 || j0 < 0 || nj < 0 || (int64_t)i0 + ni > g->N || (int64_t)j0 + nj > g->N)
		return fail(SGX_EINVAL, "sgx_grm_dense: rows %d..+%d, columns %d..+%d outside [0, %d)", i0, ni, j0, nj, g->N);
	if (ld < (size_t)nj) return fail(SGX_EINVAL, "sgx_grm_dense: ld=%zu < nj=%d", ld, nj);
	if (ni == 0 || nj == 0) return SGX_OK;
	HIPCHK(hipSetDevice(g->device));
	g->gd_ms_kernel = 0;
	for (int a = 0; a < ni; a += GD_RECT)
		for (int b = 0; b < nj; b += GD_RECT) {
			int rc = gd_rect(g, i0 + a, std::min(GD_RECT, ni - a), j0 + b, std::min(GD_RECT, nj - b),
				out + (size_t)a * ld + b, ld);
			if (rc) return rc;
		}
	return SGX_OK;
}

// the screen's tables, once per handle: s from the largest |g| of the marker table, the limb bytes, A and R
static int gd_prepare(sgx_grm *g)
{
	if (g->gd_ready) return SGX_OK;
	hipStream_t st = g->stream;
	const size_t M = g->M, Mpad = g->bpvM * 4, N = (size_t)g->N;
	HIPCHK(g->gd_cnt.reserve(2));
	HIPCHK(g->gd_lut.reserve(Mpad));
	HIPCHK(g->gd_A.reserve(N));
	HIPCHK(g->gd_R.reserve(N));
	HIPCHK(hipMemsetAsync(g->gd_cnt, 0, 2 * sizeof(unsigned long long), st));
	hipLaunchKernelGGL(gd_lutmax_kernel, dim3(GRM_RED_BLOCKS), dim3(256), 0, st, g->inv, g->l0, M, g->gd_cnt);
	unsigned long long bits = 0;
	HIPCHK(hipMemcpyAsync(&bits, g->gd_cnt, sizeof bits, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	double gmax;
	memcpy(&gmax, &bits, sizeof gmax);
	int s = 0;
	if (gmax > 0 && std::isfinite(gmax)) {
		s = std::max(-60, std::min(60, (int)std::floor(std::log2((double)GD_QMAX / gmax))));
		while (s > -60 && std::ldexp(gmax, s) > (double)GD_QMAX) s--;
		if (std::ldexp(gmax, s) > (double)GD_QMAX) return fail(SGX_EINVAL, "sgx_grm_sparse: marker table out of range");
	}
	g->gd_s = s;
	hipLaunchKernelGGL(gd_lut_kernel, dim3((unsigned)((Mpad + 255) / 256)), dim3(256), 0, st, g->inv, g->l0, M, Mpad, s,
		g->gd_lut);
	hipLaunchKernelGGL(gd_sample_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, g->Gt, g->bpvM, g->N, M, g->inv,
		g->l0, g->diag, g->gd_A, g->gd_R);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(st));
	g->gd_ready = true;
	return SGX_OK;
}

extern "C" int sgx_grm_sparse(sgx_grm *g, double cutoff, size_t cap, int32_t *i_out, int32_t *j_out, double *v_out,
	size_t *n_out, sgx_grm_sparse_stats *stats)
{
	if (!g || !n_out || (cap > 0 && (!i_out || !j_out || !v_out))) return fail(SGX_EINVAL, "sgx_grm_sparse: NULL argument");
	if (!std::isfinite(cutoff)) return fail(SGX_EINVAL, "sgx_grm_sparse: the cutoff is not finite");
	HIPCHK(hipSetDevice(g->device));
	hipStream_t st = g->stream;
	const size_t N = (size_t)g->N, M = g->M;
	sgx_grm_sparse_stats sx{};
	auto t0 = std::chrono::steady_clock::now();
	const bool first = !g->gd_ready;
	int rc = gd_prepare(g);
	if (rc) return rc;
	if (first) sx.ms_prepare = gd_ms_since(t0);
	sx.s = g->gd_s;

	// ---- screen
	t0 = std::chrono::steady_clock::now();
	const size_t nb = (N + GD_T - 1) / GD_T, nst = (N + 15) / 16;
	const size_t st_total = nst * (nst + 1) / 2;
	sx.tiles_screened = (int64_t)(nb * (nb + 1) / 2);
	sx.subtiles_total = (int64_t)st_total;
	GdBound bd{};
	bd.p2 = std::ldexp(1.0, -2 * g->gd_s);
	bd.Md = (double)M;
	bd.qa = std::ldexp(1.0, -(g->gd_s + 1)) / (double)M * (1.0 + 0x1p-20);
	bd.qb = std::ldexp(1.0, -(2 * g->gd_s + 2));
	bd.rc = 4.0 * ((double)M + 8.0) * 0x1p-53;
	bd.cutoff = cutoff;
	unsigned long long n_flag = 0;
	for (size_t want = std::min(st_total, std::max<size_t>(4 * nst + 4096, st_total / 64));;) {
		HIPCHK(g->gd_list.reserve(want));
		HIPCHK(hipMemsetAsync(g->gd_cnt, 0, 2 * sizeof(unsigned long long), st));
		hipLaunchKernelGGL(grm_screen_kernel, dim3((unsigned)nb, (unsigned)nb), dim3(256), 0, st, g->Gt, g->bpvM, g->N,
			(int)(g->bpvM * 4 / GD_KB), g->gd_lut, g->gd_A, g->gd_R, bd, g->gd_list, g->gd_cnt, g->gd_list.cap);
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpyAsync(&n_flag, g->gd_cnt, sizeof n_flag, hipMemcpyDeviceToHost, st));
		HIPCHK(hipStreamSynchronize(st));
		if (n_flag <= g->gd_list.cap) break;
		want = (size_t)n_flag;                         // (the list was too short: once more with room for all)
	}
	sx.subtiles_flagged = (int64_t)n_flag;
	sx.ms_screen = gd_ms_since(t0);

	// ---- FP64 on the flagged sub-tiles, threshold, compact
	t0 = std::chrono::steady_clock::now();
	// (room for what the flagged sub-tiles can hold at most, not for whatever the caller's cap allows)
	const size_t ent_cap = std::max<size_t>(1, std::min(cap, (size_t)n_flag * 256));
	HIPCHK(g->gd_i.reserve(ent_cap));
	HIPCHK(g->gd_j.reserve(ent_cap));
	HIPCHK(g->gd_v.reserve(ent_cap));
	const int nslab = gd_nslab(g);
	for (size_t f0 = 0; f0 < (size_t)n_flag; f0 += GD_BATCH) {
		const size_t nt = std::min<size_t>(GD_BATCH, (size_t)n_flag - f0);
		HIPCHK(g->gd_part.reserve((size_t)nslab * nt * 256));
		hipLaunchKernelGGL(grm_dense_tile_kernel, dim3((unsigned)nt, (unsigned)nslab), dim3(WAVE), 0, st, g->Gt, g->bpvM,
			g->N, M, g->inv, g->l0, g->gd_list + f0, 0, 0, 0, 1, nt, g->gd_part);
		hipLaunchKernelGGL(grm_sparse_compact_kernel, dim3((unsigned)nt), dim3(256), 0, st, g->gd_part, nt, nslab,
			g->gd_list + f0, g->N, M, cutoff, g->gd_i, g->gd_j, g->gd_v, g->gd_cnt + 1, ent_cap);
		HIPCHK(hipGetLastError());
	}
	unsigned long long n_ent = 0;
	HIPCHK(hipMemcpyAsync(&n_ent, g->gd_cnt + 1, sizeof n_ent, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	sx.ms_fp64 = gd_ms_since(t0);
	sx.entries = (int64_t)n_ent;
	*n_out = (size_t)n_ent;
	if (n_ent > cap) {
		if (stats) *stats = sx;
		return fail(SGX_ENOSPACE, "sgx_grm_sparse: %llu entries, room for %zu", n_ent, cap);
	}

	// ---- to the host, sorted by (i, j)
	t0 = std::chrono::steady_clock::now();
	const size_t n = (size_t)n_ent;
	std::vector<int> hi(n), hj(n);
	std::vector<double> hv(n);
	if (n) {
		HIPCHK(hipMemcpyAsync(hi.data(), g->gd_i, n * sizeof(int), hipMemcpyDeviceToHost, st));
		HIPCHK(hipMemcpyAsync(hj.data(), g->gd_j, n * sizeof(int), hipMemcpyDeviceToHost, st));
		HIPCHK(hipMemcpyAsync(hv.data(), g->gd_v, n * sizeof(double), hipMemcpyDeviceToHost, st));
		HIPCHK(hipStreamSynchronize(st));
	}
	std::vector<size_t> ord(n);
	for (size_t k = 0; k < n; k++) ord[k] = k;
	std::sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return hi[a] != hi[b] ? hi[a] < hi[b] : hj[a] < hj[b]; });
	for (size_t k = 0; k < n; k++) { i_out[k] = hi[ord[k]]; j_out[k] = hj[ord[k]]; v_out[k] = hv[ord[k]]; }
	sx.ms_sort = gd_ms_since(t0);
	if (stats) *stats = sx;
	return SGX_OK;
}
