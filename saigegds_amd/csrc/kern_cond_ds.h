// kern_cond_ds.h -- the sums of the conditional scan ("Conditional analysis") from the dosage rows of a
// resident sgx_dsblock (row-major, stride N elements; uint8_t rows, or double rows for f64 and i32 blocks): what
// kern_cond.h makes from 2-bit rows, with the value of row j at sample i
//     g_j(i) = present(x) ? (flip[j] ? 2 - x : x) : mean[j],      x = rows[j][i]
// as kern_skat_ds.h defines it (skat_ds_value).  B, the per-slab partial sums, skat_reduce_kernel and
// cond_finish_kernel are those of kern_cond.h.
// Part of libsaigehip.so (single translation unit: saigehip.hip).
#pragma once

// Chunks of 256 samples per sample slab: cut by N alone, as COND_SLAB_CH.  A resident block holds few rows where they
// are long (312 float64 rows of N = 430 000 in a GiB: two row groups), so the slabs are short enough to fill the
// device from the sample side: 105 slabs at that N.
static const int COND_DS_SLAB_CH = 16;

// B of a conditioning set whose variants are rows of a block: cond_build_kernel with g_c(i) in place of the table
// lookup.  One thread per (sample, column); grid.x covers N * PB.
template <typename T>
__global__ void __launch_bounds__(256)
cond_build_ds_kernel(const T *__restrict__ rows, const int *__restrict__ var_idx, const uint8_t *__restrict__ flip,
	const double *__restrict__ mean, int n_cond, const double *__restrict__ F, int P, int N, int PB, double *__restrict__ B)
{
	const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (t >= (size_t)N * PB) return;
	const size_t i = t / PB;
	const int p = (int)(t - i * PB), nd = P - 1;    // nd = 2K+1 dense columns
	double x = 0;
	if (p < nd) x = F[i * P + p];
	else if (p < nd + n_cond) {
		const int c = p - nd;
		x = F[i * P + P - 1] * skat_ds_value(rows[(size_t)var_idx[c] * (size_t)N + i], flip[c] != 0, mean[c]);
	}
	B[t] = x;
}

// One iteration: the 4 SPL samples from `base`, of which lane (v, h) owns base + SPL h + j, j < SPL, of row v of each
// of its tiles.  TAIL: the iteration reaches beyond N (the same for every lane); then every sample is masked by its
// index (skat_ds_load takes only the runs that lie inside the row wide).
template <typename T, int NCT, bool TAIL>
__device__ __forceinline__ void cond_ds_iter(const T *(&rp)[COND_RT], const bool (&fl)[COND_RT], const double (&mn)[COND_RT],
	int s0, int N, const double *__restrict__ F, int P, const double *__restrict__ B, int v,
	skat_d4 (&acc)[COND_RT][NCT], double (&wj)[COND_RT])
{
	constexpr int SPL = skat_ds_run<T>::value, PB = 16 * NCT;
	T x[COND_RT][SPL];
#pragma unroll
	for (int rt = 0; rt < COND_RT; rt++) skat_ds_load<T, SPL>(rp[rt], s0, N, x[rt]);
#pragma unroll
	for (int j = 0; j < SPL; j++) {
		const int smp = s0 + j;
		const bool ok = !TAIL || smp < N;
		double m2 = 0, b[NCT];
#pragma unroll
		for (int ct = 0; ct < NCT; ct++) b[ct] = 0;
		if (ok) {
			m2 = F[(size_t)smp * P + P - 1];
			const double *bp = B + (size_t)smp * PB + v;
#pragma unroll
			for (int ct = 0; ct < NCT; ct++) b[ct] = bp[16 * ct];
		}
#pragma unroll
		for (int rt = 0; rt < COND_RT; rt++) {
			const double a = ok ? skat_ds_value(x[rt][j], fl[rt], mn[rt]) : 0.0;
			wj[rt] = fma(m2 * a, a, wj[rt]);
#pragma unroll
			for (int ct = 0; ct < NCT; ct++) acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[ct], acc[rt][ct], 0, 0, 0);
		}
	}
}

// grid = (row groups of COND_WG_ROWS, sample slabs of slab_ch chunks of 256 samples), block = 4 waves; wave w owns the
// COND_RT row tiles from row 64 w of the group on, as in cond_rect_kernel.  Lane map of v_mfma_f64_16x16x4_f64
// (A[row v][k = h], B[k = h][col v], D[row h + 4 reg][col v]; v = lane & 15, h = lane >> 4) on skat_gram_ds_kernel's
// sample runs: an iteration covers 4 SPL samples from `base`, lane (v, h) owns base + SPL h + j of row v of each of
// its tiles -- the four k lanes of a row read one contiguous 64 (u8) or 128 (f64) bytes -- and in MFMA step j its k = h
// is sample base + SPL h + j for the row operand, the B operand and the mu2 read alike.  The B fragment of a step is
// fetched once and feeds the wave's COND_RT row tiles; the four waves of the group read the same lines.  Samples >= N
// give A = B = mu2 = 0 by their index, never by what was read; no byte beyond a row is read, so none beyond the
// block's last row.  Rows >= M read row M - 1 and store nothing.  The slab's sums go to part[slab][row][PB + 1]
// (W_jj last) by plain stores: what a row gets depends on its own values, its flip / mean and N alone.
template <typename T, int NCT>
__global__ void __launch_bounds__(256)
cond_rect_ds_kernel(const T *__restrict__ rows, int N, size_t M, const uint8_t *__restrict__ flip,
	const double *__restrict__ mean, const double *__restrict__ F, int P, const double *__restrict__ B, int slab_ch,
	double *__restrict__ part)
{
	constexpr int SPL = skat_ds_run<T>::value, WD = 16 * NCT + 1;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, v = lane & 15, hq = lane >> 4;
	const size_t row0 = (size_t)blockIdx.x * COND_WG_ROWS + (size_t)wave * (16 * COND_RT);
	const long long sb = (long long)blockIdx.y * slab_ch * 256;
	const int s_begin = (int)min((long long)N, sb), s_end = (int)min((long long)N, sb + (long long)slab_ch * 256);
	const T *rp[COND_RT];
	bool fl[COND_RT];
	double mn[COND_RT], wj[COND_RT];
	skat_d4 acc[COND_RT][NCT];
#pragma unroll
	for (int rt = 0; rt < COND_RT; rt++) {
		const size_t r = min(row0 + 16 * rt + v, M - 1);
		rp[rt] = rows + r * (size_t)N;
		fl[rt] = flip[r] != 0;
		mn[rt] = mean[r];
		wj[rt] = 0;
#pragma unroll
		for (int ct = 0; ct < NCT; ct++) acc[rt][ct] = skat_d4{0, 0, 0, 0};
	}
	int base = s_begin;
	for (; base + 4 * SPL <= s_end; base += 4 * SPL)       // (s_end <= N: every run of these lies inside the row)
		cond_ds_iter<T, NCT, false>(rp, fl, mn, base + SPL * hq, N, F, P, B, v, acc, wj);
	if (base < s_end)                                       // the row's tail: only in the last slab
		cond_ds_iter<T, NCT, true>(rp, fl, mn, base + SPL * hq, N, F, P, B, v, acc, wj);
	double *o = part + (size_t)blockIdx.y * M * WD;
#pragma unroll
	for (int rt = 0; rt < COND_RT; rt++) {
#pragma unroll
		for (int r = 0; r < 4; r++) {
			const size_t row = row0 + 16 * rt + hq + 4 * r;
			if (row < M) {
#pragma unroll
				for (int ct = 0; ct < NCT; ct++) o[row * WD + 16 * ct + v] = acc[rt][ct][r];
			}
		}
		// W_jj: the four k-lanes of row v, added in the order of h
		const double x0 = __shfl(wj[rt], v), x1 = __shfl(wj[rt], v + 16), x2 = __shfl(wj[rt], v + 32), x3 = __shfl(wj[rt], v + 48);
		const size_t row = row0 + 16 * rt + v;
		if (hq == 0 && row < M) o[row * WD + WD - 1] = ((x0 + x1) + x2) + x3;
	}
}
