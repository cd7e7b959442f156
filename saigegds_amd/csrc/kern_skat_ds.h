// kern_skat_ds.h -- the sums of the SKAT set test from the dosage rows of a resident sgx_dsblock
// (row-major, stride N elements; uint8_t rows, or double rows for f64 and i32 blocks): what kern_skat.h makes from
// 2-bit rows, with the value of entry e at sample i
//     g_e(i) = present(x) ? (flip[e] ? 2 - x : x) : mean[e],      x = rows[var_idx[e]][i]
// (u8: 0xFF is missing; double: a non-finite value is missing; mean[e] arrives flipped).  Per unit the weighted Gram
// matrix W[e,f] = sum_i mu2_i g_e(i) g_f(i) and per entry the 2K+1 dense sums against the columns of F, in FP64 on the
// matrix cores.  Tiles (SkatTile), the per-slab partial tiles and skat_reduce_kernel are those of kern_skat.h.
// Part of libsaigehip.so (single translation unit: saigehip.hip).
#pragma once

// Samples a lane owns per iteration: a run of consecutive samples that is one 16-byte (u8) or 32-byte (f64) piece of
// the row, so that the four k lanes of a row read one contiguous 64 / 128 bytes.
template <typename T> struct skat_ds_run { static constexpr int value = sizeof(T) == 1 ? 16 : 4; };

// SPL consecutive elements of a row from sample s0 on.  A resident row is aligned to its element only (N odd: u8 rows
// start at odd addresses, f64 rows on 8 but not 16 bytes), so the wide form is a memcpy from a T pointer, which claims
// no more than T's alignment.  It is taken only where the whole run lies inside the row: no byte beyond the row is
// touched.  The row's tail is read element by element, each guarded by its sample index.
template <typename T, int SPL>
__device__ __forceinline__ void skat_ds_load(const T *__restrict__ row, int s0, int N, T (&x)[SPL])
{
	if (s0 + SPL <= N) {
		__builtin_memcpy(x, row + s0, SPL * sizeof(T));
	} else {
#pragma unroll
		for (int j = 0; j < SPL; j++) x[j] = (s0 + j < N) ? row[s0 + j] : T(0);
	}
}

__device__ __forceinline__ double skat_ds_value(uint8_t x, bool fl, double mean)
{
	return x == 0xFF ? mean : (double)(fl ? 2 - (int)x : (int)x);
}
__device__ __forceinline__ double skat_ds_value(double x, bool fl, double mean)
{
	return !isfinite(x) ? mean : (fl ? __dsub_rn(2.0, x) : x);
}

// grid = (tiles, sample slabs of `slab` samples, a multiple of 4 SPL), block = one wave.  Lane map of
// v_mfma_f64_16x16x4_f64 as in kern_skat.h: lane (v = lane & 15, h = lane >> 4) gives A[row v][k = h] and
// B[k = h][col v] and holds D[row h + 4 reg][col v].  An iteration covers 4 SPL samples from `base`: lane (v, h) owns
// the samples base + SPL h + j, j = 0..SPL-1, of row entry v and of column entry v; in MFMA step j its k = h is sample
// base + SPL h + j -- for both operands, and for the mu2 and F reads.  A diagonal tile (column tile = row tile) and a
// dense tile load the row entry's samples only.  Samples >= N give A = B = 0: the mask is the sample index, never what
// was read.  The slab's tile goes to part[slab][tile][256] by plain stores: no atomics, and what a tile gets depends
// on its own entries and on N only (the slabs are cut by N), not on the other tiles of the launch.
template <typename T>
__global__ void __launch_bounds__(64)
skat_gram_ds_kernel(const T *__restrict__ rows, int N, const int *__restrict__ var_idx,
	const uint8_t *__restrict__ flip, const double *__restrict__ mean, const double *__restrict__ F, int P,
	const SkatTile *__restrict__ tiles, size_t n_tiles, int slab, double *__restrict__ part)
{
	constexpr int SPL = skat_ds_run<T>::value;
	const SkatTile t = tiles[blockIdx.x];
	const int lane = threadIdx.x, v = lane & 15, hq = lane >> 4;
	const int s_begin = blockIdx.y * slab, s_end = min(N, s_begin + slab);
	const bool row_ok = v < t.nrow, col_ok = v < t.ncol;
	const bool two = !t.dense && t.col_e0 != t.row_e0;       // an off-diagonal Gram tile: the only one with other column rows
	const long long er = t.row_e0 + min(v, t.nrow - 1);
	const long long ec = t.dense ? er : t.col_e0 + min(v, t.ncol - 1);
	const T *rrow = rows + (size_t)var_idx[er] * (size_t)N;
	const T *crow = rows + (size_t)var_idx[ec] * (size_t)N;
	const bool rfl = flip[er] != 0, cfl = flip[ec] != 0;
	const double rmean = mean[er], cmean = mean[ec];
	const int fcol = (int)t.col_e0 + v;               // dense: this lane's column of F
	skat_d4 acc = {0, 0, 0, 0};
	for (int base = s_begin; base < s_end; base += 4 * SPL) {
		const int s0 = base + SPL * hq;
		T xr[SPL], xc[SPL] = {};
		skat_ds_load<T, SPL>(rrow, s0, N, xr);
		if (two) skat_ds_load<T, SPL>(crow, s0, N, xc);
#pragma unroll
		for (int j = 0; j < SPL; j++) {
			const int smp = s0 + j;
			double a = 0, b = 0;
			if (smp < N) {
				const double *f = F + (size_t)smp * P;
				const double gr = skat_ds_value(xr[j], rfl, rmean);
				a = row_ok ? gr : 0.0;
				if (t.dense) b = col_ok ? f[fcol] : 0.0;
				else {
					a *= f[P - 1];
					if (col_ok) b = two ? skat_ds_value(xc[j], cfl, cmean) : gr;
				}
			}
			acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
		}
	}
	double *o = part + ((size_t)blockIdx.y * n_tiles + blockIdx.x) * 256;
#pragma unroll
	for (int r = 0; r < 4; r++) o[(hq + 4 * r) * 16 + v] = acc[r];
}
