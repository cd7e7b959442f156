// kern_kmat_ds.h -- the columns adj_e of kern_skat_kmat.h from the dosage rows of a resident sgx_dsblock:
// row-major, stride N elements; uint8_t rows, or double rows for f64 and i32 blocks.  The value of entry e at sample i
// is the one of kern_skat_ds.h,
//     G_e(i) = present(x) ? (flip[e] ? 2 - x : x) : mean[e],      x = rows[var_idx[e]][i]
// (skat_ds_value; mean[e] arrives flipped), with one addition: flip[e] & 2 marks an entry whose column is zeros (the
// host sets it where mean[e] is not finite, as a 2-bit entry with a non-finite table gets a table of zeros).
// The K + 1 sums of an entry are made in ONE pass over its row, each in the order of skk_colsum_kernel, so that a row of
// hard calls gives the bits its 2-bit form gives; skk_colfin_kernel adds the slabs.  Everything behind the columns
// (solves, products, the host's last step) is that of the 2-bit entries.
// Part of libsaigehip.so (single translation unit: saigehip.hip).
#pragma once

#define SKK_DS_ZERO 2         /* bit of flip[e]: the entry's column is zeros */

// The 16 samples of group d (samples 16 d .. 16 d + 15) of a row: one 16-byte piece of a u8 row, four 32-byte pieces
// of a double row, by skat_ds_load -- wide only where the whole run lies inside the row, else element by element under
// the sample index.  No byte beyond the row is touched.
__device__ __forceinline__ void skk_ds_group(const uint8_t *__restrict__ row, int d, int N, uint8_t (&x)[16])
{
	skat_ds_load<uint8_t, 16>(row, 16 * d, N, x);
}
__device__ __forceinline__ void skk_ds_group(const double *__restrict__ row, int d, int N, double (&x)[16])
{
#pragma unroll
	for (int q = 0; q < 4; q++) {
		double y[4];
		skat_ds_load<double, 4>(row, 16 * d + 4 * q, N, y);
#pragma unroll
		for (int j = 0; j < 4; j++) x[4 * q + j] = y[j];
	}
}

// The K + 1 sums of entry e over one slab of samples, c'_k = sum_i G_e(i) F[i,k] (k < K) and s = sum_i G_e(i) F[i,2K],
// from one pass over the row.  grid = (slabs of SKK_CSLAB_DW groups, entries), block = 256; NS >= K + 1 is the number
// of accumulators a thread holds (the sums beyond K + 1 stay 0 and are not stored).  Per sum the order is that of
// skk_colsum_kernel: thread t takes the groups d0 + t, d0 + t + 256, ... in ascending order, adds a group's 16 samples
// in ascending order with one fma each, then the block's fixed tree (block_sum gives every sum what block_sum<1, 256>
// gives it alone).  part[entry][slab][K + 1] by plain stores: no atomics.
template <typename T, int NS>
__global__ void __launch_bounds__(256)
skk_colsum_ds_kernel(const T *__restrict__ rows, int N, const int *__restrict__ var_idx, const uint8_t *__restrict__ flip,
	const double *__restrict__ mean, const double *__restrict__ F, int P, int K, double *__restrict__ part)
{
	__shared__ double sh[NS * 4];
	const size_t e = blockIdx.y;
	const int ndw = (N + 15) >> 4;
	const int d0 = blockIdx.x * SKK_CSLAB_DW, d1 = min(ndw, d0 + SKK_CSLAB_DW);
	const T *row = rows + (size_t)var_idx[e] * (size_t)N;
	const uint8_t fb = flip[e];
	const bool fl = (fb & 1) != 0, zero = (fb & SKK_DS_ZERO) != 0;
	const double mn = mean[e];
	double s[NS];
#pragma unroll
	for (int c = 0; c < NS; c++) s[c] = 0;
	for (int d = d0 + (int)threadIdx.x; d < d1; d += 256) {
		T x[16];
		skk_ds_group(row, d, N, x);
#pragma unroll
		for (int p = 0; p < 16; p++) {
			const int i = 16 * d + p;
			if (i < N) {
				const double g = zero ? 0.0 : skat_ds_value(x[p], fl, mn);
				const double *f = F + (size_t)i * P;
#pragma unroll
				for (int c = 0; c < NS; c++)
					if (c <= K) s[c] = fma(g, f[c < K ? c : 2 * K], s[c]);
			}
		}
	}
	block_sum<NS, 256>(s, sh);
	if (threadIdx.x == 0) {
		double *o = part + (e * gridDim.x + blockIdx.x) * (size_t)(K + 1);
#pragma unroll
		for (int c = 0; c < NS; c++)
			if (c <= K) o[c] = s[c];
	}
}

// A[e][i] = G_e(i) - sum_k X[i,k] c'_ek (k ascending by fma, as skk_adj_kernel), and 0 for N <= i < lda.
// grid = (lda / 256 up, entries).
template <typename T>
__global__ void __launch_bounds__(256)
skk_adj_ds_kernel(const T *__restrict__ rows, int N, const int *__restrict__ var_idx, const uint8_t *__restrict__ flip,
	const double *__restrict__ mean, const double *__restrict__ X, int K, const double *__restrict__ cs,
	double *__restrict__ A, size_t lda)
{
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, e = blockIdx.y;
	if (i >= lda) return;
	double a = 0;
	if (i < (size_t)N) {
		const T *row = rows + (size_t)var_idx[e] * (size_t)N;
		const uint8_t fb = flip[e];
		const double *c = cs + e * (size_t)(K + 1);
		double t = 0;
		for (int k = 0; k < K; k++) t = fma(X[i * K + k], c[k], t);
		a = ((fb & SKK_DS_ZERO) ? 0.0 : skat_ds_value(row[i], (fb & 1) != 0, mean[e])) - t;
	}
	A[e * lda + i] = a;
}
