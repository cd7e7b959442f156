// kern_firth_ds.h -- Firth bias-reduced effect size of the dosage rows of a resident sgx_dsblock
// (row-major, stride N elements; uint8_t rows, or double rows for f64 and i32 blocks): what kern_firth.h makes from a
// 2-bit row and its four-entry table, with the dosage of request r at sample i the one of sgx_ds_block_skat,
//     g_r(i) = skat_ds_value(x, flip[r], mean[r]),      x = rows[var_idx[r]][i]
// (u8: 0xFF is missing; double: a non-finite value is missing; mean[r] arrives flipped).  A request whose mean is not
// finite gets {NaN, NaN, 0, 0}, whether or not a sample of its row is missing (the 2-bit kernel's rule for a non-finite
// table).  One workgroup of FIRTH_BLOCK threads per request; workgroups loop over the requests beyond the grid.
//   A. the row is read once, FIRTH_DS_RUNS wide pieces a thread (skat_ds_load: 16 bytes of a u8 row, 32 of a double
//      row, claiming the element's alignment only -- a u8 row starts at any byte, a double row on 8 --, the row's tail
//      element by element, nothing read beyond the row); the samples with g != 0 are compacted in ascending sample
//      order into a private list of (mu, x, y) -- the row's own element x, from which g is formed again where it is
//      used: 10 bytes an entry for u8 rows, 17 for double rows.  The first FIRTH_DS_LDS_N = 2048 entries live in LDS
//      (34 KiB of lists for double rows, 20 KiB for u8 rows; with the sums' 144 bytes a workgroup stays under the
//      36 KiB of firth_kernel: four workgroups a CU), the rest -- an imputed row lists nearly every sample -- in the
//      workgroup's slice of a scratch buffer.
//   B. firth_root of kern_firth.h, unchanged: the four sums of an iteration from one pass over the list, every thread
//      its entries k = tid, tid + FIRTH_BLOCK, ... in order, then block_sum's fixed tree -- no atomics.  g takes any
//      value, so an entry costs one exp, e = exp(-|b g|), and one reciprocal (firth_entry of kern_firth.h).
// A request's four outputs depend on its row's values, its flip and mean, and the model only: not on the row's place in
// the block, the request's place in var_idx, the grid or the other requests.  A row of hard calls gives the bits of
// firth_kernel on its 2-bit form with the table {0, 1, 2, mean} ({2, 1, 0, mean} where flipped): the same list in the
// same order through the same functions.
// Part of libsaigehip.so (single translation unit: saigehip.hip).
#pragma once

#define FIRTH_DS_LDS_N 2048       /* list entries held in LDS */
#define FIRTH_DS_RUNS 4           /* pieces of skat_ds_run<T> samples a thread reads per round */

// entries of a workgroup's scratch slice for rows of N samples (those beyond the LDS part), a multiple of 64
__host__ __device__ __forceinline__ size_t firth_ds_slice_entries(int N)
{
	return N > FIRTH_DS_LDS_N ? (((size_t)(N - FIRTH_DS_LDS_N) + 63) & ~(size_t)63) : 0;
}
// ... and its bytes: the means first, then the row elements, then the traits (each part stays 8-byte aligned)
template <typename T>
__host__ __device__ __forceinline__ size_t firth_ds_slice_bytes(int N) { return firth_ds_slice_entries(N) * (sizeof(double) + sizeof(T) + 1); }

template <typename T>
struct FirthDsList {
	const double *mu_l; const T *x_l; const uint8_t *y_l;       // LDS part: entries [0, FIRTH_DS_LDS_N)
	const double *mu_g; const T *x_g; const uint8_t *y_g;       // scratch part: entry k at k - FIRTH_DS_LDS_N
	int nnz;
};

// I, A, B and sum g (y - p) at b over the list
template <typename T>
__device__ __forceinline__ void firth_ds_sums(double b, bool fl, double mean, const FirthDsList<T> &L, double *sh, double (&s)[4])
{
	s[0] = s[1] = s[2] = s[3] = 0;
	for (int k = threadIdx.x; k < L.nnz; k += FIRTH_BLOCK) {
		const bool in_lds = k < FIRTH_DS_LDS_N;
		const double m = in_lds ? L.mu_l[k] : L.mu_g[k - FIRTH_DS_LDS_N];
		const T x = in_lds ? L.x_l[k] : L.x_g[k - FIRTH_DS_LDS_N];
		const uint8_t yi = in_lds ? L.y_l[k] : L.y_g[k - FIRTH_DS_LDS_N];
		const double gi = skat_ds_value(x, fl, mean), t = b * gi;
		firth_entry(m, gi, yi != 0, exp(-fabs(t)), t > 0, s);
	}
	block_sum<4, FIRTH_BLOCK>(s, sh);
}

template <typename T>
__global__ void __launch_bounds__(FIRTH_BLOCK)
firth_ds_kernel(const T *__restrict__ rows, int N, size_t n_req, const int *__restrict__ var_idx,
	const uint8_t *__restrict__ flip, const double *__restrict__ mean, const double *__restrict__ mu,
	const double *__restrict__ y, int maxit, uint8_t *scratch, double *__restrict__ out4)
{
	constexpr int NW = FIRTH_BLOCK / WAVE, SPL = skat_ds_run<T>::value, SPT = SPL * FIRTH_DS_RUNS;   // samples a thread, a round
	__shared__ double mu_l[FIRTH_DS_LDS_N];
	__shared__ T x_l[FIRTH_DS_LDS_N];
	__shared__ uint8_t y_l[FIRTH_DS_LDS_N];
	__shared__ double sh[4 * NW];
	__shared__ int shc[NW];
	const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;
	const size_t slice = firth_ds_slice_entries(N);
	double *mu_g = reinterpret_cast<double *>(scratch + (size_t)blockIdx.x * firth_ds_slice_bytes<T>(N));
	T *x_g = reinterpret_cast<T *>(mu_g + slice);
	uint8_t *y_g = reinterpret_cast<uint8_t *>(x_g + slice);

	for (size_t r = blockIdx.x; r < n_req; r += gridDim.x) {
		const bool fl = flip[r] != 0;
		const double mn = mean[r];
		double *o = out4 + r * 4;
		if (!isfinite(mn)) {                  // (uniform: every thread read the same mean)
			if (tid == 0) { o[0] = NAN; o[1] = NAN; o[2] = 0; o[3] = 0; }
			continue;
		}

		// ---- A: compaction, SPT consecutive samples a thread and FIRTH_BLOCK threads a round
		const T *row = rows + (size_t)var_idx[r] * (size_t)N;
		int nnz = 0;
		__syncthreads();                      // the previous request's readers of the list are done
		for (int base = 0; base < N; base += FIRTH_BLOCK * SPT) {
			const int s0 = base + tid * SPT;
			T x[FIRTH_DS_RUNS][SPL];
#pragma unroll
			for (int u = 0; u < FIRTH_DS_RUNS; u++) skat_ds_load<T, SPL>(row, s0 + u * SPL, N, x[u]);
			uint64_t nz = 0;                  // bit u SPL + j: sample s0 + u SPL + j is in the row and has g != 0
#pragma unroll
			for (int u = 0; u < FIRTH_DS_RUNS; u++)
#pragma unroll
				for (int j = 0; j < SPL; j++)
					if (s0 + u * SPL + j < N && skat_ds_value(x[u][j], fl, mn) != 0) nz |= (uint64_t)1 << (u * SPL + j);
			const int cnt = __popcll(nz);
			const int incl = wave_scan_incl_i(cnt);
			if (lane == WAVE - 1) shc[wid] = incl;
			__syncthreads();
			int pos = nnz + incl - cnt, total = 0;
#pragma unroll
			for (int w = 0; w < NW; w++) { if (w < wid) pos += shc[w]; total += shc[w]; }
#pragma unroll
			for (int u = 0; u < FIRTH_DS_RUNS; u++)
#pragma unroll
				for (int j = 0; j < SPL; j++)
					if ((nz >> (u * SPL + j)) & 1) {      // (the bit is set for samples below N only)
						const int i = s0 + u * SPL + j;
						const uint8_t yi = y[i] != 0 ? 1 : 0;
						if (pos < FIRTH_DS_LDS_N) { mu_l[pos] = mu[i]; x_l[pos] = x[u][j]; y_l[pos] = yi; }
						else { mu_g[pos - FIRTH_DS_LDS_N] = mu[i]; x_g[pos - FIRTH_DS_LDS_N] = x[u][j]; y_g[pos - FIRTH_DS_LDS_N] = yi; }
						pos++;
					}
			nnz += total;
			__syncthreads();                  // shc is free for the next round; the last one publishes the list
		}
		__threadfence_block();

		// ---- B: the root of U*
		const FirthDsList<T> L = {mu_l, x_l, y_l, mu_g, x_g, y_g, nnz};
		firth_root(nnz, maxit, [&](double b, double (&s)[4]) { firth_ds_sums<T>(b, fl, mn, L, sh, s); }, o);
	}
}
