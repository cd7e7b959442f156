// kern_skat_kmat.h -- SKAT on an explicit GRM: the covariance of a unit's score statistics under the
// fitted model itself, Phi^K = A' P A.  Three steps have kernels here: the columns adj_e of a unit as a dense FP64
// matrix [m][lda] from its 2-bit rows, the covariate columns of X in the same layout, and the tall-skinny products
// A' [Y | Z] and X' Z in FP64 on the matrix cores.  The solves Y = Sigma^-1 A, Z = Sigma^-1 X between them are the loop
// of host_pcg.h.  Nothing of this is in the reference.
// Part of libsaigehip.so (single translation unit: saigehip.hip).
#pragma once

#define SKK_CSLAB_DW 512      /* column sums: dwords (of 16 samples) per sample slab, cut by N alone */
#define SKK_SLAB 2048         /* contraction: samples per slab, cut by N alone (a multiple of 16)    */

// The K + 1 sums of entry e over one slab of samples: c'_k = sum_i G_i A[i,k] (columns 0..K-1 of F) and
// s = sum_i G_i (y - mu)_i (column 2K).  grid = (slabs, entries), block = 256: thread t takes the dwords d0 + t,
// d0 + t + 256 of the slab in ascending sample order, then the block's fixed tree.  part[entry][slab][K + 1].
__global__ void __launch_bounds__(256)
skk_colsum_kernel(const uint8_t *__restrict__ packed, size_t bpv, int N, const int *__restrict__ var_idx,
	const double *__restrict__ lut, const double *__restrict__ F, int P, int K, double *__restrict__ part)
{
	__shared__ double sh[4];
	const size_t e = blockIdx.y;
	const int ndw = (N + 15) >> 4;
	const int d0 = blockIdx.x * SKK_CSLAB_DW, d1 = min(ndw, d0 + SKK_CSLAB_DW);
	const uint32_t *row = reinterpret_cast<const uint32_t *>(packed + (size_t)var_idx[e] * bpv);
	const double l[4] = {lut[4 * e], lut[4 * e + 1], lut[4 * e + 2], lut[4 * e + 3]};
	for (int c = 0; c <= K; c++) {
		const int fc = c < K ? c : 2 * K;
		double s[1] = {0};
		for (int d = d0 + (int)threadIdx.x; d < d1; d += 256) {
			const uint32_t w = row[d];
			for (int p = 0; p < 16; p++) {
				const int i = 16 * d + p;
				if (i < N) s[0] = fma(sel4(l, (w >> (2 * p)) & 3u), F[(size_t)i * P + fc], s[0]);
			}
		}
		block_sum<1, 256>(s, sh);
		if (threadIdx.x == 0) part[(e * gridDim.x + blockIdx.x) * (size_t)(K + 1) + c] = s[0];
	}
}

// cs[entry][K + 1] = the slabs' sums added in slab order.  One thread per sum.
__global__ void __launch_bounds__(256)
skk_colfin_kernel(const double *__restrict__ part, size_t n_el, int nslab, int C, double *__restrict__ cs)
{
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n_el) return;
	const size_t e = i / C, c = i % C;
	double s = 0;
	for (int k = 0; k < nslab; k++) s += part[(e * nslab + k) * (size_t)C + c];
	cs[i] = s;
}

// A[e][i] = adj_ei = G_ei - sum_k X[i,k] c'_ek (k ascending), and 0 for N <= i < lda.  grid = (lda / 256 up, entries).
__global__ void __launch_bounds__(256)
skk_adj_kernel(const uint8_t *__restrict__ packed, size_t bpv, int N, const int *__restrict__ var_idx,
	const double *__restrict__ lut, const double *__restrict__ X, int K, const double *__restrict__ cs,
	double *__restrict__ A, size_t lda)
{
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, e = blockIdx.y;
	if (i >= lda) return;
	double a = 0;
	if (i < (size_t)N) {
		const uint32_t *row = reinterpret_cast<const uint32_t *>(packed + (size_t)var_idx[e] * bpv);
		const double l[4] = {lut[4 * e], lut[4 * e + 1], lut[4 * e + 2], lut[4 * e + 3]};
		const double *c = cs + e * (size_t)(K + 1);
		double t = 0;
		for (int k = 0; k < K; k++) t = fma(X[i * K + k], c[k], t);
		a = sel4(l, (row[i >> 4] >> (2 * (i & 15))) & 3u) - t;
	}
	A[e * lda + i] = a;
}

// Xc[k][i] = X[i,k], and 0 for N <= i < lda.  grid = (lda / 256 up, K).
__global__ void __launch_bounds__(256)
skk_xcols_kernel(const double *__restrict__ X, int N, int K, double *__restrict__ Xc, size_t lda)
{
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
	if (i >= lda) return;
	Xc[k * lda + i] = i < (size_t)N ? X[i * K + k] : 0.0;
}

// One 16 x 16 tile of L' R: rows = the vectors row0 .. row0 + nrow - 1 of L, columns = the vectors col0 .. of R.
struct SkkTile {
	int row0, col0;
	int nrow, ncol;     // 1..16; the others are computed as zeros and never read
};

// 16 samples of one tile's sum, the body of the slab loop of every kernel that makes a C_ef (skk_gram_kernel here,
// ckm_panel_kernel of kern_cond_kmat.h): a4 / b4 are the lane's four samples i .. i + 3 (i = s + 4 h) of its row vector
// and of its column vector, rok / cok whether the lane's row / column is inside the tile.  A tile's accumulator starts
// at zero and takes these steps for s = slab start, + 16, ... in ascending order: that order is what fixes the bits.
__device__ __forceinline__ void skk_step16(skat_d4 &acc, const skat_d4 &a4, const skat_d4 &b4, bool rok, bool cok, int i, int N)
{
#pragma unroll
	for (int q = 0; q < 4; q++) {
		const bool ok = i + q < N;
		const double a = (rok && ok) ? a4[q] : 0.0;
		const double b = (cok && ok) ? b4[q] : 0.0;
		acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
	}
}

// grid = (tiles, sample slabs of SKK_SLAB), block = one wave.  L and R hold one vector per row, ldl and ldr doubles
// apart: multiples of 4, at least N rounded up to 16, on 32-byte boundaries.  v_mfma_f64_16x16x4_f64 with the lane map
// of skat_gram_kernel: lane (v = lane & 15, h = lane >> 4) gives A[row v][k = h] and B[k = h][col v].  Which sample a k
// stands for is free as long as both operands agree: of 16 samples s .. s + 15 the lane loads the four at s + 4 h (one
// 32-byte load per operand, the wave's four h of a vector side by side) and step t = 0..3 takes k = h as sample
// s + 4 h + t.  Samples >= N and rows / columns beyond the tile enter as zeros by selection, whatever the padding
// holds; no load goes past a vector's ld.  The slab's tile goes to part[slab][tile][256] by plain stores: no atomics,
// and element (e, f) depends on the two vectors and on N only.
__global__ void __launch_bounds__(64)
skk_gram_kernel(const double *__restrict__ L, size_t ldl, const double *__restrict__ R, size_t ldr, int N,
	const SkkTile *__restrict__ tiles, size_t n_tiles, double *__restrict__ part)
{
	const SkkTile t = tiles[blockIdx.x];
	const int lane = threadIdx.x, v = lane & 15, hq = lane >> 4;
	const int n16 = (N + 15) & ~15;
	const int s0 = blockIdx.y * SKK_SLAB, s1 = min(n16, s0 + SKK_SLAB);
	const bool rok = v < t.nrow, cok = v < t.ncol;
	const double *lp = L + (size_t)(t.row0 + min(v, t.nrow - 1)) * ldl;
	const double *rp = R + (size_t)(t.col0 + min(v, t.ncol - 1)) * ldr;
	skat_d4 acc = {0, 0, 0, 0};
	for (int s = s0; s < s1; s += 16) {
		const int i = s + 4 * hq;
		const skat_d4 a4 = *reinterpret_cast<const skat_d4 *>(lp + i);
		const skat_d4 b4 = *reinterpret_cast<const skat_d4 *>(rp + i);
		skk_step16(acc, a4, b4, rok, cok, i, N);
	}
	double *o = part + ((size_t)blockIdx.y * n_tiles + blockIdx.x) * 256;
#pragma unroll
	for (int r = 0; r < 4; r++) o[(hq + 4 * r) * 16 + v] = acc[r];
}
