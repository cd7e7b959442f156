// kern_tsblock.h -- tall-skinny FP64 block kernels of the GRM's principal components (host_pca.h).
// Part of libsaigehip.so (single translation unit: saigehip.hip).
#pragma once

// A block is stored as the operator stores right-hand sides: column c at base + c * ld, ld >= N rows,
// 1 <= L <= GRM_MAX_RHS columns.  Rows N .. ld - 1 of a column are never read.

#define TS_SLAB 1024          /* SGX_TS_SLAB: rows per partial of ts_gram (a constant: the summation order hangs on it) */
#define TS_CH 32              /* rows staged in LDS per step                                            */
#define TS_LDS (TS_CH + 2)    /* LDS column stride in doubles: the 16 columns of a fragment READ 16 distinct 16-byte
                                 slots; the staging writes (a wave covers two columns, 68 dwords apart) are not spread by it */
#define TS_AC 16              /* output columns per workgroup of ts_apply                               */
static_assert(TS_SLAB % TS_CH == 0 && TS_CH % 16 == 0, "a slab is whole staging steps, a step whole MFMA groups");
static_assert(GRM_MAX_RHS == 64, "ts_gram_kernel gives a workgroup's 4 waves 4 tiles each: 16 tiles of 16 x 16");

typedef double ts_d4 __attribute__((ext_vector_type(4)));
typedef double ts_d2 __attribute__((ext_vector_type(2)));

// 16 * ntile columns of TS_CH rows from row c0 -> s[col][TS_LDS]; rows >= s1 and columns >= L as exact zeros (not read)
__device__ __forceinline__ void ts_stage(double *__restrict__ s, const double *__restrict__ X, size_t ld, int L, int ntile,
	int c0, int s1)
{
	for (int idx = threadIdx.x; idx < 16 * ntile * TS_CH; idx += 256) {
		const int col = idx / TS_CH, r = idx % TS_CH;
		s[col * TS_LDS + r] = (col < L && c0 + r < s1) ? X[(size_t)col * ld + c0 + r] : 0.0;
	}
}

// ---- C[a][b] = sum_i A[i, a] B[i, b], the partial of one slab.  grid = slabs of TS_SLAB rows, block = 4 waves.
// The slab goes through LDS TS_CH rows at a time, each element of A and of B read from memory once (B not at all
// when it is A); wave w owns the 16 x 16 tiles w, w + 4, .. of the (ceil(La / 16), ceil(Lb / 16)) grid.
// v_mfma_f64_16x16x4_f64 with the lane map of skat_gram_kernel: lane (v = lane & 15, h = lane >> 4) gives A[row v][k = h]
// and B[k = h][col v] and holds D[row h + 4 reg][col v]; of 16 rows s .. s + 15 step t = 0..3 takes k = h as row
// s + 4 h + t.  A tile's accumulator starts at zero and takes the slab's rows in ascending groups of 16, so what
// element (a, b) gets depends on columns a and b and on N alone: not on La, Lb, the columns' places or the others.
// The slab's sums go to part[slab][64][64] by plain stores.
__global__ void __launch_bounds__(256)
ts_gram_kernel(const double *__restrict__ A, size_t lda, int La, const double *__restrict__ B, size_t ldb, int Lb, int N,
	double *__restrict__ part)
{
	__shared__ __attribute__((aligned(16))) double sa[GRM_MAX_RHS * TS_LDS], sb[GRM_MAX_RHS * TS_LDS];
	const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE, v = lane & 15, h = lane >> 4;
	const int nta = (La + 15) / 16, ntb = (Lb + 15) / 16, ntile = nta * ntb;
	const bool same = A == B && lda == ldb && La == Lb;
	const double *sB = same ? sa : sb;
	const int s0 = blockIdx.x * TS_SLAB, s1 = min(N, s0 + TS_SLAB);
	ts_d4 acc[4];
#pragma unroll
	for (int q = 0; q < 4; q++) acc[q] = ts_d4{0, 0, 0, 0};
	for (int c0 = s0; c0 < s1; c0 += TS_CH) {
		__syncthreads();                       // the last step's reads are done
		ts_stage(sa, A, lda, La, nta, c0, s1);
		if (!same) ts_stage(sb, B, ldb, Lb, ntb, c0, s1);
		__syncthreads();
#pragma unroll
		for (int q = 0; q < 4; q++) {
			const int t = wid + 4 * q;         // (the same for a whole wave)
			if (t >= ntile) continue;
			const double *pa = sa + (16 * (t / ntb) + v) * TS_LDS + 4 * h;
			const double *pb = sB + (16 * (t % ntb) + v) * TS_LDS + 4 * h;
#pragma unroll
			for (int g = 0; g < TS_CH; g += 16) {
				const ts_d2 a0 = *reinterpret_cast<const ts_d2 *>(pa + g), a1 = *reinterpret_cast<const ts_d2 *>(pa + g + 2);
				const ts_d2 b0 = *reinterpret_cast<const ts_d2 *>(pb + g), b1 = *reinterpret_cast<const ts_d2 *>(pb + g + 2);
				acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[0], b0[0], acc[q], 0, 0, 0);
				acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[1], b0[1], acc[q], 0, 0, 0);
				acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[0], b1[0], acc[q], 0, 0, 0);
				acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[1], b1[1], acc[q], 0, 0, 0);
			}
		}
	}
	double *o = part + (size_t)blockIdx.x * (GRM_MAX_RHS * GRM_MAX_RHS);
#pragma unroll
	for (int q = 0; q < 4; q++) {
		const int t = wid + 4 * q;
		if (t >= ntile) continue;
		const int b = 16 * (t % ntb) + v;
#pragma unroll
		for (int r = 0; r < 4; r++) {
			const int a = 16 * (t / ntb) + h + 4 * r;
			if (a < La && b < Lb) o[a * GRM_MAX_RHS + b] = acc[q][r];
		}
	}
}

// C[a][b] = the slabs' partials added in ascending slab order.  One thread per element.
__global__ void __launch_bounds__(256)
ts_gram_reduce_kernel(const double *__restrict__ part, int nslab, int La, int Lb, double *__restrict__ Cout)
{
	const int idx = blockIdx.x * blockDim.x + threadIdx.x;
	if (idx >= La * Lb) return;
	const int a = idx / Lb, b = idx % Lb;
	double s = 0;
	for (int k = 0; k < nslab; k++) s += part[(size_t)k * (GRM_MAX_RHS * GRM_MAX_RHS) + a * GRM_MAX_RHS + b];
	Cout[idx] = s;
}

// ---- Out[:, c] = sum_a A[:, a] T[a][c]: T ([La][Lc], row-major) in LDS, one thread per row, one fused multiply-add
// chain per output element from zero in ascending a.  grid = (rows / 256, groups of TS_AC output columns).  Element
// (i, c) depends on row i of A and column c of T only.  Out may not overlap A.
__global__ void __launch_bounds__(256)
ts_apply_kernel(const double *__restrict__ A, size_t lda, int La, const double *__restrict__ T, int Lc, int N,
	double *__restrict__ Out, size_t ldo)
{
	__shared__ double st[GRM_MAX_RHS * TS_AC];
	const int c0 = blockIdx.y * TS_AC, nc = min(TS_AC, Lc - c0);
	for (int idx = threadIdx.x; idx < La * TS_AC; idx += 256) {
		const int a = idx / TS_AC, j = idx % TS_AC;
		st[idx] = j < nc ? T[a * Lc + c0 + j] : 0.0;
	}
	__syncthreads();
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= N) return;
	double acc[TS_AC];
#pragma unroll
	for (int j = 0; j < TS_AC; j++) acc[j] = 0;
	for (int a = 0; a < La; a++) {
		const double x = A[(size_t)a * lda + i];
#pragma unroll
		for (int j = 0; j < TS_AC; j++) acc[j] = fma(x, st[a * TS_AC + j], acc[j]);
	}
#pragma unroll
	for (int j = 0; j < TS_AC; j++)
		if (j < nc) Out[(size_t)(c0 + j) * ldo + i] = acc[j];
}

// ---- R[:, c] = Y[:, c] - theta_c U[:, c], one fused multiply-add per element.  grid = (rows / 256, columns)
__global__ void __launch_bounds__(256)
ts_axpy_cols_kernel(const double *__restrict__ Y, size_t ldy, const double *__restrict__ U, size_t ldu, GrmScal theta, int N,
	double *__restrict__ R, size_t ldr)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y;
	if (i >= N) return;
	R[(size_t)c * ldr + i] = fma(-theta.v[c], U[(size_t)c * ldu + i], Y[(size_t)c * ldy + i]);
}
