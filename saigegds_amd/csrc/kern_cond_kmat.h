// kern_cond_kmat.h -- the conditional scan on an explicit GRM: what a chunk of scanned rows needs of
// A' [Y | Z] against the installed set, in one pass over the chunk.  With A_C, Y_C the set's columns and solves, Z =
// Sigma^-1 X, and A, Y the chunk's, row j needs a_j' Y_C and a_j' Z (the panel), A_C' y_j and a_j' y_j: 2 C + 1 + K sums
// where skk_gram_kernel on the unit {C, j} makes (C + 1)^2 + (C + 1) K.
// Part of libsaigehip.so (single translation unit: saigehip.hip).
#pragma once

#define CKM_PIECE 128                    /* samples of the shared vectors in LDS at a time (a multiple of 16) */
#define CKM_LDP (CKM_PIECE + 4)          /* doubles between two vectors in LDS: keeps 32-byte alignment, shifts the banks */
#define CKM_MAXSH (3 * 16)               /* shared vectors: A_C and the panel [Y_C | Z], n_cond <= 16 and n_cond + K <= 32 */
#define CKM_WG_TILES 4                   /* row tiles of a workgroup: one per wave, SGX_GRM_MAX_RHS = 64 rows */

// grid = (row tiles of the chunk / CKM_WG_TILES up, sample slabs of SKK_SLAB), block = 4 waves, one 16-row tile of the
// chunk each.  S holds the set's vectors lda apart: A_C [n_cond], then the panel Y_C [n_cond] and Z [K]; A and Y the
// chunk's m columns and their solves, lda apart too (lda a multiple of 16, at least N rounded up to 16).  NPT: column
// tiles of the panel, (n_cond + K + 15) / 16.
// Per slab the workgroup brings the 2 n_cond + K shared vectors into LDS once, CKM_PIECE samples at a time (50.7 KB:
// three workgroups a CU of the 160 KB), and every wave reads them from there; its own 16 rows of A and Y come from
// memory once, 32 bytes a lane and step as in skk_gram_kernel, and feed all of its tiles:
//   tile t < NPT   rows = the wave's rows of A, columns = panel vectors 16 t ..      -> a_j' y_c, a_j' z_k
//   tile NPT       rows = A_C, columns = the wave's rows of Y                        -> a_c' y_j
//   tile NPT + 1   rows = the wave's rows of A, columns = the same rows of Y         -> the diagonal is a_j' y_j
// Every tile is a sum of skk_step16 in ascending sample order from the slab's start, so an element has the bits
// skk_gram_kernel gives the same two vectors.  Samples >= N, rows beyond m and columns beyond the panel enter as
// zeros by selection; no load goes past a vector's lda (a slab ends at N rounded up to 16).  The slab's tiles go to
// part[slab][row tile][NPT + 2][256] by plain stores: no atomics.
template <int NPT>
__global__ void __launch_bounds__(256)
ckm_panel_kernel(const double *__restrict__ S, int n_cond, int K, const double *__restrict__ A, const double *__restrict__ Y,
	size_t lda, int N, int m, double *__restrict__ part)
{
	__shared__ __attribute__((aligned(32))) double sh[CKM_MAXSH * CKM_LDP];
	constexpr int NT = NPT + 2;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, v = lane & 15, hq = lane >> 4;
	const int n16 = (N + 15) & ~15;
	const int s0 = blockIdx.y * SKK_SLAB, s1 = min(n16, s0 + SKK_SLAB);
	const int nrt = (m + 15) >> 4, rt = blockIdx.x * CKM_WG_TILES + wave;
	const bool active = rt < nrt;
	const int nsh = 2 * n_cond + K, np = n_cond + K;
	const int nrow = active ? min(16, m - 16 * rt) : 1;
	const bool rok = active && v < nrow, sok = v < n_cond;
	const size_t row = active ? (size_t)(16 * rt + min(v, nrow - 1)) : 0;
	const double *ap = A + row * lda, *yp = Y + row * lda;
	const double *sc = sh + (size_t)min(v, n_cond - 1) * CKM_LDP;          // A_C, vector v
	const double *sp[NPT];
	bool pok[NPT];
#pragma unroll
	for (int t = 0; t < NPT; t++) {
		pok[t] = 16 * t + v < np;
		sp[t] = sh + (size_t)(n_cond + min(16 * t + v, np - 1)) * CKM_LDP;
	}
	skat_d4 accP[NPT], accQ = {0, 0, 0, 0}, accG = {0, 0, 0, 0};
#pragma unroll
	for (int t = 0; t < NPT; t++) accP[t] = skat_d4{0, 0, 0, 0};

	for (int p0 = s0; p0 < s1; p0 += CKM_PIECE) {
		const int p1 = min(s1, p0 + CKM_PIECE);
		__syncthreads();                                   // the piece before has been read
		for (int k = threadIdx.x; k < nsh * (CKM_PIECE / 4); k += 256) {
			const int c = k / (CKM_PIECE / 4), i = p0 + 4 * (k % (CKM_PIECE / 4));
			if (i < p1)
				*reinterpret_cast<skat_d4 *>(sh + (size_t)c * CKM_LDP + (i - p0)) = *reinterpret_cast<const skat_d4 *>(S + (size_t)c * lda + i);
		}
		__syncthreads();
		if (!active) continue;
		for (int s = p0; s < p1; s += 16) {
			const int i = s + 4 * hq, li = i - p0;
			const skat_d4 a4 = *reinterpret_cast<const skat_d4 *>(ap + i);
			const skat_d4 y4 = *reinterpret_cast<const skat_d4 *>(yp + i);
			const skat_d4 c4 = *reinterpret_cast<const skat_d4 *>(sc + li);
#pragma unroll
			for (int t = 0; t < NPT; t++) {
				const skat_d4 b4 = *reinterpret_cast<const skat_d4 *>(sp[t] + li);
				skk_step16(accP[t], a4, b4, rok, pok[t], i, N);
			}
			skk_step16(accQ, c4, y4, sok, rok, i, N);
			skk_step16(accG, a4, y4, rok, rok, i, N);
		}
	}
	if (!active) return;
	double *o = part + ((size_t)blockIdx.y * nrt + rt) * NT * 256;
#pragma unroll
	for (int r = 0; r < 4; r++) {
		const int e = (hq + 4 * r) * 16 + v;
#pragma unroll
		for (int t = 0; t < NPT; t++) o[t * 256 + e] = accP[t][r];
		o[NPT * 256 + e] = accQ[r];
		o[(NPT + 1) * 256 + e] = accG[r];
	}
}
