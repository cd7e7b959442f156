// mf_fixed.h -- what the exact-integer contractions on the matrix cores (v_mfma_i32_16x16x64_i8) share:
// the 56-bit fixed-point limb format, the limb tile image and its sample order, the column-group
// description of the scan's epilogue, and the hi/lo integer sums the epilogues work in.
// Used by the scan (kern_score3.h, host_init.h) and by the implicit-GRM operator (kern_grm.h).
// Part of libsaigehip.so (single translation unit: saigehip.hip).
#pragma once

// Why a matrix formulation at all: with FP64 the dense score sums cost
// 2(2K+2) flop per (variant, sample) against 0.25 B of input, i.e. they are
// FP64-bound at ~11 M variants/s, and skipping zeros turns them
// into a 64 B gather per carrier.  The sums are, however, integer-weighted:
//     sum_i code_i * F[i,c],   code_i in {0,1,2,3}.
// F is converted ONCE (sgx_init; per product for the GRM operator) to 56-bit fixed point per column,
//     F[i,c] ~ q[i,c] * 2^-e_c,   q = sum_{l<7} d_l 256^l,  d_l in [-128,127],
// so that every sum is an exact int32 dot product per limb
//     S[c,l] = sum_i code_i * d_l[i,c]              (|S| <= 384 N < 2^31)
// which v_mfma_i32_16x16x64_i8 evaluates at ~16x the FP64 FMA rate, with no
// rounding anywhere: the reduction order (and the split of N across workgroups,
// merged by integer atomics) cannot change a single bit.  The quantisation
// error is 2^-55 of the column maximum per entry, below the rounding error of
// a double-precision dot product.
//
// Planes of the scan (score3_epilogue).  A = raw 2-bit codes (0,1,2,3) against all limb columns gives
//     V[c] = T1 + 2 T2 + 3 T3      (T_g = sum of q over samples with code g)
// A' = twice bit 1 of the code against the mu2 limbs gives  B2 = 2 (T2 + T3)  (mu2 only), and the sums
// over the missing samples give T3[c] and n3.  From these, in integer arithmetic,
//     W[c] = V[c] - 3 T3[c] = T1 + 2 T2,   H2 = B2 / 2 - T3[mu2] = T2[mu2],
//     AC = V[ones] - 3 n3,   Num = N - n3,
// and with imp = 2 AF the sums the epilogue needs (dev_common.h):
//     no flip:  sum G F = W + imp T3          sum G^2 mu2 = W + 2 H2 + imp^2 T3
//     flip:     sum G F = 2 Ftot - W - imp T3
//               sum G^2 mu2 = 4 (Ftot - S1 - H2 - T3) + S1 + (2-imp)^2 T3,  S1 = W - 2 H2.
// The GRM operator's two planes (codes, [code == 3]) and their algebra: kern_grm.h.

typedef int v4i __attribute__((ext_vector_type(4)));

#define MF_VPB 256           /* rows per workgroup of a contraction kernel (mf_grid's default)      */
#define MF_NLIMB 7           /* limbs of a full-precision column (56-bit fixed point)              */
#define MF_LIMB_A 5          /* limbs of the t_XVX_inv_XV columns (c'): see "Limb counts" below     */
#define MF_LIMB_E 6          /* limbs of the w X columns (e)                                        */
#define MF_MAXP (2 * SGX_MAX_COEFF + 2)   /* value columns: c' (K), e (K), s, w                     */
#define MF_MAXG 4

// what a contraction kernel needs of one column group
struct MfTab {
	const uint8_t *Fl;         // [ngrp_pad][NCOL][16] int8 limb digits, sample order mf_pos()
	int ntile;                 // number of 256-sample tiles = ngrp_pad / 16
};

// Limb counts.  s = G.(y-mu) and w = sum w_i G_i^2 carry 7 limbs (56 bits: below the rounding of a
// double-precision dot product).  The covariate projections enter the statistics only through
//     var2 = c'.XVX.c' + w - 2 e.c'      S = s - S_a.c'
// where c' = (X'VX)^-1 X'V G is O(AF) for the intercept direction and O(1/sqrt(N)) otherwise,
// XVX c' - e vanishes when the two weight vectors (no-K V, GLMM mu2) agree, and S_a = X'(y-mu) is
// ~0 at the fit.  e therefore carries 6 limbs (48 bits) and the t_XVX_inv_XV columns 5 (40 bits):
// measured effect on var2 <= 5e-14 relative and on S/sqrt(var2) <= 6e-16 (golden model and the
// N = 100 000 synthetic model, tools/limb_sim.py) -- under the rounding noise of the reference's
// own double sums, and 2000 x under the 1e-10 parity bar.  With K = 3 the value
// columns then fill exactly 3 B fragments: 3*5 + 3*6 + 7 + 7 + 1 = 48.
//
// Column groups.  A workgroup's accumulators hold up to 4 B fragments (64 limb columns); with
// more covariates the columns are cut into groups (never inside a column) and the contraction
// kernel runs once per group over the same packed rows.  Group 0 carries s, w, the constant-1
// column and the bit-1 fragment.  Accumulator row of a variant = the groups' rows one after the
// other: goff[g] ints in, group g has gncol[g] ints of value (+ bit-1) sums followed by
// 16 * nbfv[g] ints of missing-plane sums.
struct MfEpi {
	int ngroups, acc_stride;
	int goff[MF_MAXG], gncol[MF_MAXG];
	int col_ones;              // group 0: column of the constant 1
	int col_b1;                // group 0: first column of the w limbs in the bit-1 fragment
	unsigned char cgrp[MF_MAXP], ccol[MF_MAXP], climb[MF_MAXP];   // per value column: group, first limb column, limbs
	int derive_c;              // quantitative traits: c' = XVXi e instead of carried columns (climb = 0)
	double XVXi[SGX_MAX_COEFF * SGX_MAX_COEFF];
	int escale[MF_MAXP];       // F = q * 2^-escale
	long long ftot_hi[MF_MAXP];// sum_i q[i,c] = hi * 2^32 + lo
	long long ftot_lo[MF_MAXP];
};

// Sample order inside a group of 16.  One dword of the packed row holds 16 codes,
// code s in bits 2s..2s+1.  The A fragment takes them as 4 dwords of 4 bytes; with
//     val[t] = (w >> 2t) & 0x03030303      (byte j of val[t] = code of sample 4j + t)
// the unpack is two VALU operations per dword, and the B tiles simply store the 16
// samples of a group in that same order: sample s at byte mf_pos(s) = 4 (s & 3) + (s >> 2).
__host__ __device__ __forceinline__ int mf_pos(int s) { return ((s & 3) << 2) | (s >> 2); }

// value = hi * 2^32 + lo, both parts small enough to be exact in a double
struct HiLo { long long hi, lo; };
__device__ __forceinline__ double hl_to_double(HiLo x) { return (double)x.hi * 4294967296.0 + (double)x.lo; }
__device__ __forceinline__ HiLo hl(long long hi, long long lo) { HiLo x; x.hi = hi; x.lo = lo; return x; }
__device__ __forceinline__ HiLo hl_axpy(long long a, HiLo x, HiLo y) { return hl(a * x.hi + y.hi, a * x.lo + y.lo); }

// limb sums of one full-precision column (MF_NLIMB limbs) -> HiLo
__device__ __forceinline__ HiLo mf_limbs(const int *a)
{
	long long lo = 0, hi = 0;
#pragma unroll
	for (int l = 3; l >= 0; l--) lo = lo * 256 + a[l];
#pragma unroll
	for (int l = MF_NLIMB - 1; l >= 4; l--) hi = hi * 256 + a[l];
	return hl(hi, lo);
}

// Lane-map self-test of v_mfma_i32_16x16x64_i8 with asymmetric integer data:
//   A[row l&15][k = 16(l>>4)+j], B[k = 16(l>>4)+j][col l&15], D[(l>>4)*4+reg][l&15]
__global__ void mfma_selftest_kernel(const int8_t *A, const int8_t *B, int *D)
{
	const int lane = threadIdx.x, r = lane & 15, kg = lane >> 4;
	v4i a, b, c = {0, 0, 0, 0};
	for (int k = 0; k < 4; k++) {
		int av = 0, bv = 0;
		for (int j = 0; j < 4; j++) {
			av |= (int)(uint8_t)A[r * 64 + 16 * kg + 4 * k + j] << (8 * j);
			bv |= (int)(uint8_t)B[(16 * kg + 4 * k + j) * 16 + r] << (8 * j);
		}
		a[k] = av; b[k] = bv;
	}
	c = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0);
	for (int reg = 0; reg < 4; reg++) D[(kg * 4 + reg) * 16 + r] = c[reg];
}
