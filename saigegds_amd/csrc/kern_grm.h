// kern_grm.h -- implicit-GRM operator of the null-model fit on 2-bit genotypes.
// Part of libsaigehip.so (single translation unit: saigehip.hip).
#pragma once
#include <type_traits>

// Reference: src/saige_fitnull.cpp
//   saige_store_2b_geno   :159-230  standardised-genotype table, diag(GRM)
//   get_crossprod_b_grm   :435-536  out = G'(G b)/M over the packed genotypes
//   get_diag_sigma        :542-559, get_crossprod :564-576, PCG_diag_sigma :581-614
// G is the M x N matrix of standardised genotypes of the GRM markers,
//   G[v,i] = lut_v[code]:  lut_v = {-2af, 1-2af, 2-2af, 0(missing)} * inv_v,
//   inv_v = 1/sqrt(2 af (1-af))  (0 for a monomorphic marker, :195-197).
// With l0 = -2 af inv:  lut_v[code] = l0_v + code * inv_v for code 0..2, so both
// halves of the product are sums of integer codes times one real vector:
//   pass 1 (per marker, over samples):   dot_v = l0_v (sum b - T3b_v) + inv_v (V_v - 3 T3b_v)
//        V_v = sum_i code_vi b_i,  T3b_v = sum_{missing} b_i
//   pass 2 (per sample, over markers):   M out_i = C0 + X_i - Gam_i
//        x_v = dot_v inv_v,  C0 = sum_v dot_v l0_v,
//        X_i = sum_v code_vi x_v,  Gam_i = sum_{missing} (3 - 2 af_v) x_v
// Both are evaluated by grm_contract_kernel (code plane + missing plane) on the
// marker-major matrix and on its 2-bit transpose, with b / (x, gam) converted to
// 56-bit fixed-point limbs first (mf_fixed.h), so each pass is one streaming sweep
// of the packed matrix with exact integer accumulation.
//
// Every entry point works on a set of right-hand sides (columns); a single product or solve is a
// set of one.  Column c of a set lives at base + c * ld; blockIdx.y picks the column of a launch.

#define GRM_MAX_RHS 64        /* SGX_GRM_MAX_RHS                                     */
#define GRM_MAXF 3            /* value fragments of a contraction launch (4 spill: DESIGN.md)   */
#define GRM_GROUP (2 * GRM_MAXF)   /* columns per pass-1 launch: two per 16-column fragment         */
#define GRM_GROUP2 GRM_MAXF        /* columns per pass-2 launch: one per fragment (x and gam limbs) */
#define GRM_NAF 4             /* A fragments (16 rows each) per wave: 2 waves per SIMD at <= 256 registers */
#define GRM_WAVES 4           /* waves per workgroup -> MF_VPB rows                  */
static_assert(16 * GRM_NAF * GRM_WAVES == MF_VPB, "mf_grid plans workgroups of MF_VPB rows");

struct GrmCols {              // the columns of a set a launch works on (kernel argument, by value)
	int n;
	int c[GRM_MAX_RHS];
};

struct GrmScal {              // one double per column of a launch (by value)
	double v[GRM_MAX_RHS];
};

#define GRM_MAX_GROUPS 64     /* SGX_GRM_MAX_GROUPS: marker groups of a handle (leave-one-group-out columns) */

struct GrmIdx {               // one index per column of a launch (by value): excluded group (-1: none), weight row
	int v[GRM_MAX_RHS];
};

// ---- per-marker statistics: af, inv, l0  (:181-203); one workgroup per marker
__global__ void __launch_bounds__(256)
grm_marker_stats(const uint8_t *__restrict__ packed, size_t bpv, int N, size_t M,
	double *__restrict__ af_out, double *__restrict__ inv_out, double *__restrict__ l0_out)
{
	__shared__ int shi[8];
	const size_t v = blockIdx.x;
	if (v >= M) return;
	const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;
	const uint32_t *row = reinterpret_cast<const uint32_t *>(packed + v * bpv);
	const int ndw = (N + 15) >> 4;
	int nvalid = 0, sum = 0;
	for (int d = tid; d < ndw; d += 256) {
		const uint32_t w = row[d];
		const uint32_t km = keep_mask(N - d * 16);
		const uint32_t lo = w & LO_MASK & km, hi = (w >> 1) & LO_MASK & km;
		const int n3 = __popc(lo & hi), n1 = __popc(lo & ~hi), n2 = __popc(hi & ~lo);
		nvalid += min(16, N - d * 16) - n3;
		sum += n1 + 2 * n2;
	}
	nvalid = wave_sum_i(nvalid); sum = wave_sum_i(sum);
	if (lane == 0) { shi[wid] = nvalid; shi[4 + wid] = sum; }
	__syncthreads();
	if (tid == 0) {
		const int nv = shi[0] + shi[1] + shi[2] + shi[3], sm = shi[4] + shi[5] + shi[6] + shi[7];
		double af = double(sm) / (2 * nv);
		double inv = 1 / sqrt(2 * af * (1 - af));
		if (!isfinite(af) || !isfinite(inv)) af = inv = 0;
		af_out[v] = af; inv_out[v] = inv; l0_out[v] = (0 - 2 * af) * inv;
	}
}

// ---- 2-bit transpose: src [R][src_bpv] (C columns) -> dst [C][dst_bpv] (R columns)
// one workgroup per tile of 64 source rows x 256 source columns
__global__ void __launch_bounds__(256)
transpose_2bit(const uint8_t *__restrict__ src, size_t src_bpv, size_t R, int C,
	uint8_t *__restrict__ dst, size_t dst_bpv)
{
	__shared__ uint32_t tile[64][17];      // 64 rows x 16 dwords (+1 pad)
	const int tid = threadIdx.x;
	const size_t r0 = (size_t)blockIdx.y * 64;
	const int c0 = blockIdx.x * 256;        // first source column; 16 dwords per row
	for (int k = tid; k < 64 * 16; k += 256) {
		const int rr = k >> 4, d = k & 15;
		uint32_t w = 0;
		if (r0 + rr < R && (size_t)(c0 / 4 + d * 4 + 4) <= src_bpv)
			w = *reinterpret_cast<const uint32_t *>(src + (r0 + rr) * src_bpv + c0 / 4 + d * 4);
		tile[rr][d] = w;
	}
	__syncthreads();
	// output: 256 destination rows (source columns) x 64 destination columns = 4 dwords each
	for (int k = tid; k < 256 * 4; k += 256) {
		const int cc = k >> 2, q = k & 3;   // destination row c0+cc, its dword q (16 source rows)
		if (c0 + cc >= C) continue;
		uint32_t w = 0;
#pragma unroll
		for (int s = 0; s < 16; s++) {
			const uint32_t code = (tile[16 * q + s][cc >> 4] >> (2 * (cc & 15))) & 3u;
			w |= code << (2 * s);
		}
		*reinterpret_cast<uint32_t *>(dst + (size_t)(c0 + cc) * dst_bpv + r0 / 4 + q * 4) = w;
	}
}

// ---- diag(GRM)_i = (1/M) sum_v lut_v[code_vi]^2  (:205-227); one wave per sample
// on the sample-major matrix
__global__ void __launch_bounds__(256)
grm_diag_kernel(const uint8_t *__restrict__ gt, size_t bpvM, int N, size_t M,
	const double *__restrict__ inv, const double *__restrict__ l0, double *__restrict__ diag)
{
	const int lane = threadIdx.x & (WAVE - 1);
	const int i = blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
	if (i >= N) return;
	const uint32_t *row = reinterpret_cast<const uint32_t *>(gt + (size_t)i * bpvM);
	const size_t ndw = (M + 15) >> 4;
	double s = 0;
	for (size_t d = lane; d < ndw; d += WAVE) {
		const uint32_t w = row[d];
		for (int k = 0; k < 16; k++) {
			const size_t v = d * 16 + k;
			if (v >= M) break;
			const uint32_t code = (w >> (2 * k)) & 3u;
			const double g = (code == 3u) ? 0.0 : fma((double)code, inv[v], l0[v]);
			s = fma(g, g, s);
		}
	}
	s = wave_sum(s);
	if (lane == 0) diag[i] = s / (double)M;
}

// ---- diag(GRM) by marker group: S[c][i] = sum over the markers v of group c of lut_v[code_vi]^2; one wave
// (= one workgroup) per sample on the sample-major matrix, addressed as grm_diag_kernel.  A lane keeps the sum of
// its current run of one group in a register and adds it to its own LDS slot acc[c][lane] when the group
// changes; the lanes' slots are then summed by wave_sum.  The order of every sum is fixed by the group layout
// alone.  LDS: ngroups * WAVE doubles.
__global__ void __launch_bounds__(WAVE)
grm_diag_groups_kernel(const uint8_t *__restrict__ gt, size_t bpvM, int N, size_t M,
	const double *__restrict__ inv, const double *__restrict__ l0, const int *__restrict__ grp, int ngroups,
	double *__restrict__ S)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
	double *acc = reinterpret_cast<double *>(smem);      // [ngroups][WAVE]
	const int lane = threadIdx.x;
	const int i = blockIdx.x;
	if (i >= N) return;
	for (int c = 0; c < ngroups; c++) acc[c * WAVE + lane] = 0;
	const uint32_t *row = reinterpret_cast<const uint32_t *>(gt + (size_t)i * bpvM);
	const size_t ndw = (M + 15) >> 4;
	double s = 0;
	int cur = -1;
	for (size_t d = lane; d < ndw; d += WAVE) {
		const uint32_t w = row[d];
		for (int k = 0; k < 16; k++) {
			const size_t v = d * 16 + k;
			if (v >= M) break;
			const int c = grp[v];
			if (c != cur) {
				if (cur >= 0) acc[cur * WAVE + lane] += s;
				s = 0; cur = c;
			}
			const uint32_t code = (w >> (2 * k)) & 3u;
			const double g = (code == 3u) ? 0.0 : fma((double)code, inv[v], l0[v]);
			s = fma(g, g, s);
		}
	}
	if (cur >= 0) acc[cur * WAVE + lane] += s;
	for (int c = 0; c < ngroups; c++) {
		const double t = wave_sum(acc[c * WAVE + lane]);
		if (lane == 0) S[(size_t)c * N + i] = t;
	}
}

// diag_excl[c][i] = (sum over c' != c of S[c'][i], ascending c') / (M - M_c) -> D row 1 + c; row 0 is the
// diagonal of the whole GRM (excl = -1).  Every term is non-negative: nothing cancels when one group holds
// most markers.  A group that holds every marker has no complement: its row is 0 and is never used.
__global__ void __launch_bounds__(256)
grm_diag_excl_kernel(int N, int ngroups, const double *__restrict__ S, const double *__restrict__ msub,
	const double *__restrict__ diag, double *__restrict__ D)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= N) return;
	D[i] = diag[i];
	for (int c = 0; c < ngroups; c++) {
		double t = 0;
		for (int c2 = 0; c2 < ngroups; c2++)
			if (c2 != c) t += S[(size_t)c2 * N + i];
		D[(size_t)(1 + c) * N + i] = (msub[c] > 0) ? t / msub[c] : 0.0;
	}
}

// ---- the contraction: acc[row][..] += sum over samples of (code, [code == 3]) x limb columns
// grid = (row tiles of MF_VPB, sample splits: mf_grid); block = 64 * GRM_WAVES; LDS = 2 B tiles.
// packed: 2-bit rows of bpv bytes, bpv % 128 == 0 covering whole pairs of 256-sample tiles; tile
// ranges (t0, t1 - t0, tb.ntile) are even.  tb.Fl: B tiles of 16 NBFV limb columns.
// Accumulator row (acc_stride = 32 NBFV ints): [0, 16 NBFV) the code plane against every limb
// column, [16 NBFV, 32 NBFV) the same columns summed over MISSING samples only (plane [code == 3]);
// that plane is multiplied only in fragments that contain a missing code, which a wave decides with
// one ballot.  A lane fetches 2 x 16 B of each of its rows per PAIR of tiles (the two halves of one
// 128-B line, by back-to-back instructions): half as many lines in flight per byte.
template <int NBFV>
__global__ void __launch_bounds__(WAVE * GRM_WAVES, 2)   /* waves per SIMD */
grm_contract_kernel(const uint8_t *__restrict__ packed, size_t bpv, int M, MfTab tb,
	int tiles_per_split, int *__restrict__ accbuf, int acc_stride)
{
	constexpr int NAF = GRM_NAF;
	constexpr int NCOL = 16 * NBFV;
	constexpr int TILE_BYTES = 16 * NCOL * 16;
	constexpr int NDMA = (TILE_BYTES / 1024 + GRM_WAVES - 1) / GRM_WAVES;   // DMA instructions per wave and tile
	constexpr int AW = 2;                                                   // 16-B pieces of a row held per lane
	static_assert(AW * NAF + NDMA <= 4 * NAF, "more loads per tile than MFMA groups");
	extern __shared__ __attribute__((aligned(16))) uint8_t smem[];   // 2 x TILE_BYTES, nothing else
	uint8_t *ldsB = smem;

	const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;
	const int r = lane & 15, kg = lane >> 4;
	// Workgroups are handed to the 8 XCDs round-robin in dispatch order, so those with the same
	// (linear id % 8) share an L2.  Give each such group whole sample splits: its resident
	// workgroups then stream the same B tiles, which stay in that L2, while every packed row
	// is still read once.  (A placement guess only: correctness does not depend on it.)
	unsigned vt_idx = blockIdx.x, split = blockIdx.y;
	{
		const unsigned VT = gridDim.x, L = blockIdx.y * VT + blockIdx.x, full = gridDim.y & ~7u;
		if (L < full * VT) { const unsigned q = L >> 3; split = 8 * (q / VT) + (L & 7); vt_idx = q % VT; }
	}
	const int vbase = vt_idx * (16 * NAF * GRM_WAVES) + wid * 16 * NAF;
	const int t0 = split * tiles_per_split;
	const int t1 = min(tb.ntile, t0 + tiles_per_split);

	v4i acc[NAF][NBFV], accm[NAF][NBFV];
#pragma unroll
	for (int f = 0; f < NAF; f++) {
#pragma unroll
		for (int b = 0; b < NBFV; b++) acc[f][b] = (v4i){0, 0, 0, 0};
#pragma unroll
		for (int b = 0; b < NBFV; b++) accm[f][b] = (v4i){0, 0, 0, 0};
	}
	bool saw_missing = false;   // wave-uniform

	// this lane's 16 B of each of its rows in tile t: dwords 16t+4kg .. +3.  Row pointers advance by
	// 64 B per tile; bpv is a multiple of 64 that covers every tile (sgx_row_stride), rows past M
	// are clamped (their sums are never stored)
	const uint8_t *rowp[NAF];
	const uint8_t *const row0 = packed + (size_t)t0 * 64 + 16 * kg;
#pragma unroll
	for (int f = 0; f < NAF; f++)
		rowp[f] = row0 + (size_t)min(vbase + 16 * f + r, M - 1) * bpv;
	auto load_A1 = [&](uint4 &dst, int f, int piece) {
		// (measured with the streaming hint: 4.46 -> 5.04 ms per product -- a lane's 16 bytes are a quarter of a
		// 64-byte piece that four instructions share; the hint drops the line between them)
		dst = *reinterpret_cast<const uint4 *>(rowp[f] + 64 * piece);
		if (piece == AW - 1) rowp[f] += 64 * AW;
	};
	// one KiB of B tile t -> LDS buffer (t & 1) by LDS-DMA, lane-linear
	auto dma_B1 = [&](int t, int i) {
		const int k = wid + i * GRM_WAVES;
		if (k >= TILE_BYTES / 1024) return;
		const uint8_t *src = tb.Fl + (size_t)t * TILE_BYTES;
		uint8_t *dst = ldsB + (size_t)(t & 1) * TILE_BYTES;
		__builtin_amdgcn_global_load_lds(
			(const __attribute__((address_space(1))) void *)(src + (size_t)k * 1024 + lane * 16),
			(__attribute__((address_space(3))) void *)(dst + k * 1024), 16, 0, 0);
	};

	uint4 acur[NAF][AW], anxt[NAF][AW];
	if (t0 < t1) {
#pragma unroll
		for (int f = 0; f < NAF; f++)
#pragma unroll
			for (int p = 0; p < AW; p++) load_A1(acur[f][p], f, p);
#pragma unroll
		for (int i = 0; i < NDMA; i++) dma_B1(t0, i);
	}

	// one 256-sample tile; HH = which of the AW row pieces it reads
	auto tile = [&](int t, auto HH) {
		constexpr int hh = decltype(HH)::value;
		__syncthreads();   // tile t landed (each wave drained its own DMA), tile t-1 fully consumed
		const bool more_B = t + 1 < t1;                  // there is a next tile
		const bool more_A = t + (AW - hh) < t1;          // there is a next row piece set (fetched in the hh = 0 tile)
		// loads of this tile, one per MFMA group: the A pieces of the next tile pair, then the next B tile
		auto vmem_slot = [&](int idx) {
			if (hh == 0 && idx < AW * NAF) {
				if (more_A) load_A1(anxt[idx / AW][idx % AW], idx / AW, idx % AW);
			} else {
				const int i = idx - (hh == 0 ? AW * NAF : 0);
				if (i < NDMA && more_B) dma_B1(t + 1, i);
			}
			__builtin_amdgcn_sched_barrier(0);
		};
		const uint8_t *bt = ldsB + (size_t)(t & 1) * TILE_BYTES;
#pragma unroll
		for (int u = 0; u < 4; u++) {
			const int g = 4 * kg + u;
			v4i bfrag[NBFV];
#pragma unroll
			for (int b = 0; b < NBFV; b++)
				bfrag[b] = *reinterpret_cast<const v4i *>(bt + ((size_t)(g * NCOL + b * 16 + r)) * 16);
#pragma unroll
			for (int f = 0; f < NAF; f++) {
				const uint4 aw = acur[f][hh];
				const uint32_t w = (u == 0) ? aw.x : (u == 1) ? aw.y : (u == 2) ? aw.z : aw.w;
				vmem_slot(u * NAF + f);
				v4i val;   // byte j of val[k] = code of sample 4j + k (mf_pos)
#pragma unroll
				for (int k = 0; k < 4; k++) val[k] = (int)((w >> (2 * k)) & 0x03030303u);
#pragma unroll
				for (int b = 0; b < NBFV; b++)
					acc[f][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(val, bfrag[b], acc[f][b], 0, 0, 0);
				// samples beyond N have all-zero limbs, so stray codes there add nothing
				const uint32_t m3 = w & (w >> 1) & LO_MASK;
				if (__ballot(m3 != 0)) {
					saw_missing = true;
					v4i ms;
#pragma unroll
					for (int k = 0; k < 4; k++) ms[k] = (int)((m3 >> (2 * k)) & 0x01010101u);
#pragma unroll
					for (int b = 0; b < NBFV; b++)
						accm[f][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ms, bfrag[b], accm[f][b], 0, 0, 0);
				}
			}
		}
		if (hh == AW - 1) {
#pragma unroll
			for (int f = 0; f < NAF; f++)
#pragma unroll
				for (int p = 0; p < AW; p++) acur[f][p] = anxt[f][p];
		}
	};
	for (int t = t0; t < t1; t += 2) {
		tile(t, std::integral_constant<int, 0>());
		tile(t + 1, std::integral_constant<int, AW - 1>());
	}

	// ---- results: integer atomics (exact, order-independent)
#pragma unroll
	for (int f = 0; f < NAF; f++) {
#pragma unroll
		for (int reg = 0; reg < 4; reg++) {
			const int v = vbase + 16 * f + kg * 4 + reg;
			if (v < M) {
				int *dst = accbuf + (size_t)v * acc_stride;
#pragma unroll
				for (int b = 0; b < NBFV; b++) atomicAdd(&dst[b * 16 + r], acc[f][b][reg]);
				if (saw_missing) {
#pragma unroll
					for (int b = 0; b < NBFV; b++)
						if (accm[f][b][reg] != 0) atomicAdd(&dst[NCOL + b * 16 + r], accm[f][b][reg]);
				}
			}
		}
	}
}

// ---- fixed-point conversion of real vectors into limb columns
// max|x| of column y -> out[3 * y + slot] (zeroed beforehand)
__global__ void __launch_bounds__(256)
absmax_kernel(const double *__restrict__ X, size_t ld, GrmCols cols, size_t n, int slot,
	unsigned long long *__restrict__ out)
{
	const double *__restrict__ x = X + (size_t)cols.c[blockIdx.y] * ld;
	double m = 0;
	for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
		const double a = fabs(x[i]);
		m = (a > m) ? a : m;      // NaN never wins
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) { const double t = __shfl_xor(m, o, WAVE); m = (t > m) ? t : m; }
	// non-negative doubles order like their bit patterns
	if ((threadIdx.x & (WAVE - 1)) == 0) atomicMax(out + 3 * blockIdx.y + slot, (unsigned long long)__double_as_longlong(m));
}

// exponent e with max|x| * 2^e < 2^54
__device__ __forceinline__ int limb_scale(unsigned long long maxbits)
{
	const double mx = __longlong_as_double((long long)maxbits);
	if (!(mx > 0) || !isfinite(mx)) return 0;
	return 54 - __builtin_amdgcn_frexp_exp(mx);
}

// x[n] of column y -> limb digits in 7 columns of the tile image Fl[ngrp_pad][ncol][16], the first one
// 16 * (y / per_frag) + 7 * (y % per_frag) + off; zeros beyond n.  The columns nobody writes must be
// zero beforehand
__global__ void __launch_bounds__(256)
limbs_kernel(const double *__restrict__ X, size_t ld, GrmCols cols, size_t n, size_t n_pad, int ncol,
	int per_frag, int off, const unsigned long long *__restrict__ maxbits, int slot, uint8_t *__restrict__ Fl)
{
	const int y = blockIdx.y;
	const double *__restrict__ x = X + (size_t)cols.c[y] * ld;
	const int col0 = 16 * (y / per_frag) + MF_NLIMB * (y % per_frag) + off;
	const int e = limb_scale(maxbits[3 * y + slot]);
	for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n_pad; i += (size_t)gridDim.x * blockDim.x) {
		long long q = 0;
		if (i < n) {
			const double v = x[i];
			q = isfinite(v) ? __double2ll_rn(ldexp(v, e)) : 0;
		}
		uint8_t *base = Fl + ((i >> 4) * ncol + col0) * 16 + mf_pos((int)(i & 15));
		long long rem = q;
#pragma unroll
		for (int l = 0; l < MF_NLIMB; l++) {
			const long long d = (l < MF_NLIMB - 1) ? (((rem + 128) & 255) - 128) : rem;
			rem = (rem - d) >> 8;
			base[l * 16] = (uint8_t)(int8_t)d;
		}
	}
}

// deterministic block partial sums per column: out[y * gridDim.x + blockIdx.x] = sum of a[i] (* b[i])
template <bool WITH_B>
__global__ void __launch_bounds__(256)
dot_partial_kernel(const double *__restrict__ A, const double *__restrict__ B, size_t ld, GrmCols cols,
	size_t n, double *__restrict__ out)
{
	__shared__ double sh[4];
	const size_t c = (size_t)cols.c[blockIdx.y];
	const double *__restrict__ a = A + c * ld;
	const double *__restrict__ b = WITH_B ? B + c * ld : nullptr;
	double s[1] = {0};
	for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
		s[0] = WITH_B ? fma(a[i], b[i], s[0]) : s[0] + a[i];
	block_sum<1, 256>(s, sh);
	if (threadIdx.x == 0) out[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s[0];
}

// dot_v of one marker and column from the exact sums of a pass-1 launch with nbfv fragments (a: the column's
// first limb of the marker's row of acc); the one statement of it, for the product and for grm_dot_out_kernel
__device__ __forceinline__ double grm_dot_value(const int *__restrict__ a, int nbfv, int e, double sb, double l0v, double invv)
{
	const HiLo V = mf_limbs(a), T3 = mf_limbs(a + 16 * nbfv);
	const double t3 = ldexp(hl_to_double(T3), -e);
	const double vw = ldexp(hl_to_double(hl_axpy(-3, T3, V)), -e);     // sum over codes 1,2 of code*b
	return l0v * (sb - t3) + invv * vw;
}

// ---- dot_v itself, per column y of a pass-1 launch: Out[cols.c[y]][v] = sum_i G[v, i] b_i (sgx_grm_marker_dots);
// the sums, the scale and the expression are those grm_dot_epilogue turns into x_v
__global__ void __launch_bounds__(256)
grm_dot_out_kernel(size_t M, int nbfv, const int *__restrict__ acc, const unsigned long long *__restrict__ maxb,
	GrmScal sum_b, const double *__restrict__ inv, const double *__restrict__ l0, double *__restrict__ Out, size_t ldo,
	GrmCols cols)
{
	const int y = blockIdx.y;
	const int stride = 32 * nbfv, col = 16 * (y >> 1) + MF_NLIMB * (y & 1);
	const int e = limb_scale(maxb[3 * y]);
	const double sb = sum_b.v[y];
	double *__restrict__ o = Out + (size_t)cols.c[y] * ldo;
	for (size_t v = blockIdx.x * (size_t)blockDim.x + threadIdx.x; v < M; v += (size_t)gridDim.x * blockDim.x)
		o[v] = grm_dot_value(acc + v * stride + col, nbfv, e, sb, l0[v], inv[v]);
}

// ---- pass-1 epilogue: dot_v -> x_v, gam_v, and the C0 partial sums, per column y of a pass-1 launch
// with nbfv fragments (two columns per fragment); x_v, gam_v -> XV / GV row y (stride M),
// C0 partials -> c0_partial[y * gridDim.x + blockIdx.x]
// LOCO: column y leaves out the markers of group excl.v[y] (-1: none): they get x_v = gam_v = 0 and no C0
// term, so pass 2 never sees them; every other marker's values are those of the plain form, bit for bit.
template <bool LOCO>
__global__ void __launch_bounds__(256)
grm_dot_epilogue(size_t M, int nbfv, const int *__restrict__ acc, const unsigned long long *__restrict__ maxb,
	GrmScal sum_b, const double *__restrict__ af, const double *__restrict__ inv,
	const double *__restrict__ l0, double *__restrict__ XV, double *__restrict__ GV,
	double *__restrict__ c0_partial, const int *__restrict__ grp, GrmIdx excl)
{
	__shared__ double sh[4];
	const int y = blockIdx.y;
	const int ex = LOCO ? excl.v[y] : -1;
	const int stride = 32 * nbfv, col = 16 * (y >> 1) + MF_NLIMB * (y & 1);
	const int e = limb_scale(maxb[3 * y]);
	const double sb = sum_b.v[y];
	double *__restrict__ xv = XV + (size_t)y * M;
	double *__restrict__ gv = GV + (size_t)y * M;
	double c0[1] = {0};
	for (size_t v = blockIdx.x * (size_t)blockDim.x + threadIdx.x; v < M; v += (size_t)gridDim.x * blockDim.x) {
		const double dot = grm_dot_value(acc + v * stride + col, nbfv, e, sb, l0[v], inv[v]);
		const double x = dot * inv[v];
		if constexpr (LOCO) {
			if (ex >= 0 && grp[v] == ex) { xv[v] = 0; gv[v] = 0; continue; }
		}
		xv[v] = x;
		gv[v] = (3 - 2 * af[v]) * x;
		c0[0] = fma(dot, l0[v], c0[0]);
	}
	block_sum<1, 256>(c0, sh);
	if (threadIdx.x == 0) c0_partial[(size_t)y * gridDim.x + blockIdx.x] = c0[0];
}

// ---- pass-2 epilogue: out_i = (C0 + X_i - Gam_i) / M
// A sample without a single non-zero standardised genotype (every code missing or on a monomorphic
// marker: diag_i == 0, a sum of squares) has out_i = 0 as a sum of zero terms, and the reference's
// loop gives exactly that; C0 + X_i - Gam_i only cancels to rounding level there.  0 * v keeps a
// NaN or infinity of b visible, as 0 * dot does in the reference (:507-519).
__device__ __forceinline__ double grm_out_value(double C0, double X, double G, double M, double diag_i)
{
	const double v = (C0 + X - G) / M;
	return (diag_i == 0) ? 0 * v : v;
}

// per column y of a pass-2 launch with nbfv fragments (one column per fragment: x limbs 0.., gam limbs 7..)
// LOCO: the divisor is the column's own marker count msub.v[y] = M - M_excl, and the diag_i == 0 rule reads the
// column's own diagonal, row 1 + excl.v[y] of diag ([1 + groups][N]; row 0: the whole GRM)
template <bool LOCO>
__global__ void __launch_bounds__(256)
grm_out_epilogue(int N, size_t M, int nbfv, const int *__restrict__ acc, const unsigned long long *__restrict__ maxb,
	GrmScal C0, const double *__restrict__ diag, double *__restrict__ Out, size_t ldo, GrmCols cols,
	GrmScal msub, GrmIdx excl)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	const int y = blockIdx.y;
	if (i >= N) return;
	const int ex = limb_scale(maxb[3 * y + 1]), eg = limb_scale(maxb[3 * y + 2]);
	const int *a = acc + (size_t)i * (32 * nbfv) + 16 * y;
	const double X = ldexp(hl_to_double(mf_limbs(a)), -ex);                            // code plane x x limbs
	const double G = ldexp(hl_to_double(mf_limbs(a + 16 * nbfv + MF_NLIMB)), -eg);     // missing plane x gam limbs
	const double m = LOCO ? msub.v[y] : (double)M;
	const double di = LOCO ? diag[(size_t)(1 + excl.v[y]) * N + i] : diag[i];
	Out[(size_t)cols.c[y] * ldo + i] = grm_out_value(C0.v[y], X, G, m, di);
}

// ---- vector kernels of PCG_diag_sigma (:581-614); w and minv are shared by the columns, or (PERCOL) column c
// has its own: weights W row widx.v[c], minv row c
// minv = 1 / max(tau0/w + tau1*diag, 1e-4)   (get_diag_sigma :542-559)
__global__ void pcg_minv_kernel(int n, const double *w, const double *diag, double tau0, double tau1, double *minv)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	double v = tau0 / w[i] + tau1 * diag[i];
	if (v < 1e-4) v = 1e-4;
	minv[i] = 1 / v;
}

// the same per column c of cols: w = W row widx.v[c], diag = row 1 + excl.v[c] of D ([1 + groups][n]) -> Minv row c
__global__ void pcg_minv_cols_kernel(int n, const double *W, GrmIdx widx, const double *D, GrmIdx excl,
	double tau0, double tau1, double *Minv, GrmCols cols)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const size_t c = (size_t)cols.c[blockIdx.y];
	double v = tau0 / W[(size_t)widx.v[c] * n + i] + tau1 * D[(size_t)(1 + excl.v[c]) * n + i];
	if (v < 1e-4) v = 1e-4;
	Minv[c * n + i] = 1 / v;
}

// r = b, z = minv*r, p = z, x = 0
template <bool PERCOL>
__global__ void pcg_init_kernel(int n, const double *B, size_t ldb, const double *minv,
	double *R, double *Z, double *P, double *X, GrmCols cols)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const size_t c = (size_t)cols.c[blockIdx.y], o = c * n + i;
	const double ri = B[c * ldb + i];
	R[o] = ri; Z[o] = minv[PERCOL ? o : (size_t)i] * ri; P[o] = Z[o]; X[o] = 0;
}

// Ap = tau0 * p / w + tau1 * gp   (get_crossprod :564-576); GP may be NULL when tau1 == 0
template <bool PERCOL>
__global__ void pcg_ap_kernel(int n, const double *P, const double *w, const double *GP, double tau0, double tau1,
	double *AP, GrmCols cols, GrmIdx widx)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const size_t o = (size_t)cols.c[blockIdx.y] * n + i;
	const size_t wi = PERCOL ? (size_t)widx.v[cols.c[blockIdx.y]] * n + i : (size_t)i;
	const double base = tau0 * (P[o] * (1 / w[wi]));
	AP[o] = GP ? base + tau1 * GP[o] : base;
}

// x += a p; r -= a Ap; z = minv r   (a per column)
template <bool PERCOL>
__global__ void pcg_update_kernel(int n, GrmScal a, const double *P, const double *AP, const double *minv,
	double *X, double *R, double *Z, GrmCols cols)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const size_t o = (size_t)cols.c[blockIdx.y] * n + i;
	const double ai = a.v[blockIdx.y];
	X[o] += ai * P[o];
	const double ri = R[o] - ai * AP[o];
	R[o] = ri; Z[o] = minv[PERCOL ? o : (size_t)i] * ri;
}

// p = z + bet p   (bet per column)
__global__ void pcg_dir_kernel(int n, GrmScal bet, const double *Z, double *P, GrmCols cols)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const size_t o = (size_t)cols.c[blockIdx.y] * n + i;
	P[o] = Z[o] + bet.v[blockIdx.y] * P[o];
}
