// kern_exact.h -- exact p-value of a binary-trait row with few minor alleles: carrier list + a
// Poisson-binomial dynamic programme in one wave
// Part of libsaigehip.so (single translation unit: saigehip.hip).
#pragma once

// ---------------------------------------------------------------------------
// One WAVE per row, EXACT_BLOCK / 64 rows a workgroup, waves looping over the rows; no workgroup barrier, no atomics.
// With the row's table t = lut[4j ..], g_i = t[code_i]; the table is valid when t[1] == 1, (t[0], t[2]) is (0, 2) or
// (2, 0) and t[3] is finite.  Carriers: codes 0..2 with g in {1, 2}, ascending; MAC = sum g over them.
//   A. the 2-bit row is read once in 16-byte pieces (64 samples a lane; a lane loads EXACT_UNROLL pieces before it
//      looks at the first), samples beyond N masked.  64 pieces without a carrier or a missing code -- nearly all of
//      a rare row -- cost the loads and a few bit operations.  64 pieces with carriers rank them by a wave scan of
//      the lanes' counts and write the first SGX_EXACT_LIST of them as (mu, code | y << 2) (the entry of
//      kern_firth.h) into the wave's own LDS slice; MAC is counted over the whole row whether or not the list is
//      full (a full list means MAC > 63: no result).  Code-3 samples are not resampled: every lane adds y - mu of
//      its own in piece order, sample order inside a piece, and the lanes' partials meet in wave_sum's fixed tree;
//      delta = t[3] * that sum.
//   B. f[a] = P(A = a), A = sum_carriers g y, in lane a (a <= MAC <= 63): from f = [1, 0, ...] a carrier is one
//      broadcast read of its entry, one shift of f up by g lanes, and f <- (1 - mu) f + mu f_shifted.  Alongside,
//      on wave-uniform values, A_obs = sum g y and sum g mu in list order; m' = sum g mu - delta.
//   C. d_a = |a - m'|, d_obs = |A_obs - m'| in double; full = sum_{d_a >= d_obs} f[a], gt = sum_{d_a > d_obs} f[a],
//      eq = sum_{d_a == d_obs} f[a], each summed over a = 0 .. MAC ascending (one lane broadcast a term, the terms
//      that do not belong are skipped, not added as zeros -- the same thing for a sum of non-negative terms, and
//      what the definition says).  out4 = {gt + eq / 2, full, MAC, 1}.
// No result ({NaN, NaN, MAC, 0}): MAC == 0 or MAC > max_mac; an invalid table gives {NaN, NaN, 0, 0} and the row is
// not read.  A row's bits depend on the row, its table and the model only: nothing here knows the row's index, the
// grid or another row.

#define SGX_EXACT_LIST 64         /* list entries of a wave's LDS slice: one more than SGX_EXACT_MAX_MAC carriers can fill */
#define EXACT_BLOCK 256
#define EXACT_UNROLL 4            /* 16-byte pieces a lane loads before it looks at the first */

// v of lane `src` (wave-uniform) in every lane
__device__ __forceinline__ double wave_bcast(double v, int src) { return __shfl(v, src, WAVE); }

__global__ void __launch_bounds__(EXACT_BLOCK)
exact_kernel(const uint8_t *__restrict__ rows, size_t bpv, int N, size_t M, const double *__restrict__ lut,
	const double *__restrict__ mu, const double *__restrict__ y, int max_mac, double *__restrict__ out4)
{
	constexpr int NW = EXACT_BLOCK / WAVE;
	__shared__ double mu_s[NW][SGX_EXACT_LIST];
	__shared__ uint8_t cy_s[NW][SGX_EXACT_LIST];
	const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
	double *mu_l = mu_s[wid];
	uint8_t *cy_l = cy_s[wid];
	const int npiece = (N + 63) >> 6;

	for (size_t v = (size_t)blockIdx.x * NW + wid; v < M; v += (size_t)gridDim.x * NW) {
		double t[4];
#pragma unroll
		for (int c = 0; c < 4; c++) t[c] = lut[v * 4 + c];
		double *o = out4 + v * 4;
		const bool plain = t[0] == 0 && t[2] == 2, flipped = t[0] == 2 && t[2] == 0;
		if (!(t[1] == 1 && (plain || flipped) && isfinite(t[3]))) {      // (wave-uniform: every lane read the same table)
			if (lane == 0) { o[0] = NAN; o[1] = NAN; o[2] = 0; o[3] = 0; }
			continue;
		}
		const uint32_t fswap = plain ? 0u : LO_MASK;       // code 1 is the het; the hom is code 2, code 0 where flipped

		// ---- A: one pass over the row
		const uint8_t *row = rows + v * bpv;
		int nnz = 0, mac = 0;                              // wave-uniform: carriers ranked so far; per lane: its allele count
		double miss = 0;                                   // per lane: sum of y - mu over its code-3 samples
		for (int p0 = 0; p0 < npiece; p0 += WAVE * EXACT_UNROLL) {
			uint4 q[EXACT_UNROLL];
#pragma unroll
			for (int u = 0; u < EXACT_UNROLL; u++) {       // the round's loads first: EXACT_UNROLL KiB a wave in flight
				const int p = p0 + u * WAVE + lane;
				q[u] = p < npiece ? *reinterpret_cast<const uint4 *>(row + (size_t)p * 16) : make_uint4(0, 0, 0, 0);
			}
#pragma unroll
			for (int u = 0; u < EXACT_UNROLL; u++) {
				const int p = p0 + u * WAVE + lane;        // (beyond the row: keep_mask leaves nothing of the zeros)
				const uint32_t wd[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
				uint32_t car[4], mis[4], any_mis = 0;
				int cnt = 0;
				const bool edge = p * 64 + 64 > N;         // the piece holds samples beyond N (or lies beyond the row)
#pragma unroll
				for (int d = 0; d < 4; d++) {
					// low and high bit of every code; a flipped table swaps codes 0 and 2: the high bit turns where the low is 0
					const uint32_t lo = wd[d] & LO_MASK, hi = ((wd[d] >> 1) & LO_MASK) ^ (~lo & fswap);
					uint32_t c = lo ^ hi, m3 = lo & hi, h2 = hi & ~lo;       // het or hom, missing, hom
					if (edge) {
						const uint32_t keep = keep_mask(N - (p * 64 + d * 16));
						c &= keep; m3 &= keep; h2 &= keep;
					}
					car[d] = c; mis[d] = m3;
					cnt += __popc(c);
					mac += __popc(c) + __popc(h2);
					any_mis |= m3;
				}
				if (__ballot(cnt != 0) != 0) {             // (wave-uniform) pieces with carriers: rank and list them
					const int incl = wave_scan_incl_i(cnt);
					int pos = nnz + incl - cnt;
					nnz += __builtin_amdgcn_readlane(incl, WAVE - 1);
#pragma unroll
					for (int d = 0; d < 4; d++) {
						uint32_t m = car[d];
						while (m) {
							const int b = __ffs(m) - 1;      // bit 2s
							m &= m - 1;
							if (pos < SGX_EXACT_LIST) {
								const int i = p * 64 + d * 16 + (b >> 1);
								mu_l[pos] = mu[i];
								cy_l[pos] = (uint8_t)(((wd[d] >> b) & 3u) | (y[i] != 0 ? 4u : 0u));
							}
							pos++;
						}
					}
				}
				if (any_mis) {
#pragma unroll
					for (int d = 0; d < 4; d++) {
						uint32_t m = mis[d];
						while (m) {
							const int b = __ffs(m) - 1;
							m &= m - 1;
							const int i = p * 64 + d * 16 + (b >> 1);
							miss += y[i] - mu[i];
						}
					}
				}
			}
		}
		const int MAC = wave_sum_i(mac);
		if (MAC == 0 || MAC > max_mac) {                   // (wave-uniform)
			if (lane == 0) { o[0] = NAN; o[1] = NAN; o[2] = (double)MAC; o[3] = 0; }
			continue;
		}
		const double delta = t[3] * wave_sum(miss);
		// the list is this wave's own: its LDS operations complete in order, the compiler must not move them
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

		// ---- B: the pmf of A, f[a] in lane a (nnz <= MAC <= 63 entries are listed)
		double f = lane == 0 ? 1.0 : 0.0, gmu = 0;
		int a_obs = 0;
		for (int k = 0; k < nnz; k++) {
			const double m = mu_l[k];
			const uint32_t cy = cy_l[k];
			const int g = (cy & 3u) == 1u ? 1 : 2;
			const double up = __shfl_up(f, g, WAVE);
			const double fs = lane >= g ? up : 0.0;
			f = (1 - m) * f + m * fs;
			gmu += (double)g * m;
			a_obs += (cy & 4u) ? g : 0;
		}
		__builtin_amdgcn_wave_barrier();                   // the next row's list is written after these reads

		// ---- C: the two tails, ascending a
		const double mp = gmu - delta;
		const double d_obs = fabs((double)a_obs - mp);
		double full = 0, gt = 0, eq = 0;
		for (int a = 0; a <= MAC; a++) {
			const double fa = wave_bcast(f, a), d = fabs((double)a - mp);
			if (d >= d_obs) full += fa;
			if (d > d_obs) gt += fa;
			if (d == d_obs) eq += fa;
		}
		if (lane == 0) { o[0] = gt + 0.5 * eq; o[1] = full; o[2] = (double)MAC; o[3] = 1; }
	}
}
