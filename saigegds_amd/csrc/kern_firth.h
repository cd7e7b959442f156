// kern_firth.h -- Firth bias-reduced effect size of a binary-trait row: compaction + safeguarded Newton
// Part of libsaigehip.so (single translation unit: saigehip.hip).
#pragma once

// ---------------------------------------------------------------------------
// One workgroup per row (workgroups loop over the rows when there are more rows than the grid).  With the null
// model's fitted mean mu as offset the penalised fit has ONE parameter:
//     logit p_i(b) = logit mu_i + b g_i,    w_i = p_i (1 - p_i),    g_i = lut[code_i]
//     I = sum w g^2     A = sum w (1 - 2p) g^3     B = sum w (1 - 6w) g^4
//     U* = sum g (y - p) + A / 2I            (score of  loglik + 1/2 log I)
//     dU*/db = -I + (B / I - A^2 / I^2) / 2
// and a sample with g = 0 is in none of the sums.
//   A. the 2-bit row is read once in 16-byte pieces (64 samples a thread); the samples with g != 0 are compacted in
//      ascending sample order into a private list of (mu, code | y << 2): the first FIRTH_LDS_N entries in LDS, the
//      rest -- a flipped row lists nearly every sample -- in the workgroup's slice of a scratch buffer.
//   B. Newton on U* from b = 0, with U* / I where dU*/db >= 0 (Fisher scoring's step), steps capped at +-5 and kept
//      inside the sign bracket (lo, hi) (lo: last b with U* > 0, hi: last with U* < 0) by bisection once BOTH ends
//      are finite -- a step ONTO the far end counts as leaving (a capped step does land there: 0 -> 5 -> 0 -> ...), a
//      step of zero does not (the iterate is an end of its own bracket); done when |step| <= 1e-12 max(1, |b|).  The four sums of an iteration come from one pass over
//      the list: every thread its entries k = tid, tid + BLOCK, ... in order, then block_sum's fixed tree -- no
//      atomics, so a row's bits depend on the row, its table and the model only.
// Only four values of g occur, so e = exp(-|b g|) is evaluated per code, not per entry; an entry costs one reciprocal.
// p and 1 - p are formed without cancellation and without overflow from
//     b g <= 0:  a = mu e,  c = 1 - mu           b g > 0:  a = mu,  c = (1 - mu) e
//     p = a / (a + c),   1 - p = c / (a + c)          (firth_entry, shared with kern_firth_ds.h).
// All threads execute the scalar control flow redundantly on identical values (as kern_spa.h).

#define FIRTH_LDS_N 4096          /* list entries held in LDS: 36 KiB a workgroup, four workgroups a CU */
#define FIRTH_BLOCK 256
#define FIRTH_STEP_MAX 5.0
#define FIRTH_TOL 1e-12

// entries of a workgroup's scratch slice for rows of N samples (those beyond the LDS part), a multiple of 64
__host__ __device__ __forceinline__ size_t firth_slice_entries(int N)
{
	return N > FIRTH_LDS_N ? (((size_t)(N - FIRTH_LDS_N) + 63) & ~(size_t)63) : 0;
}
// ... and its bytes: the doubles first, then the bytes (kept 8-byte aligned)
__host__ __device__ __forceinline__ size_t firth_slice_bytes(int N) { return firth_slice_entries(N) * 9; }

// bit 2s set iff the code of sample s of the dword equals c
__device__ __forceinline__ uint32_t eq_fields(uint32_t w, uint32_t c)
{
	const uint32_t e = ~(w ^ (c * LO_MASK));
	return e & (e >> 1) & LO_MASK;
}

struct FirthList {
	const double *mu_l; const uint8_t *cy_l;       // LDS part: entries [0, FIRTH_LDS_N)
	const double *mu_g; const uint8_t *cy_g;       // scratch part: entry k at k - FIRTH_LDS_N
	int nnz;
};

// One list entry's terms of I, A, B and sum g (y - p): m its fitted mean, gi != 0 its dosage, yi its trait, e =
// exp(-|b gi|), pos = b gi > 0.  The one statement of the per-entry arithmetic: firth_sums below and kern_firth_ds.h
// both inline it, so that the compiler contracts it the same way in both.
__device__ __forceinline__ void firth_entry(double m, double gi, bool yi, double e, bool pos, double (&s)[4])
{
	const double a = pos ? m : m * e, c = pos ? (1 - m) * e : 1 - m;
	const double r = fast_rcp(a + c);
	const double p = a * r, q = c * r, w = p * q, g2 = gi * gi;
	s[0] = fma(w, g2, s[0]);
	s[1] = fma(w * (q - p), g2 * gi, s[1]);
	s[2] = fma(w * fma(-6.0, w, 1.0), g2 * g2, s[2]);
	s[3] = fma(gi, yi ? q : -p, s[3]);
}

// I, A, B and sum g (y - p) at b over the list
__device__ __forceinline__ void firth_sums(double b, const double (&g)[4], const FirthList &L, double *sh, double (&s)[4])
{
	double e[4];
	uint32_t pos = 0;                         // bit c: b g[c] > 0
#pragma unroll
	for (int c = 0; c < 4; c++) {
		const double x = b * g[c];
		e[c] = exp(-fabs(x));
		pos |= (x > 0) ? (1u << c) : 0u;
	}
	s[0] = s[1] = s[2] = s[3] = 0;
	for (int k = threadIdx.x; k < L.nnz; k += FIRTH_BLOCK) {
		const bool in_lds = k < FIRTH_LDS_N;
		const double m = in_lds ? L.mu_l[k] : L.mu_g[k - FIRTH_LDS_N];
		const uint32_t cy = in_lds ? L.cy_l[k] : L.cy_g[k - FIRTH_LDS_N];
		const uint32_t code = cy & 3u;
		firth_entry(m, sel4(g, code), (cy & 4u) != 0, sel4(e, code), ((pos >> code) & 1u) != 0, s);
	}
	block_sum<4, FIRTH_BLOCK>(s, sh);
}

// Phase B: the root of U* over a list of nnz entries whose four sums at b `sums(b, s)` makes (every thread calls it
// with the same b and gets the same s) -> o[0..3] = {beta, SE, iterations, converged}, written by thread 0.
template <typename F>
__device__ __forceinline__ void firth_root(int nnz, int maxit, F &&sums, double *o)
{
	double beta = 0, lo = -INFINITY, hi = INFINITY, se = NAN;
	int it = 0, state = 0;                // 0 running, 1 converged, 2 no information (I = 0 or a non-finite sum)
	double s[4];
	if (nnz == 0) state = 2;
	while (state == 0 && it < maxit) {
		it++;
		sums(beta, s);
		const double I = s[0], A = s[1], B = s[2];
		const double U = s[3] + 0.5 * A / I;
		if (!(I > 0) || !isfinite(U)) { state = 2; break; }
		const double dU = -I + 0.5 * (B / I - (A / I) * (A / I));
		if (U > 0) lo = beta; else if (U < 0) hi = beta;
		double d = (dU < 0) ? -U / dU : U / I;
		d = fmin(FIRTH_STEP_MAX, fmax(-FIRTH_STEP_MAX, d));
		double nb = beta + d;
		if (isfinite(lo) && isfinite(hi) && nb != beta && !(nb > lo && nb < hi)) nb = 0.5 * (lo + hi);
		if (U == 0) nb = beta;
		d = nb - beta;
		beta = nb;
		if (fabs(d) <= FIRTH_TOL * fmax(1.0, fabs(beta))) state = 1;
	}
	if (state == 1) {                     // SE at the root itself
		sums(beta, s);
		se = 1.0 / sqrt(s[0]);
		if (!(s[0] > 0)) state = 2;
	}
	if (threadIdx.x == 0) {
		o[0] = state == 2 ? NAN : beta;
		o[1] = state == 1 ? se : NAN;
		o[2] = (double)it;
		o[3] = state == 1 ? 1.0 : 0.0;
	}
}

__global__ void __launch_bounds__(FIRTH_BLOCK)
firth_kernel(const uint8_t *__restrict__ rows, size_t bpv, int N, size_t M, const double *__restrict__ lut,
	const double *__restrict__ mu, const double *__restrict__ y, int maxit, uint8_t *scratch,
	double *__restrict__ out4)
{
	constexpr int NW = FIRTH_BLOCK / WAVE;
	__shared__ double mu_l[FIRTH_LDS_N];
	__shared__ uint8_t cy_l[FIRTH_LDS_N];
	__shared__ double sh[4 * NW];
	__shared__ int shc[NW];
	const int tid = threadIdx.x, lane = tid & (WAVE - 1), wid = tid / WAVE;
	const size_t slice = firth_slice_entries(N);
	double *mu_g = reinterpret_cast<double *>(scratch + (size_t)blockIdx.x * firth_slice_bytes(N));
	uint8_t *cy_g = reinterpret_cast<uint8_t *>(mu_g + slice);
	const int npiece = (N + 63) >> 6;

	for (size_t v = blockIdx.x; v < M; v += gridDim.x) {
		double g[4];
		bool finite = true;
		uint32_t nzc = 0;                     // bit c: code c has a non-zero dosage
#pragma unroll
		for (int c = 0; c < 4; c++) {
			g[c] = lut[v * 4 + c];
			finite = finite && isfinite(g[c]);
			nzc |= (g[c] != 0) ? (1u << c) : 0u;
		}
		double *o = out4 + v * 4;
		if (!finite) {                        // (uniform: every thread read the same table)
			if (tid == 0) { o[0] = NAN; o[1] = NAN; o[2] = 0; o[3] = 0; }
			continue;
		}

		// ---- A: compaction, 64 samples a thread and FIRTH_BLOCK pieces a round
		const uint8_t *row = rows + v * bpv;
		int nnz = 0;
		__syncthreads();                      // the previous row's readers of the list are done
		for (int p0 = 0; p0 < npiece; p0 += FIRTH_BLOCK) {
			const int p = p0 + tid;
			uint32_t msk[4] = {0, 0, 0, 0}, wd[4] = {0, 0, 0, 0};
			int cnt = 0;
			if (p < npiece) {
				const uint4 q = *reinterpret_cast<const uint4 *>(row + (size_t)p * 16);
				wd[0] = q.x; wd[1] = q.y; wd[2] = q.z; wd[3] = q.w;
#pragma unroll
				for (int d = 0; d < 4; d++) {
					uint32_t m = 0;
#pragma unroll
					for (uint32_t c = 0; c < 4; c++) m |= ((nzc >> c) & 1u) ? eq_fields(wd[d], c) : 0u;
					m &= keep_mask(N - (p * 64 + d * 16)) & LO_MASK;
					msk[d] = m;
					cnt += __popc(m);
				}
			}
			const int incl = wave_scan_incl_i(cnt);
			if (lane == WAVE - 1) shc[wid] = incl;
			__syncthreads();
			int pos = nnz + incl - cnt, total = 0;
#pragma unroll
			for (int w = 0; w < NW; w++) { if (w < wid) pos += shc[w]; total += shc[w]; }
#pragma unroll
			for (int d = 0; d < 4; d++) {
				uint32_t m = msk[d];
				while (m) {
					const int b = __ffs(m) - 1;          // bit 2s
					m &= m - 1;
					const int i = p * 64 + d * 16 + (b >> 1);
					const uint32_t cy = ((wd[d] >> b) & 3u) | (y[i] != 0 ? 4u : 0u);
					if (pos < FIRTH_LDS_N) { mu_l[pos] = mu[i]; cy_l[pos] = (uint8_t)cy; }
					else { mu_g[pos - FIRTH_LDS_N] = mu[i]; cy_g[pos - FIRTH_LDS_N] = (uint8_t)cy; }
					pos++;
				}
			}
			nnz += total;
			__syncthreads();                  // shc is free for the next round; the last one publishes the list
		}
		__threadfence_block();

		// ---- B: the root of U*
		const FirthList L = {mu_l, cy_l, mu_g, cy_g, nnz};
		firth_root(nnz, maxit, [&](double b, double (&s)[4]) { firth_sums(b, g, L, sh, s); }, o);
	}
}
