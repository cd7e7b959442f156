// kern_grm_dense.h -- the explicit GRM: K = G'G/M as numbers, in dense blocks and as the thresholded
// sparse relatedness matrix, from the sample-major 2-bit transpose Gt and the per-marker table (inv, l0) of a
// sgx_grm handle.  Nothing of this is in the reference (it has the GRM as an operator only).
//   grm_dense_tile_kernel   one 16 x 16 tile of K in FP64 on the matrix cores: THE definition of K_ij
//   grm_screen_kernel       sum_v Q_vi Q_vj exactly in int8 limbs (Q = round(g 2^s)): which 16 x 16 sub-tiles may
//                           hold a pair at or above the cutoff, by a rigorous bound; it only saves work
// Part of libsaigehip.so (single translation unit: saigehip.hip).
#pragma once

#define GD_SLAB_DW 4096       /* FP64 slab: 4096 dwords = 65536 markers; the cuts depend on M only               */
#define GD_T 64               /* screen: samples per workgroup tile edge (4 sub-tiles of 16)                      */
#define GD_KB 128             /* screen: markers per step (two K = 64 MFMAs)                                      */
#define GD_ROWB (GD_KB + 16)  /* screen: LDS bytes per sample of a limb image (padded: conflict-free b128 reads)  */
#define GD_CHUNK 512          /* screen: steps per int32 chunk, 65536 markers: 127^2 * 65536 < 2^31               */
#define GD_QMAX 16256         /* |Q| <= 127 * 128: limbs h in [-127, 127], l in [-64, 63], Q = 128 h + l          */

typedef int gd_i4 __attribute__((ext_vector_type(4)));

struct GdTile { int a, b; };  // 16-sample tiles of K: rows 16 a .., columns 16 b .., a <= b

// A rectangle's tile grid (rows ti0 .. +nti, columns tj0 .. +ntj) that straddles the diagonal holds some tiles twice,
// as (ti, tj) and as (tj, ti).  Of such a pair only the one with ti < tj is computed; the other is read from it.
__device__ __forceinline__ bool gd_mirrored(int ti, int tj, int ti0, int nti, int tj0, int ntj)
{
	return ti > tj && tj >= ti0 && tj < ti0 + nti && ti >= tj0 && ti < tj0 + ntj;
}

// ---- FP64 tile.  grid = (tiles, slabs), block = one wave.  v_mfma_f64_16x16x4_f64 as in skat_gram_kernel: lane
// (v = lane & 15, h = lane >> 4) gives A[row v][k = h] and B[k = h][col v] and holds D[row h + 4 reg][col v].  The lane
// reads dword d of sample 16 a + v (A) and of sample 16 b + v (B); in step t = 0..3 of the dword its k is marker
// 16 d + 4 t + h.  g = code == 3 ? 0 : fma(code, inv, l0), the form of grm_diag_kernel; markers >= M and samples >= N
// give exact zeros.  A tile is (a, b) from the list, or (list == NULL) the tile of a rectangle's grid, ordered so that
// a <= b.  The slab's tile goes to part[slab][tile][256] by plain stores.  What element (r, c) gets depends on the two
// samples' rows, on inv, l0 and M only: the order of the sum is set by the marker index, whatever the tile, the launch or
// its bounds.
__global__ void __launch_bounds__(64)
grm_dense_tile_kernel(const uint8_t *__restrict__ gt, size_t bpvM, int N, size_t M, const double *__restrict__ inv,
	const double *__restrict__ l0, const GdTile *__restrict__ list, int ti0, int nti, int tj0, int ntj, size_t n_tiles,
	double *__restrict__ part)
{
	GdTile t;
	if (list) t = list[blockIdx.x];
	else {
		const int ti = ti0 + (int)(blockIdx.x / (unsigned)ntj), tj = tj0 + (int)(blockIdx.x % (unsigned)ntj);
		if (gd_mirrored(ti, tj, ti0, nti, tj0, ntj)) return;   // (the grid's tile (tj, ti) holds the same numbers)
		t.a = min(ti, tj); t.b = max(ti, tj);
	}
	const int lane = threadIdx.x, v = lane & 15, hq = lane >> 4;
	const int ia = 16 * t.a + v, ib = 16 * t.b + v;
	const bool aok = ia < N, bok = ib < N;
	const uint32_t *arow = reinterpret_cast<const uint32_t *>(gt + (size_t)min(ia, N - 1) * bpvM);
	const uint32_t *brow = reinterpret_cast<const uint32_t *>(gt + (size_t)min(ib, N - 1) * bpvM);
	const size_t ndw = (M + 15) >> 4;
	const size_t d0 = (size_t)blockIdx.y * GD_SLAB_DW, d1 = min(ndw, d0 + GD_SLAB_DW);
	// three levels, cut by the marker index alone: the MFMA chain runs over 16 dwords (256 markers), 16 chains are
	// added into mid, 16 mids (a slab has 16) into top: no sum has more than 64 + 16 + 16 terms in a row
	skat_d4 acc = {0, 0, 0, 0}, mid = {0, 0, 0, 0}, top = {0, 0, 0, 0};
	for (size_t d = d0; d < d1; d++) {
		const uint32_t wa = arow[d], wb = brow[d];
#pragma unroll
		for (int s4 = 0; s4 < 4; s4++) {
			const int pos = 4 * s4 + hq;
			const size_t mv = 16 * d + pos;
			const bool ok = mv < M;
			const size_t mc = ok ? mv : M - 1;
			const double iv = inv[mc], lv = l0[mc];
			const uint32_t ca = (wa >> (2 * pos)) & 3u, cb = (wb >> (2 * pos)) & 3u;
			const double a = (ok && aok && ca != 3u) ? fma((double)ca, iv, lv) : 0.0;
			const double b = (ok && bok && cb != 3u) ? fma((double)cb, iv, lv) : 0.0;
			acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
		}
		if ((d & 15) == 15 || d + 1 == d1) { mid += acc; acc = skat_d4{0, 0, 0, 0}; }
		if ((d & 255) == 255 || d + 1 == d1) { top += mid; mid = skat_d4{0, 0, 0, 0}; }
	}
	double *o = part + ((size_t)blockIdx.y * n_tiles + blockIdx.x) * 256;
#pragma unroll
	for (int r = 0; r < 4; r++) o[(hq + 4 * r) * 16 + v] = top[r];
}

// K of element (r, c) of a tile: its slabs added in slab order, over M.  The one place a K_ij is put together.
__device__ __forceinline__ double gd_value(const double *__restrict__ part, size_t n_tiles, int nslab, size_t tile,
	int r, int c, size_t M)
{
	double s = 0;
	for (int k = 0; k < nslab; k++) s += part[((size_t)k * n_tiles + tile) * 256 + r * 16 + c];
	return s / (double)M;
}

// out[(i - i0) * nj + (j - j0)] = K_ij of a rectangle whose tile grid (ti0.., tj0.., ntj wide) is in part.  One thread
// per element.  K_ij is read at (min, max): element (i, j) and element (j, i) are the same number of the same tile
// position, whichever of the rectangle's tiles holds it.
__global__ void __launch_bounds__(256)
grm_dense_gather_kernel(const double *__restrict__ part, size_t n_tiles, int nslab, int ti0, int nti, int tj0, int ntj,
	int i0, int ni, int j0, int nj, size_t M, double *__restrict__ out)
{
	const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (e >= (size_t)ni * nj) return;
	const int i = i0 + (int)(e / (size_t)nj), j = j0 + (int)(e % (size_t)nj);
	int ti = i / 16, tj = j / 16;
	if (gd_mirrored(ti, tj, ti0, nti, tj0, ntj)) { const int x = ti; ti = tj; tj = x; }
	const size_t tile = (size_t)(ti - ti0) * ntj + (tj - tj0);
	const int lo = min(i, j), hi = max(i, j);
	out[e] = gd_value(part, n_tiles, nslab, tile, lo & 15, hi & 15, M);
}

// the entries of the flagged tiles: pairs i <= j < N with K_ij >= cutoff, and every diagonal entry.  One workgroup per
// tile, one thread per element.  The slot comes from a counter (the host sorts); the value is a plain store.
__global__ void __launch_bounds__(256)
grm_sparse_compact_kernel(const double *__restrict__ part, size_t n_tiles, int nslab, const GdTile *__restrict__ list,
	int N, size_t M, double cutoff, int *__restrict__ io, int *__restrict__ jo, double *__restrict__ vo,
	unsigned long long *__restrict__ cnt, size_t cap)
{
	const GdTile t = list[blockIdx.x];
	const int r = threadIdx.x >> 4, c = threadIdx.x & 15;
	const int i = 16 * t.a + r, j = 16 * t.b + c;
	if (i >= N || j >= N || i > j) return;
	const double v = gd_value(part, n_tiles, nslab, blockIdx.x, r, c, M);
	if (i != j && !(v >= cutoff)) return;
	const unsigned long long slot = atomicAdd(cnt, 1ull);
	if (slot < cap) { io[slot] = i; jo[slot] = j; vo[slot] = v; }
}

// ---- screen, once per handle: max |g| over the table, the limb table, the per-sample bound terms
__global__ void __launch_bounds__(256)
gd_lutmax_kernel(const double *__restrict__ inv, const double *__restrict__ l0, size_t M, unsigned long long *out)
{
	double m = 0;
	for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < M; v += (size_t)gridDim.x * 256)
		for (int c = 0; c < 3; c++) m = fmax(m, fabs(fma((double)c, inv[v], l0[v])));
	atomicMax(out, (unsigned long long)__double_as_longlong(m));
}

// lut[v] = {h bytes, l bytes} of Q = rint(g 2^s) per code (byte c of the word; code 3 and markers >= M: 0)
__global__ void __launch_bounds__(256)
gd_lut_kernel(const double *__restrict__ inv, const double *__restrict__ l0, size_t M, size_t Mpad, int s,
	uint2 *__restrict__ lut)
{
	const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (v >= Mpad) return;
	uint2 w = make_uint2(0u, 0u);
	if (v < M)
		for (int c = 0; c < 3; c++) {
			const int q = (int)rint(ldexp(fma((double)c, inv[v], l0[v]), s));
			const int l = ((q + 64) & 127) - 64, h = (q - l) >> 7;
			w.x |= (uint32_t)(h & 0xff) << (8 * c);
			w.y |= (uint32_t)(l & 0xff) << (8 * c);
		}
	lut[v] = w;
}

// A_i >= sum_v |g_vi| and R_i >= sqrt(diag_i), both pushed up by 2^-20 (far above their own rounding); one wave per
// sample, addressed as grm_diag_kernel
__global__ void __launch_bounds__(256)
gd_sample_kernel(const uint8_t *__restrict__ gt, size_t bpvM, int N, size_t M, const double *__restrict__ inv,
	const double *__restrict__ l0, const double *__restrict__ diag, double *__restrict__ A, double *__restrict__ R)
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
			s += (code == 3u) ? 0.0 : fabs(fma((double)code, inv[v], l0[v]));
		}
	}
	s = wave_sum(s);
	if (lane == 0) { A[i] = s * (1.0 + 0x1p-20); R[i] = sqrt(diag[i]) * (1.0 + 0x1p-20); }
}

struct GdBound {              // constants of the screen bound, by value
	double p2;                // 2^-2s
	double Md;                // M
	double qa;                // 2^-(s+1) / M
	double qb;                // 2^-(2s+2)
	double rc;                // 4 (M + 8) 2^-53
	double cutoff;
};

// ---- screen.  grid = (nb, nb) workgroup tiles of GD_T samples, those with bj < bi leave at once; block = 4 waves.
// Per step of GD_KB markers thread t decodes 64 codes of one sample (t & 127: the 64 row samples of the tile, then
// its 64 column samples; markers 64 (t >> 7) .. of the step) through the byte table into the two limb images in LDS,
// once for the whole tile.  Wave w then multiplies its 16 rows with the 4 column sub-tiles: hh, hl, lh and ll by
// v_mfma_i32_16x16x64_i8 (A and B use the same k map, so a Gram sum does not depend on it).  Every GD_CHUNK steps the
// int32 sums are folded into int64: S = 2^14 hh + 2^7 (hl + lh) + ll = sum_v Q_vi Q_vj, exact.
// A sub-tile is listed when it is a diagonal one or when some pair of it has approx + delta >= cutoff.
__global__ void __launch_bounds__(256)
grm_screen_kernel(const uint8_t *__restrict__ gt, size_t bpvM, int N, int nsteps, const uint2 *__restrict__ lut,
	const double *__restrict__ A, const double *__restrict__ R, GdBound bd, GdTile *__restrict__ list,
	unsigned long long *__restrict__ cnt, size_t cap)
{
	__shared__ __attribute__((aligned(16))) uint8_t sm[2 * 2 * GD_T * GD_ROWB];   // [side][limb][sample][GD_ROWB]
	const int bi = blockIdx.y, bj = blockIdx.x;
	if (bj < bi) return;
	const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
	const int half = __builtin_amdgcn_readfirstlane(t >> 7);
	const int sidx = t & 127, side = sidx >> 6, sl = sidx & 63;
	const int smp = (side ? bj : bi) * GD_T + sl;
	const bool sok = smp < N;
	const uint8_t *grow = gt + (size_t)min(smp, N - 1) * bpvM + half * 16;
	uint8_t *dH = sm + ((side * 2 + 0) * GD_T + sl) * GD_ROWB + half * 64;
	uint8_t *dL = sm + ((side * 2 + 1) * GD_T + sl) * GD_ROWB + half * 64;
	const int fr = lane & 15, fq = lane >> 4;
	const uint8_t *aH = sm + ((0 * 2 + 0) * GD_T + 16 * wid + fr) * GD_ROWB + 16 * fq;
	const uint8_t *aL = sm + ((0 * 2 + 1) * GD_T + 16 * wid + fr) * GD_ROWB + 16 * fq;
	const uint8_t *bH = sm + ((1 * 2 + 0) * GD_T + fr) * GD_ROWB + 16 * fq;
	const uint8_t *bL = sm + ((1 * 2 + 1) * GD_T + fr) * GD_ROWB + 16 * fq;
	const gd_i4 z4 = {0, 0, 0, 0};
	gd_i4 hh[4], hl[4], lh[4], ll[4];
	long long tot[4][4];
#pragma unroll
	for (int c = 0; c < 4; c++) {
		hh[c] = hl[c] = lh[c] = ll[c] = z4;
#pragma unroll
		for (int r = 0; r < 4; r++) tot[c][r] = 0;
	}
	for (int st = 0; st < nsteps; st++) {
		uint4 w = make_uint4(0u, 0u, 0u, 0u);
		if (sok) w = *reinterpret_cast<const uint4 *>(grow + (size_t)st * 32);
		const uint2 *lp = lut + (size_t)st * GD_KB + half * 64;
		__syncthreads();                               // the previous step's fragment reads are done
		const uint32_t wq[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
		for (int q = 0; q < 4; q++) {
			uint32_t oh[4] = {0, 0, 0, 0}, ol[4] = {0, 0, 0, 0};
#pragma unroll
			for (int k = 0; k < 16; k++) {
				const uint2 e = lp[16 * q + k];
				const uint32_t sh = ((wq[q] >> (2 * k)) & 3u) * 8u;
				oh[k >> 2] |= ((e.x >> sh) & 0xffu) << (8 * (k & 3));
				ol[k >> 2] |= ((e.y >> sh) & 0xffu) << (8 * (k & 3));
			}
			*reinterpret_cast<uint4 *>(dH + 16 * q) = make_uint4(oh[0], oh[1], oh[2], oh[3]);
			*reinterpret_cast<uint4 *>(dL + 16 * q) = make_uint4(ol[0], ol[1], ol[2], ol[3]);
		}
		__syncthreads();
#pragma unroll
		for (int ks = 0; ks < GD_KB / 64; ks++) {
			const gd_i4 ah = *reinterpret_cast<const gd_i4 *>(aH + 64 * ks);
			const gd_i4 al = *reinterpret_cast<const gd_i4 *>(aL + 64 * ks);
#pragma unroll
			for (int c = 0; c < 4; c++) {
				const gd_i4 bh = *reinterpret_cast<const gd_i4 *>(bH + 16 * c * GD_ROWB + 64 * ks);
				const gd_i4 bl = *reinterpret_cast<const gd_i4 *>(bL + 16 * c * GD_ROWB + 64 * ks);
				hh[c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, bh, hh[c], 0, 0, 0);
				hl[c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, bl, hl[c], 0, 0, 0);
				lh[c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, bh, lh[c], 0, 0, 0);
				ll[c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, bl, ll[c], 0, 0, 0);
			}
		}
		if ((st + 1) % GD_CHUNK == 0 || st + 1 == nsteps) {
#pragma unroll
			for (int c = 0; c < 4; c++) {
#pragma unroll
				for (int r = 0; r < 4; r++)
					tot[c][r] += 16384ll * hh[c][r] + 128ll * ((long long)hl[c][r] + lh[c][r]) + ll[c][r];
				hh[c] = hl[c] = lh[c] = ll[c] = z4;
			}
		}
	}
	// C/D map of the 16 x 16 int32 tile: column = lane & 15, row = 4 (lane >> 4) + reg
	const int sti = bi * 4 + wid;
	if (16 * sti >= N) return;
	const int j_l = fr;
	double Ai[4], Ri[4];
#pragma unroll
	for (int r = 0; r < 4; r++) {
		const int i = min(16 * sti + 4 * fq + r, N - 1);
		Ai[r] = A[i]; Ri[r] = R[i];
	}
#pragma unroll
	for (int c = 0; c < 4; c++) {
		const int stj = bj * 4 + c;
		if (stj < sti || 16 * stj >= N) continue;      // (wave-uniform)
		const int j = 16 * stj + j_l;
		const bool jok = j < N;
		const double Aj = A[min(j, N - 1)], Rj = R[min(j, N - 1)];
		bool hit = false;
#pragma unroll
		for (int r = 0; r < 4; r++) {
			const double approx = ((double)tot[c][r] * bd.p2) / bd.Md;
			const double delta = (bd.qa * (Ai[r] + Aj) + bd.qb + bd.rc * Ri[r] * Rj + fabs(approx) * 0x1p-50)
				* (1.0 + 0x1p-20);
			hit |= jok && (16 * sti + 4 * fq + r < N) && (approx + delta >= bd.cutoff);
		}
		const bool any = (stj == sti) || __any(hit);
		if (any && lane == 0) {
			const unsigned long long slot = atomicAdd(cnt, 1ull);
			if (slot < cap) { list[slot].a = sti; list[slot].b = stj; }
		}
	}
}
