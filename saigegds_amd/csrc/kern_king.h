// kern_king.h -- KING-robust kinship: five exact integer counts per pair of samples, contracted over the
// markers of a sgx_grm handle's sample-major 2-bit transpose Gt.  No allele frequency, no floating-point sum.
//   king_counts_kernel   the five counts of a rectangle of pairs
//   king_pairs_kernel    the related pairs (i < j, kinship >= cutoff) of the tiles on and above the diagonal, as a list
// Part of libsaigehip.so (single translation unit: saigehip.hip).
//
// Counts of a pair (i, j), over the markers v < M where both are called (code != 3):
//     nn both called    hi code_i == 1    hj code_j == 1    hh both == 1    ibs0 (0, 2) or (2, 0)
// Planes, int8 per (sample, marker): p = [code != 3], h = [code == 1], c = code - 1 where called and 0 where missing
// (-1, 0, +1: the signed homozygote plane).  Five products of v_mfma_i32_16x16x64_i8:
//     nn = p.p    hi = h.p    hj = p.h    hh = h.h    cc = c.c = (both homozygous, same) - ibs0
// and with the homozygote indicator o = p - h: o.o = nn - hi - hj + hh = (same) + ibs0, so
//     ibs0 = (nn - hi - hj + hh - cc) / 2, an even number halved: exact.
// Every sum is an int32 of magnitude <= M < 2^31.  A code at or beyond M is turned into 3 before the planes are made,
// so what Gt holds there enters nothing.
//
// Tile shape of grm_screen_kernel: 4 waves own 64 x 64 pairs; per step of 128 markers thread t decodes 64 codes of one
// of the 128 samples (64 row samples, 64 column samples; its half of the step) into the three planes in LDS, once for
// the whole tile; wave w multiplies its 16 rows with the 4 column sub-tiles.  The decode is bit arithmetic on the packed
// dword (no table): the missing mask and p on all 16 fields at once, then (x >> 2t) & 0x03030303 per plane as in
// kern_ld.h, which puts markers t, t + 4, t + 8, t + 12 of the dword in the bytes of output dword t.  A and B use that
// same k map, so no sum depends on it.  The markers are not cut into slabs: the pair list needs a pair's complete counts
// in one place, and at the sizes where the kernel's time matters the tile grid alone fills the device.

#define KG_T 64                         /* samples per workgroup tile edge (4 sub-tiles of 16)                  */
#define KG_KB 128                       /* markers per step (two K = 64 MFMAs)                                   */
#define KG_ROWB (KG_KB + 16)            /* LDS bytes per sample of a plane (padded as GD_ROWB)                   */
#define KG_PLANE (KG_T * KG_ROWB)       /* one plane of one side                                                 */
#define KG_LDS (2 * 3 * KG_PLANE)       /* [side][plane p, h, c][sample][KG_ROWB] = 55 296 bytes                 */

struct KgCounts { gd_i4 q[5][4]; };     // [nn, hi, hj, hh, ibs0][column sub-tile]: C/D map of a 16 x 16 int32 tile

// 16 codes of one dword -> 16 bytes of each plane
__device__ __forceinline__ void kg_planes(uint32_t w, uint4 &p, uint4 &h, uint4 &c)
{
	const uint32_t m = w & (w >> 1) & 0x55555555u;           // 1 in a field whose code is 3
	const uint32_t pb = m ^ 0x55555555u;                     // 1 where called
	const uint32_t wk = w ^ (m << 1);                        // codes 0, 1, 2 and 1 for missing
	uint32_t pv[4], hv[4], cv[4];
#pragma unroll
	for (int t = 0; t < 4; t++) {
		const uint32_t x = (wk >> (2 * t)) & 0x03030303u;
		const uint32_t pt = (pb >> (2 * t)) & 0x01010101u;
		const uint32_t ct = (x + 0x7F7F7F7Fu) ^ 0x80808080u; // bytes: 0 -> 0xFF, 1 -> 0, 2 -> 1 (no carry leaves a byte)
		pv[t] = pt;
		cv[t] = ct;
		hv[t] = pt ^ (ct & 0x01010101u);                     // called and not homozygous
	}
	p = make_uint4(pv[0], pv[1], pv[2], pv[3]);
	h = make_uint4(hv[0], hv[1], hv[2], hv[3]);
	c = make_uint4(cv[0], cv[1], cv[2], cv[3]);
}

// The five counts of the 64 x 64 pairs (row0 + a, col0 + b) into o: wave w of the workgroup gets rows 16 w .. of them.
// Samples at or beyond N are read as sample N - 1 (their entries are never stored).  sm: KG_LDS bytes.
__device__ __forceinline__ void kg_contract(const uint8_t *__restrict__ gt, size_t bpvM, int N, size_t M, int row0,
	int col0, uint8_t *sm, KgCounts &o)
{
	const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
	const int half = __builtin_amdgcn_readfirstlane(t >> 7);
	const int side = __builtin_amdgcn_readfirstlane((t >> 6) & 1);
	const int smp = min((side ? col0 : row0) + lane, N - 1);
	const uint8_t *grow = gt + (size_t)smp * bpvM + half * 16;
	uint8_t *dst = sm + (side * 3 * KG_T + lane) * KG_ROWB + half * 64;
	const int fr = lane & 15, fq = lane >> 4;
	const uint8_t *af = sm + (16 * wid + fr) * KG_ROWB + 16 * fq;
	const uint8_t *bf = sm + 3 * KG_PLANE + fr * KG_ROWB + 16 * fq;
	const gd_i4 z4 = {0, 0, 0, 0};
	gd_i4 pp[4], hp[4], ph[4], hh[4], cc[4];
#pragma unroll
	for (int c = 0; c < 4; c++) pp[c] = hp[c] = ph[c] = hh[c] = cc[c] = z4;
	const int nsteps = (int)((M + KG_KB - 1) / KG_KB);
	uint4 wn = *reinterpret_cast<const uint4 *>(grow);
	for (int st = 0; st < nsteps; st++) {
		uint4 w = wn;
		if (st + 1 < nsteps) wn = *reinterpret_cast<const uint4 *>(grow + (size_t)(st + 1) * 32);
		uint32_t wq[4] = {w.x, w.y, w.z, w.w};
		if ((size_t)(st + 1) * KG_KB > M) {                 // (block-uniform) the step that holds marker M: codes >= M -> 3
			const long long left = (long long)M - ((long long)st * KG_KB + half * 64);
#pragma unroll
			for (int q = 0; q < 4; q++) {
				const long long r = left - 16 * q;          // markers of this dword below M
				if (r <= 0) wq[q] = 0xFFFFFFFFu;
				else if (r < 16) wq[q] |= 0xFFFFFFFFu << (2 * (int)r);
			}
		}
		__syncthreads();                                    // the previous step's fragment reads are done
#pragma unroll
		for (int q = 0; q < 4; q++) {
			uint4 p, h, c;
			kg_planes(wq[q], p, h, c);
			*reinterpret_cast<uint4 *>(dst + 16 * q) = p;
			*reinterpret_cast<uint4 *>(dst + KG_PLANE + 16 * q) = h;
			*reinterpret_cast<uint4 *>(dst + 2 * KG_PLANE + 16 * q) = c;
		}
		__syncthreads();
#pragma unroll
		for (int ks = 0; ks < KG_KB / 64; ks++) {
			const gd_i4 ap = *reinterpret_cast<const gd_i4 *>(af + 64 * ks);
			const gd_i4 ah = *reinterpret_cast<const gd_i4 *>(af + KG_PLANE + 64 * ks);
			const gd_i4 ac = *reinterpret_cast<const gd_i4 *>(af + 2 * KG_PLANE + 64 * ks);
#pragma unroll
			for (int c = 0; c < 4; c++) {
				const gd_i4 bp = *reinterpret_cast<const gd_i4 *>(bf + 16 * c * KG_ROWB + 64 * ks);
				const gd_i4 bh = *reinterpret_cast<const gd_i4 *>(bf + KG_PLANE + 16 * c * KG_ROWB + 64 * ks);
				const gd_i4 bc = *reinterpret_cast<const gd_i4 *>(bf + 2 * KG_PLANE + 16 * c * KG_ROWB + 64 * ks);
				pp[c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ap, bp, pp[c], 0, 0, 0);
				hp[c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, bp, hp[c], 0, 0, 0);
				ph[c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ap, bh, ph[c], 0, 0, 0);
				hh[c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, bh, hh[c], 0, 0, 0);
				cc[c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ac, bc, cc[c], 0, 0, 0);
			}
		}
	}
#pragma unroll
	for (int c = 0; c < 4; c++) {
		o.q[0][c] = pp[c]; o.q[1][c] = hp[c]; o.q[2][c] = ph[c]; o.q[3][c] = hh[c];
		o.q[4][c] = (pp[c] - hp[c] - ph[c] + hh[c] - cc[c]) >> 1;
	}
}

// out[q][(i - i0) * nj + (j - j0)] = count q of the pair (i, j), i0 <= i < i0 + ni, j0 <= j < j0 + nj <= N: tiles as
// they fall, the diagonal is nothing special.  grid = (ceil(nj / 64), ceil(ni / 64)), block = 4 waves.
__global__ void __launch_bounds__(256)
king_counts_kernel(const uint8_t *__restrict__ gt, size_t bpvM, int N, size_t M, int i0, int ni, int j0, int nj,
	int *__restrict__ out)
{
	__shared__ __attribute__((aligned(16))) uint8_t sm[KG_LDS];
	const int row0 = i0 + (int)blockIdx.y * KG_T, col0 = j0 + (int)blockIdx.x * KG_T;
	KgCounts k;
	kg_contract(gt, bpvM, N, M, row0, col0, sm, k);
	// C/D map: column = lane & 15, row = 4 (lane >> 4) + reg
	const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
	const size_t plane = (size_t)ni * nj;
#pragma unroll
	for (int c = 0; c < 4; c++) {
		const int j = col0 + 16 * c + fr;
#pragma unroll
		for (int r = 0; r < 4; r++) {
			const int i = row0 + 16 * wid + 4 * fq + r;
			if (i >= i0 + ni || j >= j0 + nj) continue;
			int *e = out + (size_t)(i - i0) * nj + (j - j0);
#pragma unroll
			for (int q = 0; q < 5; q++) e[q * plane] = k.q[q][c][r];
		}
	}
}

// KING-robust kinship (between-family form) and the share of IBS0 markers from a pair's counts: one conversion per
// integer, one division, one subtraction -- nothing a compiler can contract (4.0 mn is exact).  mn > 0 implies nn > 0.
__device__ __forceinline__ double kg_kinship(int hi, int hj, int hh, int ibs0, int mn)
{
	const int D = (hi + hj - 2 * hh) + 4 * ibs0;             // sum over both-called of (g_i - g_j)^2
	return 0.5 - (double)D / (4.0 * (double)mn);
}

// Every pair i < j < N with mn = min(hi, hj) > 0 and kinship >= cutoff, from the tiles with bj >= bi (the others leave
// at once): the slot comes from a counter (the host sorts), the values are plain stores.  grid = (nb, nb).
__global__ void __launch_bounds__(256)
king_pairs_kernel(const uint8_t *__restrict__ gt, size_t bpvM, int N, size_t M, double cutoff, int *__restrict__ io,
	int *__restrict__ jo, double *__restrict__ kin, double *__restrict__ ibs, int *__restrict__ c5,
	unsigned long long *__restrict__ cnt, size_t cap)
{
	__shared__ __attribute__((aligned(16))) uint8_t sm[KG_LDS];
	if (blockIdx.x < blockIdx.y) return;
	const int row0 = (int)blockIdx.y * KG_T, col0 = (int)blockIdx.x * KG_T;
	KgCounts k;
	kg_contract(gt, bpvM, N, M, row0, col0, sm, k);
	const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
#pragma unroll
	for (int c = 0; c < 4; c++) {
		const int j = col0 + 16 * c + fr;
#pragma unroll
		for (int r = 0; r < 4; r++) {
			const int i = row0 + 16 * wid + 4 * fq + r;
			if (i >= j || j >= N) continue;
			const int nn = k.q[0][c][r], hi = k.q[1][c][r], hj = k.q[2][c][r], hh = k.q[3][c][r], i0 = k.q[4][c][r];
			const int mn = min(hi, hj);
			if (mn <= 0) continue;
			const double kv = kg_kinship(hi, hj, hh, i0, mn);
			if (!(kv >= cutoff)) continue;
			const unsigned long long slot = atomicAdd(cnt, 1ull);
			if (slot >= cap) continue;
			io[slot] = i; jo[slot] = j; kin[slot] = kv; ibs[slot] = (double)i0 / (double)nn;
			int *e = c5 + slot * 5;
			e[0] = nn; e[1] = hi; e[2] = hj; e[3] = hh; e[4] = i0;
		}
	}
}
