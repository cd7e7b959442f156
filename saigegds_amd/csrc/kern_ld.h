// kern_ld.h -- pairwise LD of 2-bit rows: the six integer sums of a pair over the samples called in both rows, and
// the r^2 decision on them.  An integer Gram contracted over the SAMPLES, exact.
// Part of libsaigehip.so (single translation unit: saigehip.hip).
//
// Rows on the device ("canonical rows").  LD_UNIT samples (64 bytes) is the unit of every load: a row takes
// ceil(n_samp / LD_UNIT) units, and every 2-bit field at or beyond n_samp holds code 3 (ld_tail_kernel sees to the
// fields of the last byte, the upload to the bytes after it).  A missing sample contributes to no sum, so the kernels
// below never look at n_samp: whatever the caller's row held beyond it cannot enter a result.
//
// Planes.  With p = [code != 3], x = code p (0, 1, 2) and x2 = x^2 (0, 1, 4) as int8 per sample, the sums of a pair are
//     n = p.p    sx = x.p    sy = p.x    sxx = x2.p    syy = p.x2    sxy = x.x
// six products of v_mfma_i32_16x16x64_i8 per 16 x 16 pairs and 64 samples.  A lane's A (or B) operand is 16 samples of
// one row = one dword of the packed row; val[t] = (w >> 2t) & 0x03030303 puts them in the bytes of four dwords in the
// order mf_pos() (mf_fixed.h), and both sides use the same order, so the sums do not depend on it.  The planes are four
// to six VALU operations per dword of val.  A wave holds 32 x 32 pairs (2 x 2 fragments, 24 accumulators): each side's
// decode then serves two fragments of the other, and the VALU work per MFMA is about a third of a 16 x 16 tile's.
// No LDS: a lane loads its 16 bytes (four MFMA steps of one row) straight from the row.
//
// Exactness.  Every sum is an int32 (<= 4 n_samp < 2^31 for n_samp < 2^29).  The samples are cut into slabs along the
// grid's z; the slabs of a pair meet by integer atomicAdd, which no order of arrival can change.

#define LD_UNIT 256          /* samples of one 64-byte unit of a row                        */
#define LD_TILE 32           /* rows of a wave's tile on either side                        */
#define LD_WAVES 4           /* waves of a workgroup: four tiles of B rows against one of A */

// the fields at and beyond n_samp in the last used byte of each row -> code 3 (missing)
__global__ void ld_tail_kernel(uint8_t *rows, size_t stride, int m, int n_samp)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= m || (n_samp & 3) == 0) return;
	rows[(size_t)i * stride + (n_samp >> 2)] |= (uint8_t)(0xFFu << (2 * (n_samp & 3)));
}

struct LdPlanes { v4i p, x, x2; };

// one dword of a canonical row (16 codes) -> the three int8 planes of its samples
__device__ __forceinline__ LdPlanes ld_planes(uint32_t w)
{
	LdPlanes o;
#pragma unroll
	for (int t = 0; t < 4; t++) {
		const uint32_t v = (w >> (2 * t)) & 0x03030303u;
		const uint32_t m = v & (v >> 1);                 // 1 where the code is 3
		const uint32_t x = v ^ (m * 3u);                 // the code, 0 where missing
		o.p[t] = (int)(m ^ 0x01010101u);
		o.x[t] = (int)x;
		o.x2[t] = (int)((x & 0x01010101u) | ((x & 0x02020202u) << 1));
	}
	return o;
}

// Row c of the B side: a ring of b_cap rows that starts at b_head (a plain matrix: b_head = 0, b_cap >= mb).
// out[(i * ldo + col0 + j) * 6 + q] += the sums of (A row i, B row j) over the slab's samples; `lower`: only the tiles
// that hold a pair with j < i are computed (the block against itself).
// grid = (ceil(mb / (LD_TILE LD_WAVES)), ceil(ma / LD_TILE), slabs), block = 64 LD_WAVES.
__global__ void __launch_bounds__(64 * LD_WAVES)
ld_counts_kernel(const uint8_t *__restrict__ A, int ma, const uint8_t *__restrict__ B, int mb, int b_head, int b_cap,
	size_t stride, int n_units, int units_per_slab, int lower, int *__restrict__ out, int ldo, int col0)
{
	const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
	const int fr = lane & 15, kg = lane >> 4;
	const int i0 = blockIdx.y * LD_TILE, j0 = (blockIdx.x * LD_WAVES + wid) * LD_TILE;
	if (j0 >= mb || (lower && j0 >= i0 + LD_TILE - 1)) return;          // (wave-uniform; no barrier below)
	const int u0 = blockIdx.z * units_per_slab, u1 = min(n_units, u0 + units_per_slab);
	const uint8_t *ap[2], *bp[2];
#pragma unroll
	for (int f = 0; f < 2; f++) {
		const int ia = min(i0 + 16 * f + fr, ma - 1);                   // (rows past the end: a valid row, never stored)
		const int jb = (b_head + min(j0 + 16 * f + fr, mb - 1)) % b_cap;
		ap[f] = A + (size_t)ia * stride + 16 * kg;
		bp[f] = B + (size_t)jb * stride + 16 * kg;
	}
	const v4i z4 = {0, 0, 0, 0};
	v4i acc[2][2][6];
#pragma unroll
	for (int a = 0; a < 2; a++)
#pragma unroll
		for (int b = 0; b < 2; b++)
#pragma unroll
			for (int q = 0; q < 6; q++) acc[a][b][q] = z4;
	for (int u = u0; u < u1; u++) {
		uint4 wa[2], wb[2];
#pragma unroll
		for (int f = 0; f < 2; f++) {
			wa[f] = *reinterpret_cast<const uint4 *>(ap[f] + (size_t)u * 64);
			wb[f] = *reinterpret_cast<const uint4 *>(bp[f] + (size_t)u * 64);
		}
#pragma unroll
		for (int s = 0; s < 4; s++) {
			LdPlanes pa[2], pb[2];
#pragma unroll
			for (int f = 0; f < 2; f++) {
				pa[f] = ld_planes(s == 0 ? wa[f].x : s == 1 ? wa[f].y : s == 2 ? wa[f].z : wa[f].w);
				pb[f] = ld_planes(s == 0 ? wb[f].x : s == 1 ? wb[f].y : s == 2 ? wb[f].z : wb[f].w);
			}
#pragma unroll
			for (int a = 0; a < 2; a++)
#pragma unroll
				for (int b = 0; b < 2; b++) {
					acc[a][b][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(pa[a].p, pb[b].p, acc[a][b][0], 0, 0, 0);
					acc[a][b][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(pa[a].x, pb[b].p, acc[a][b][1], 0, 0, 0);
					acc[a][b][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(pa[a].p, pb[b].x, acc[a][b][2], 0, 0, 0);
					acc[a][b][3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(pa[a].x2, pb[b].p, acc[a][b][3], 0, 0, 0);
					acc[a][b][4] = __builtin_amdgcn_mfma_i32_16x16x64_i8(pa[a].p, pb[b].x2, acc[a][b][4], 0, 0, 0);
					acc[a][b][5] = __builtin_amdgcn_mfma_i32_16x16x64_i8(pa[a].x, pb[b].x, acc[a][b][5], 0, 0, 0);
				}
		}
	}
	// C/D map of a 16 x 16 int32 tile: column (B row) = lane & 15, row (A row) = 4 (lane >> 4) + reg
#pragma unroll
	for (int a = 0; a < 2; a++)
#pragma unroll
		for (int b = 0; b < 2; b++) {
			const int j = j0 + 16 * b + fr;
#pragma unroll
			for (int r = 0; r < 4; r++) {
				const int i = i0 + 16 * a + 4 * kg + r;
				if (i >= ma || j >= mb) continue;
				int *o = out + ((size_t)i * ldo + col0 + j) * 6;
#pragma unroll
				for (int q = 0; q < 6; q++) {
					const int v = acc[a][b][q][r];
					if (v) atomicAdd(o + q, v);
				}
			}
		}
}

// The decision on the six sums of a pair: in LD iff vx > 0, vy > 0 and c^2 > t2 vx vy, with c, vx, vy
// exact in int64 and the comparison in double -- three conversions, three products, no sum to contract.
__global__ void ld_flags_kernel(const int *__restrict__ sums, size_t n_pairs, double t2, uint8_t *__restrict__ flags)
{
	const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= n_pairs) return;
	const int *s = sums + k * 6;
	const long long n = s[0], sx = s[1], sy = s[2], sxx = s[3], syy = s[4], sxy = s[5];
	const long long c = n * sxy - sx * sy, vx = n * sxx - sx * sx, vy = n * syy - sy * sy;
	const double cd = (double)c, lhs = cd * cd, vv = (double)vx * (double)vy, rhs = t2 * vv;
	flags[k] = (uint8_t)(vx > 0 && vy > 0 && lhs > rhs);
}

// the block's rows idx[0 .. n_keep) -> the ring's rows (tail + k) % cap, 16 bytes a thread; grid = (x, n_keep)
__global__ void ld_push_kernel(const uint8_t *__restrict__ blk, const int *__restrict__ idx, uint8_t *__restrict__ win,
	size_t tail, size_t cap, size_t stride)
{
	const size_t k = blockIdx.y;
	const uint4 *src = reinterpret_cast<const uint4 *>(blk + (size_t)idx[k] * stride);
	uint4 *dst = reinterpret_cast<uint4 *>(win + ((tail + k) % cap) * stride);
	for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < stride / 16; q += (size_t)gridDim.x * blockDim.x)
		dst[q] = src[q];
}
