// kern_skat.h -- the sums of the SKAT set test: per unit the weighted Gram matrix of its 2-bit rows
//     W[e,f] = sum_i mu2_i lut_e[code_ei] lut_f[code_fi]
// and per entry the 2K+1 dense sums of the score stage (c', e, s of DESIGN.md 3.1) against the columns of F, in FP64
// on the matrix cores.  Nothing of this is in the reference (it has no variance-component test).
// Part of libsaigehip.so (single translation unit: saigehip.hip).
#pragma once

// One 16 x 16 output tile: 16 entries of a unit (rows) against 16 entries of the same unit, or against 16 columns of F.
struct SkatTile {
	long long row_e0;   // first entry of the row tile (index into var_idx / lut)
	long long col_e0;   // first entry of the column tile, or (dense) the first column of F
	int nrow, ncol;     // rows / columns that exist (1..16); the others are computed as zeros and never read
	int dense;          // 1: the columns are columns of F and the rows carry no weight mu2 (F's columns have theirs)
	int pad;
};

typedef double skat_d4 __attribute__((ext_vector_type(4)));

// grid = (tiles, sample slabs of slab_dw dwords), block = one wave.  v_mfma_f64_16x16x4_f64: lane (v = lane & 15,
// h = lane >> 4) gives A[row v][k = h] and B[k = h][col v], one double each, and holds D[row h + 4 reg][col v] in
// reg = 0..3 (NOT the f32 16x16 map, whose rows are 4 h + reg).  The lane loads dword d of row entry v and of column
// entry v; in step t = 0..3 of the dword its k is sample 16 d + 4 t + h.  Samples >= N give A = B = 0.  The slab's
// tile goes to part[slab][tile][256] by plain stores: no atomics, and what a tile gets depends on its own entries and
// on N only (the slabs are cut by N), not on the other tiles of the launch.
__global__ void __launch_bounds__(64)
skat_gram_kernel(const uint8_t *__restrict__ packed, size_t bpv, int N, const int *__restrict__ var_idx,
	const double *__restrict__ lut, const double *__restrict__ F, int P, const SkatTile *__restrict__ tiles,
	size_t n_tiles, int slab_dw, double *__restrict__ part)
{
	const SkatTile t = tiles[blockIdx.x];
	const int lane = threadIdx.x, v = lane & 15, hq = lane >> 4;
	const int ndw = (N + 15) >> 4;
	const int d0 = blockIdx.y * slab_dw, d1 = min(ndw, d0 + slab_dw);
	double lr[4] = {0, 0, 0, 0}, lc[4] = {0, 0, 0, 0};
	const long long er = t.row_e0 + min(v, t.nrow - 1);
	const uint32_t *rrow = reinterpret_cast<const uint32_t *>(packed + (size_t)var_idx[er] * bpv);
	const uint32_t *crow = rrow;
	if (v < t.nrow) { lr[0] = lut[4 * er]; lr[1] = lut[4 * er + 1]; lr[2] = lut[4 * er + 2]; lr[3] = lut[4 * er + 3]; }
	const bool col_ok = v < t.ncol;
	if (!t.dense) {
		const long long ec = t.col_e0 + min(v, t.ncol - 1);
		crow = reinterpret_cast<const uint32_t *>(packed + (size_t)var_idx[ec] * bpv);
		if (col_ok) { lc[0] = lut[4 * ec]; lc[1] = lut[4 * ec + 1]; lc[2] = lut[4 * ec + 2]; lc[3] = lut[4 * ec + 3]; }
	}
	const int fcol = (int)t.col_e0 + v;               // dense: this lane's column of F
	skat_d4 acc = {0, 0, 0, 0};
	for (int d = d0; d < d1; d++) {
		const uint32_t wr = rrow[d], wc = crow[d];
#pragma unroll
		for (int s4 = 0; s4 < 4; s4++) {
			const int pos = 4 * s4 + hq, smp = 16 * d + pos;
			const bool ok = smp < N;
			double a = 0, b = 0;
			if (ok) {
				const double *f = F + (size_t)smp * P;
				a = sel4(lr, (wr >> (2 * pos)) & 3u);
				if (t.dense) b = col_ok ? f[fcol] : 0.0;
				else { a *= f[P - 1]; b = sel4(lc, (wc >> (2 * pos)) & 3u); }
			}
			acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
		}
	}
	double *o = part + ((size_t)blockIdx.y * n_tiles + blockIdx.x) * 256;
#pragma unroll
	for (int r = 0; r < 4; r++) o[(hq + 4 * r) * 16 + v] = acc[r];
}

// out[tile][256] = the slabs' partial tiles added in slab order.  One thread per element.
__global__ void __launch_bounds__(256)
skat_reduce_kernel(const double *__restrict__ part, size_t n_el, int nslab, double *__restrict__ out)
{
	const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n_el) return;
	double s = 0;
	for (int k = 0; k < nslab; k++) s += part[(size_t)k * n_el + i];
	out[i] = s;
}
