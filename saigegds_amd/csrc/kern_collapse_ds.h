// kern_collapse_ds.h -- the pseudo-variant of a group of resident dosage rows: per sample the largest
// minor-allele dosage over the group's rows, as one more row of the block in the block's own form (u8, or f64 with
// non-finite = missing).  Part of libsaigehip.so (single translation unit: saigehip.hip).
#pragma once

// ---------------------------------------------------------------------------
// A workgroup takes one slab of one group: COLLAPSE_DS_BLOCK threads with 16 u8 samples (one 16-byte piece) or 4 f64
// samples (two pieces) each, and loops over the group's entries; the workgroups loop over the (group, slab) pairs.
//   Per sample, from top = +0.0 (u8: 0):
//     x = row_e[i];   v = missing(x) ? 0 : (flip_e ? 2 - x : x);   if (v > top) top = v
//   u8: 0xFF is missing and 2 - x is integer arithmetic, so a value above 2 in a flipped row is negative and never
//   enters; the result is at most 254 and never the missing code.  f64: non-finite is missing, 2 - x is one rounded
//   subtraction, and the strict comparison keeps negative values, -0.0 and NaN out -- a maximum of values that are all
//   >= +0.0 in the order of the numbers, so neither the order of the entries nor an entry taken twice changes a bit.
//   A round loads UNROLL entries' pieces before it looks at the first (8 KiB a wave in flight); the round past the
//   group's end takes the last entry again instead of branching around its loads.  var_idx[e] and flip[e] are the
//   same for the whole workgroup: scalar loads.
//   Loads and stores follow ds_load's rule (kern_burden_ds.h): 16-byte accesses only where every row starts on a
//   multiple of 16 bytes (N * sizeof(T) % 16 == 0; the block's base is 256-byte aligned) and the thread's samples all
//   lie inside the row, element accesses otherwise; nothing at or beyond sample N is read or written.
// The result goes to row out_row0 + g of the same buffer, which no group of the call reads (the host checks every
// index against out_row0).  A group's row depends on its entries' rows and flips only: no atomics, no LDS, no
// scratch, and the grid only decides which workgroup takes which pair.

#define COLLAPSE_DS_BLOCK 256
#define COLLAPSE_DS_PIECE 16                  /* bytes of a vector load */
template <typename T> struct CollapseDs;
template <> struct CollapseDs<uint8_t> { static constexpr int SPT = 16, UNROLL = 8; };   // one piece a thread, 8 entries a round
template <> struct CollapseDs<double> { static constexpr int SPT = 4, UNROLL = 4; };     // two pieces a thread, 4 entries a round
#define COLLAPSE_DS_SLAB(T) (COLLAPSE_DS_BLOCK * CollapseDs<T>::SPT)   /* samples of a row a workgroup takes: 4096 u8, 1024 f64 */

__device__ __forceinline__ void collapse_ds_max(uint8_t x, bool fl, uint8_t &top)
{
	const int v = x == 0xFF ? 0 : (fl ? 2 - (int)x : (int)x);
	if (v > (int)top) top = (uint8_t)v;
}
__device__ __forceinline__ void collapse_ds_max(double x, bool fl, double &top)
{
	const double v = isfinite(x) ? (fl ? __dsub_rn(2.0, x) : x) : 0.0;
	if (v > top) top = v;
}

template <typename T>
__global__ void __launch_bounds__(COLLAPSE_DS_BLOCK)
collapse_ds_kernel(T *rows, int N, size_t out_row0, size_t n_groups, const int64_t *__restrict__ grp_ptr,
	const int32_t *__restrict__ var_idx, const uint8_t *__restrict__ flip)
{
	constexpr int SPT = CollapseDs<T>::SPT, UNROLL = CollapseDs<T>::UNROLL;
	static_assert(SPT * sizeof(T) % COLLAPSE_DS_PIECE == 0, "whole pieces a thread");
	const size_t nslab = ((size_t)N + COLLAPSE_DS_SLAB(T) - 1) / COLLAPSE_DS_SLAB(T), total = n_groups * nslab;
	const bool vec = ((size_t)N * sizeof(T)) % COLLAPSE_DS_PIECE == 0;     // every row starts on a multiple of a piece
	for (size_t b = blockIdx.x; b < total; b += gridDim.x) {
		const size_t g = b / nslab, s0 = ((b % nslab) * COLLAPSE_DS_BLOCK + threadIdx.x) * SPT;   // the thread's first sample
		if (s0 >= (size_t)N) continue;
		const int i0 = (int)s0;
		const bool whole = (size_t)N - s0 >= (size_t)SPT;       // (not i0 + SPT <= N: N may be close to INT_MAX)
		const int64_t e_end = grp_ptr[g + 1];
		T top[SPT];
#pragma unroll
		for (int s = 0; s < SPT; s++) top[s] = T(0);
		for (int64_t e0 = grp_ptr[g]; e0 < e_end; e0 += UNROLL) {
			T v[UNROLL][SPT];
			bool fl[UNROLL];
#pragma unroll
			for (int u = 0; u < UNROLL; u++) {                  // the round's loads first
				const int64_t e = e0 + u < e_end ? e0 + u : e_end - 1;
				const T *row = rows + (size_t)var_idx[e] * (size_t)N;
				if (whole) ds_load<T, SPT>(row, i0, N, vec, v[u]);
				else {
#pragma unroll
					for (int s = 0; s < SPT; s++) v[u][s] = s0 + s < (size_t)N ? row[s0 + s] : T(0);
				}
				fl[u] = flip[e] != 0;
			}
#pragma unroll
			for (int u = 0; u < UNROLL; u++)
#pragma unroll
				for (int s = 0; s < SPT; s++) collapse_ds_max(v[u][s], fl[u], top[s]);
		}
		T *o = rows + (out_row0 + g) * (size_t)N + s0;
		if (vec && whole) {
#pragma unroll
			for (int l = 0; l < SPT * (int)sizeof(T) / COLLAPSE_DS_PIECE; l++) {
				uint4 q;
				memcpy(&q, reinterpret_cast<const uint8_t *>(top) + l * COLLAPSE_DS_PIECE, COLLAPSE_DS_PIECE);
				*reinterpret_cast<uint4 *>(reinterpret_cast<uint8_t *>(o) + l * COLLAPSE_DS_PIECE) = q;
			}
		} else {
#pragma unroll
			for (int s = 0; s < SPT; s++)
				if (s0 + s < (size_t)N) o[s] = top[s];
		}
	}
}
