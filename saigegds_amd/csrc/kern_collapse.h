// kern_collapse.h -- the pseudo-variant of a group of 2-bit rows: per sample the largest minor-allele
// dosage over the group's rows, as a 2-bit row of its own, and the numbers of samples with dosage 1 and with dosage 2
// Part of libsaigehip.so (single translation unit: saigehip.hip).
#pragma once

// ---------------------------------------------------------------------------
// A workgroup takes one slab of one group: COLLAPSE_SLAB bytes of the row (16 384 samples), a 16-byte piece a thread,
// and loops over the group's entries; the workgroups loop over the (group, slab) pairs.  Integer work only.
//   Per word, with c0 / c1 the low / high bit of every code (code 3 = missing counts as dosage 0):
//     dosage 2:  hi = c1 & ~c0,  flipped row (dosage = 2 - code): hi = ~c1 & ~c0   -> (c1 ^ flipmask) & ~c0
//     dosage 1:  lo = c0 & ~c1   either way
//   The maximum of fields that are never 3: HI |= hi, LO |= lo over the entries, and LO &= ~HI once at the end -- an
//   OR, so neither the order of the entries nor an entry taken twice changes a bit.  A round loads COLLAPSE_UNROLL
//   pieces before it looks at the first (8 KiB a wave in flight); the round past the group's end takes the last entry
//   again instead of branching around its loads.
//   The fields at and beyond N are cleared in the result (a flipped row makes 2s of zero padding), the pieces beyond
//   ceil(N / 4) bytes come out as zeros up to the row stride.
//   counts[2g], counts[2g + 1]: popcounts of LO and HI, summed over the wave and added by one integer atomic a wave to
//   words the host zeroed before the launch: integer sums, the same bits in any order.
// A group's row and counts depend on its entries' rows and flips only: nothing here knows another group, and the grid
// only decides which workgroup takes which pair.

#define COLLAPSE_BLOCK 256
#define COLLAPSE_SLAB (COLLAPSE_BLOCK * 16)   /* bytes of a row a workgroup takes: 16 384 samples */
#define COLLAPSE_UNROLL 8                     /* 16-byte pieces a thread loads before it looks at the first */

__global__ void __launch_bounds__(COLLAPSE_BLOCK)
collapse_kernel(const uint8_t *__restrict__ rows, size_t bpv, int N, size_t n_groups, const int64_t *__restrict__ grp_ptr,
	const int32_t *__restrict__ var_idx, const uint8_t *__restrict__ flip, uint8_t *__restrict__ out_rows,
	int32_t *__restrict__ counts)
{
	const size_t nslab = (bpv + COLLAPSE_SLAB - 1) / COLLAPSE_SLAB, total = n_groups * nslab;
	const int lane = threadIdx.x & (WAVE - 1);
	for (size_t b = blockIdx.x; b < total; b += gridDim.x) {
		const size_t g = b / nslab, p = (b % nslab) * COLLAPSE_BLOCK + threadIdx.x;   // the thread's piece of the row
		const bool active = p * 16 < bpv;                  // (bpv is a multiple of 16: an active piece lies inside every row)
		const int64_t e_end = grp_ptr[g + 1];
		uint32_t HI[4] = {0, 0, 0, 0}, LO[4] = {0, 0, 0, 0};
		if (active) {
			const uint8_t *col = rows + p * 16;
			for (int64_t e0 = grp_ptr[g]; e0 < e_end; e0 += COLLAPSE_UNROLL) {
				uint4 q[COLLAPSE_UNROLL];
				uint32_t fm[COLLAPSE_UNROLL];
#pragma unroll
				for (int u = 0; u < COLLAPSE_UNROLL; u++) {    // the round's loads first; entry and flip are wave-uniform
					const int64_t e = e0 + u < e_end ? e0 + u : e_end - 1;
					q[u] = *reinterpret_cast<const uint4 *>(col + (size_t)var_idx[e] * bpv);
					fm[u] = flip[e] ? LO_MASK : 0u;
				}
#pragma unroll
				for (int u = 0; u < COLLAPSE_UNROLL; u++) {
					const uint32_t wd[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
#pragma unroll
					for (int d = 0; d < 4; d++) {
						const uint32_t c0 = wd[d] & LO_MASK, c1 = (wd[d] >> 1) & LO_MASK;
						HI[d] |= (c1 ^ fm[u]) & ~c0;
						LO[d] |= c0 & ~c1;
					}
				}
			}
		}
		int n1 = 0, n2 = 0;
		if (active) {
			uint32_t o[4];
#pragma unroll
			for (int d = 0; d < 4; d++) {
				// samples of this word: 64 p + 16 d ..; beyond N nothing is kept (p * 64 fits: p < bpv / 16, N <= 4 bpv)
				const long long left = (long long)N - ((long long)p * 64 + d * 16);
				const uint32_t keep = keep_mask(left > 16 ? 16 : (int)(left < 0 ? 0 : left));
				const uint32_t hi = HI[d] & keep, lo = LO[d] & ~HI[d] & keep;
				n1 += __popc(lo);
				n2 += __popc(hi);
				o[d] = lo | (hi << 1);
			}
			*reinterpret_cast<uint4 *>(out_rows + g * bpv + p * 16) = make_uint4(o[0], o[1], o[2], o[3]);
		}
		n1 = wave_sum_i(n1);
		n2 = wave_sum_i(n2);
		if (lane == 0) {
			if (n1) atomicAdd(&counts[2 * g], n1);
			if (n2) atomicAdd(&counts[2 * g + 1], n2);
		}
	}
}
