// kern_quant.h -- ingest: dosage rows as the file stores them -> 2-bit hard-call rows and the counts of the marker filter
// Part of libsaigehip.so (single translation unit: saigehip.hip).
#pragma once
#include <type_traits>

// A file without genotype/data gives the null-model fit its GRM markers from annotation/format/DS: the reference's
// saige_get_sparse (src/saige_fitnull.cpp:273-288) rounds every dosage to a hard call and builds the same 2-bit operator.
// Here the stored rows (kern_unpack.h: the five classes, unpack_real's two roundings) are rounded on the device:
//     v not finite                -> code 3 (missing)
//     r = round(v), C's round     -> code r if r is 0, 1 or 2, else 3
// round(v) (halves away from zero) is 0 exactly on (-0.5, 0.5), 1 on [0.5, 1.5) and 2 on [1.5, 2.5), so the code is
// decided by comparisons in double: no integer cast of an unbounded value (1e30f -> 3), -0.4 and -0.0 -> 0, a NaN fails
// every comparison -> 3.  The orientation stays the alt allele's, as for $dosage_alt rows.
__device__ __forceinline__ uint32_t quant_code(double v)
{
	return v > -0.5 && v < 0.5 ? 0u : v >= 0.5 && v < 1.5 ? 1u : v >= 1.5 && v < 2.5 ? 2u : 3u;
}

// What a thread gathers over its samples of one row: n_valid and allele_sum of the codes, ds_valid of the finite decoded
// dosages and their sum before rounding -- the integer classes as the exact int64 sum of the stored values (the row's
// ds_sum = that * scale + ds_valid * offset, quantize_finish), float32 as a double sum in sample order.
template <typename T> struct QuantAcc {
	using sum_t = std::conditional_t<unpack_traits<T>::real, double, long long>;
	int nv = 0, as = 0, dv = 0;
	sum_t s = 0;
	__device__ __forceinline__ uint32_t take(T x, double scale, double offset)
	{
		const double v = unpack_real(x, scale, offset);
		const bool fin = __builtin_isfinite(v);
		const uint32_t c = quant_code(v);
		nv += c != 3u; as += c != 3u ? (int)c : 0; dv += fin;
		if constexpr (unpack_traits<T>::real) s += fin ? v : 0.0;
		else s += fin ? (long long)x : 0ll;
		return c;
	}
};

// the 16 samples [g0, g0 + 16) of the row `in`, which starts `a` bytes behind a 16-byte line of its ADDRESS: the
// sizeof(T) lines that hold them (one more where a != 0), moved down by a bytes (a is the same for every thread of the
// row: wave-uniform selects, one v_alignbit per word).  The caller has checked that every line lies inside the row.
template <typename T>
__device__ __forceinline__ void quant_load16(const T *__restrict__ in, int g0, unsigned a, T e[16])
{
	constexpr int NW = 4 * (int)sizeof(T);                      // dwords of 16 samples
	const uint4 *line = reinterpret_cast<const uint4 *>(reinterpret_cast<const uint8_t *>(in + g0) - a);
	uint32_t w[NW + 4];
#pragma unroll
	for (int k = 0; k < NW / 4; k++) {
		const uint4 q = line[k];
		w[4 * k] = q.x; w[4 * k + 1] = q.y; w[4 * k + 2] = q.z; w[4 * k + 3] = q.w;
	}
	w[NW] = w[NW + 1] = w[NW + 2] = w[NW + 3] = 0;
	if (a) {
		const uint4 q = line[NW / 4];
		w[NW] = q.x; w[NW + 1] = q.y; w[NW + 2] = q.z; w[NW + 3] = q.w;
	}
	const unsigned q = a >> 2, r = (a & 3) * 8;
	uint32_t x[NW + 1];
#pragma unroll
	for (int i = 0; i <= NW; i++) x[i] = q == 0 ? w[i] : q == 1 ? w[i + 1] : q == 2 ? w[i + 2] : w[i + 3];
	union { uint32_t d[NW]; T e[16]; } u;
#pragma unroll
	for (int i = 0; i < NW; i++) u.d[i] = __builtin_amdgcn_alignbit(x[i + 1], x[i], r);
#pragma unroll
	for (int k = 0; k < 16; k++) e[k] = u.e[k];
}

// Row j of `out` (out_stride bytes, a multiple of 4; every dword of it is written, the codes of samples from n_samp on
// as 0: the padding of gds.pack_dosage_2bit) = the codes of row j of `raw` (stride n_file_samp values), and block
// partials of the row's four counts at [blockIdx.x * m + j] of p_nv / p_as / p_dv / p_s.  Memory-bound: sizeof(T)
// bytes in, a quarter of a byte out per sample.  A thread makes one output dword (16 samples) of the rows of its
// stride: grid.x = ceil(out_stride / 4 / 256) blocks cover a row exactly (no stride in x), grid.y strides over the
// rows.  The sample -> thread -> block assignment depends on n_samp alone, and the partials are added in a fixed order
// (a thread's samples in index order, the lanes of a wave by shuffles, the four waves and then the blocks in index
// order), so the counts -- the float32 sum too -- are the same bit for bit whatever the chunk, the row's address or
// the grid's second dimension.
//   sel == nullptr (n_file_samp == n_samp): 16-byte loads cut on the 16-byte lines of the row's ADDRESS (quant_load16;
//     n_file_samp * sizeof(T) need not be a multiple of 16).  Where a thread's lines are not wholly inside the row --
//     the row's first dword when it starts off a line, its last ones -- the values go element by element: nothing
//     outside the row is read.
//   sel: sample i = raw[sel[i]].  The thread's 16 indices are read once (four 16-byte loads, consecutive threads
//     consecutive 64 bytes) and kept for every row of its stride; the values are gathered.
template <typename T>
__global__ void __launch_bounds__(256)
quantize_rows(const T *__restrict__ raw, size_t n_file_samp, const int *__restrict__ sel, int n_samp, size_t m,
	double scale, double offset, uint8_t *__restrict__ out, size_t out_stride,
	int *__restrict__ p_nv, int *__restrict__ p_as, int *__restrict__ p_dv, typename QuantAcc<T>::sum_t *__restrict__ p_s)
{
	using sum_t = typename QuantAcc<T>::sum_t;
	__shared__ int l_nv[4], l_as[4], l_dv[4];
	__shared__ sum_t l_s[4];
	const int nd = (int)(out_stride / 4);
	const int dw = blockIdx.x * 256 + threadIdx.x;
	const bool live = dw < nd;
	const int g0 = live ? dw * 16 : 0;
	const int left = live ? min(16, n_samp - g0) : 0;           // samples of the dword that exist (<= 0: padding only)
	int s[16];
	if (sel) {
		if (left == 16) {
#pragma unroll
			for (int k = 0; k < 4; k++) {
				const int4 v = *reinterpret_cast<const int4 *>(sel + g0 + 4 * k);
				s[4 * k] = v.x; s[4 * k + 1] = v.y; s[4 * k + 2] = v.z; s[4 * k + 3] = v.w;
			}
		} else {
#pragma unroll
			for (int k = 0; k < 16; k++) s[k] = k < left ? sel[g0 + k] : -1;
		}
	}
	const size_t row_bytes = (size_t)n_samp * sizeof(T);        // (no selection: n_file_samp == n_samp)
	for (size_t j = blockIdx.y; j < m; j += gridDim.y) {
		const T *in = raw + j * n_file_samp;
		QuantAcc<T> acc;
		uint32_t word = 0;
		if (left > 0) {
			if (sel) {
#pragma unroll
				for (int k = 0; k < 16; k++)
					if (s[k] >= 0) word |= acc.take(in[(size_t)s[k]], scale, offset) << (2 * k);
			} else {
				const unsigned a = (unsigned)(reinterpret_cast<uintptr_t>(in) & 15);      // the same for every dword of the row
				const size_t b0 = (size_t)g0 * sizeof(T);             // the dword's first byte in the row
				if (left == 16 && b0 >= a && b0 - a + 16 * sizeof(T) + (a ? 16 : 0) <= row_bytes) {
					T e[16];
					quant_load16(in, g0, a, e);
#pragma unroll
					for (int k = 0; k < 16; k++) word |= acc.take(e[k], scale, offset) << (2 * k);
				} else {
					for (int k = 0; k < left; k++) word |= acc.take(in[g0 + k], scale, offset) << (2 * k);
				}
			}
		}
		if (live) reinterpret_cast<uint32_t *>(out + j * out_stride)[dw] = word;
		// the block's partial sums of row j
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) {
			acc.nv += __shfl_down(acc.nv, o);
			acc.as += __shfl_down(acc.as, o);
			acc.dv += __shfl_down(acc.dv, o);
			acc.s += __shfl_down(acc.s, o);
		}
		const int wv = threadIdx.x >> 6;
		if ((threadIdx.x & 63) == 0) { l_nv[wv] = acc.nv; l_as[wv] = acc.as; l_dv[wv] = acc.dv; l_s[wv] = acc.s; }
		__syncthreads();
		if (threadIdx.x == 0) {
			const size_t p = (size_t)blockIdx.x * m + j;
			p_nv[p] = l_nv[0] + l_nv[1] + l_nv[2] + l_nv[3];
			p_as[p] = l_as[0] + l_as[1] + l_as[2] + l_as[3];
			p_dv[p] = l_dv[0] + l_dv[1] + l_dv[2] + l_dv[3];
			p_s[p] = ((l_s[0] + l_s[1]) + l_s[2]) + l_s[3];
		}
		__syncthreads();
	}
}

// The counts of row j = the sums of its nbx block partials in block order (a thread a row; the partials of a block lie
// row after row, so the reads coalesce).  S = long long: ds_sum = (double)sum * scale + ds_valid * offset, each
// operation rounded on its own; S = double: the sum itself.
template <typename S>
__global__ void __launch_bounds__(256)
quantize_finish(const int *__restrict__ p_nv, const int *__restrict__ p_as, const int *__restrict__ p_dv,
	const S *__restrict__ p_s, unsigned nbx, size_t m, double scale, double offset,
	int *__restrict__ n_valid, int *__restrict__ allele_sum, int *__restrict__ ds_valid, double *__restrict__ ds_sum)
{
#pragma clang fp contract(off)
	for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (size_t)gridDim.x * blockDim.x) {
		int nv = 0, as = 0, dv = 0;
		S s = 0;
		for (unsigned b = 0; b < nbx; b++) {
			const size_t p = (size_t)b * m + j;
			nv += p_nv[p]; as += p_as[p]; dv += p_dv[p]; s += p_s[p];
		}
		n_valid[j] = nv; allele_sum[j] = as; ds_valid[j] = dv;
		if constexpr (std::is_same<S, double>::value) ds_sum[j] = s;
		else {
			const double a = (double)s * scale, b = (double)dv * offset;
			ds_sum[j] = a + b;
		}
	}
}
