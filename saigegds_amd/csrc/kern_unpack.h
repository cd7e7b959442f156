// kern_unpack.h -- ingest: packed-real dosage rows as the file stores them -> the float64 rows of the dosage kernels
// Part of libsaigehip.so (single translation unit: saigehip.hip).
#pragma once

// A SeqArray file keeps imputed dosages (annotation/format/DS/data) as dPackedReal8[U] / dPackedReal16[U]: 1- or
// 2-byte integers with the node's `scale` and `offset`, the all-ones (unsigned) or most negative (signed) code =
// missing; or as dFloat32.  value = raw * scale + offset in two roundings, the product and then the sum -- what
// saigegds_amd/gds.py computes on the host (numpy: a multiply, then an add) -- so the decoded rows equal the host's
// bit for bit.  float rows are widened as they are (NaN / Inf stay, scale and offset do not apply).
template <typename T> struct unpack_traits;
template <> struct unpack_traits<uint8_t>  { static constexpr bool real = false; static constexpr int miss = 0xFF; };
template <> struct unpack_traits<int8_t>   { static constexpr bool real = false; static constexpr int miss = -128; };
template <> struct unpack_traits<uint16_t> { static constexpr bool real = false; static constexpr int miss = 0xFFFF; };
template <> struct unpack_traits<int16_t>  { static constexpr bool real = false; static constexpr int miss = -32768; };
template <> struct unpack_traits<float>    { static constexpr bool real = true;  static constexpr int miss = 0; };

template <typename T>
__device__ __forceinline__ double unpack_real(T v, double scale, double offset)
{
	// __dadd_rn(__dmul_rn(v, scale), offset) in meaning; written out under contract(off) because the two intrinsics
	// are a plain `*` and `+` to the compiler, which fuses them into one v_fma_f64 (one rounding) under hipcc's default
#pragma clang fp contract(off)
	if constexpr (unpack_traits<T>::real) return (double)v;
	else {
		const double prod = (double)v * scale;
		return (int)v == unpack_traits<T>::miss ? (double)NAN : prod + offset;
	}
}

// Row r of `out` (n_samp doubles, stride n_samp) = the decoded samples of row r of `raw` (stride n_file_samp).
// Memory-bound: sizeof(T) bytes in, 8 bytes out per sample.  grid.x walks a row, grid.y strides over the rows.
//   sel == nullptr: the first n_samp samples of the row.  A thread takes one 16-byte load (16 / sizeof(T) samples)
//     and stores the doubles as 16-byte pairs.  n_file_samp * sizeof(T) need not be a multiple of 16, so the loads
//     are cut on the 16-byte lines of the row's ADDRESS (the first and last line of a row go element by element,
//     nothing outside the row is read), and the pairs start one double later where the line's first double sits on
//     an odd multiple of 8 bytes -- both per row, wave-uniform.
//   sel: sample i = raw[sel[i]]: sel is read coalesced (once per thread, for every row of the thread's stride), the
//     raw values are gathered, the doubles are written coalesced.
template <typename T>
__global__ void __launch_bounds__(256)
unpack_real_rows(const T *__restrict__ raw, size_t n_file_samp, const int *__restrict__ sel, int n_samp,
	size_t n_rows, double scale, double offset, double *__restrict__ out_f64)
{
	if (sel) {
		for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_samp; i += gridDim.x * blockDim.x) {
			const size_t s = (size_t)sel[i];
			for (size_t r = blockIdx.y; r < n_rows; r += gridDim.y)
				out_f64[r * (size_t)n_samp + i] = unpack_real(raw[r * n_file_samp + s], scale, offset);
		}
		return;
	}
	constexpr int VE = 16 / (int)sizeof(T);                     // samples of one 16-byte load
	for (size_t r = blockIdx.y; r < n_rows; r += gridDim.y) {
		const T *in = raw + r * n_file_samp;
		double *o = out_f64 + r * (size_t)n_samp;
		const int a0 = (int)((reinterpret_cast<uintptr_t>(in) & 15) / sizeof(T));    // samples the row starts behind a line's start
		const int nvec = (a0 + n_samp + VE - 1) / VE;
		for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < nvec; v += gridDim.x * blockDim.x) {
			const int g0 = v * VE - a0;                         // the line's first sample (a0 is the same for every line of the row)
			if (g0 < 0 || g0 + VE > n_samp) {                   // the row's first / last line
				for (int k = max(g0, 0); k < min(g0 + VE, n_samp); k++) o[k] = unpack_real(in[k], scale, offset);
				continue;
			}
			union { uint4 q; T e[VE]; } u;
			u.q = *reinterpret_cast<const uint4 *>(in + g0);
			double d[VE];
#pragma unroll
			for (int k = 0; k < VE; k++) d[k] = unpack_real(u.e[k], scale, offset);
			double *p = o + g0;
			if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
#pragma unroll
				for (int k = 0; k < VE; k += 2) *reinterpret_cast<double2 *>(p + k) = make_double2(d[k], d[k + 1]);
			} else {
				p[0] = d[0];
#pragma unroll
				for (int k = 1; k + 1 < VE; k += 2) *reinterpret_cast<double2 *>(p + k) = make_double2(d[k], d[k + 1]);
				p[VE - 1] = d[VE - 1];
			}
		}
	}
}
