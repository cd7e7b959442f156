// kern_burden_ds.h -- aggregate tests on dosage rows (u8, or f64 with NaN = missing): per-variant counts and
// the weighted collapse of the variants of a unit into several burden rows at once
// (ds_mat_mafmac / ds_mat_burden, reference src/saige_main.cpp:485-610, INTSXP and REALSXP branches next to RAW).
// Part of libsaigehip.so (single translation unit: saigehip.hip).
#pragma once

__host__ __device__ inline bool ds_ok(uint8_t v) { return v != 0xFF; }
__host__ __device__ inline bool ds_ok(double v) { return isfinite(v); }

// What one dosage adds to the `int sum` of ds_mat_burden.  The reference declares that sum `int` in every
// branch, the REALSXP one included (:589-591), so `sum += s[j]` truncates after every addition: for finite
// dosages in [0, 2] whose fractional part is below 1 - 2^-20 the result is the sum of the floors, which does
// not depend on the order of the samples.  The mean used for imputation and the flip decision of real-valued
// dosages come from this sum; maf, mac and the weights come from the plain double sum of ds_mat_mafmac.
// Integer dosages (u8, i32) are their own floor.
__host__ __device__ inline long long ds_trunc_term(double v) { return (long long)floor(v); }
__host__ __device__ inline long long ds_trunc_term(uint8_t v) { return v; }

// Per-variant counts of resident dosage rows: n_valid, the plain sum (double; an exact integer for u8 / i32
// rows) and the truncated sum of ds_trunc_term.  One workgroup per variant (the dosage twin of geno_stats_kernel).
template <typename T>
__global__ void __launch_bounds__(256)
ds_stats_kernel(const T *__restrict__ rows, int N, int *__restrict__ n_valid, double *__restrict__ sum,
	long long *__restrict__ sum_trunc)
{
	__shared__ int sh_n[4];
	__shared__ double sh_s[4];
	__shared__ long long sh_t[4];
	const T *row = rows + (size_t)blockIdx.x * (size_t)N;
	int nv = 0; double sd = 0, lo = 0; long long st = 0;
	for (int i = threadIdx.x; i < N; i += 256) {
		const T v = row[i];
		if (ds_ok(v)) {
			nv++; st += ds_trunc_term(v);
			if (sizeof(T) > 1) {                     // compensated: a thread's 1 700 terms at N = 430 000 lose nothing
				const double x = (double)v, t = __dadd_rn(sd, x), z = __dsub_rn(t, sd);
				lo = __dadd_rn(lo, __dadd_rn(__dsub_rn(sd, __dsub_rn(t, z)), __dsub_rn(x, z)));
				sd = t;
			}
		}
	}
	nv = wave_sum_i(nv);
	if (sizeof(T) > 1) sd = wave_sum(__dadd_rn(sd, lo));
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) st += __shfl_xor(st, o, WAVE);
	const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
	if (lane == 0) { sh_n[wid] = nv; sh_s[wid] = sd; sh_t[wid] = st; }
	__syncthreads();
	if (threadIdx.x == 0) {
		const long long t = sh_t[0] + sh_t[1] + sh_t[2] + sh_t[3];
		n_valid[blockIdx.x] = sh_n[0] + sh_n[1] + sh_n[2] + sh_n[3];
		sum_trunc[blockIdx.x] = t;
		sum[blockIdx.x] = sizeof(T) > 1 ? (sh_s[0] + sh_s[1]) + (sh_s[2] + sh_s[3]) : (double)t;
	}
}

// SPT consecutive dosages of a row from sample i0 on.  vec: the row starts on a multiple of the load width
// (wave-uniform); 16-byte loads then, element loads otherwise and in the row's tail.
template <typename T, int SPT>
__device__ __forceinline__ void ds_load(const T *__restrict__ row, int i0, int N, bool vec, T (&v)[SPT])
{
	constexpr int LB = SPT * (int)sizeof(T) < 16 ? SPT * (int)sizeof(T) : 16;     // bytes per load
	constexpr int NL = SPT * (int)sizeof(T) / LB, EL = LB / (int)sizeof(T);
	if (vec && i0 + SPT <= N) {
#pragma unroll
		for (int l = 0; l < NL; l++) {
			if constexpr (LB == 16) {
				const uint4 q = *reinterpret_cast<const uint4 *>(row + i0 + l * EL);
				memcpy(&v[l * EL], &q, 16);
			} else if constexpr (LB == 8) {
				const uint2 q = *reinterpret_cast<const uint2 *>(row + i0 + l * EL);
				memcpy(&v[l * EL], &q, 8);
			} else {
				const uint32_t q = *reinterpret_cast<const uint32_t *>(row + i0 + l * EL);
				memcpy(&v[l * EL], &q, 4);
			}
		}
	} else {
#pragma unroll
		for (int s = 0; s < SPT; s++) v[s] = (i0 + s < N) ? row[i0 + s] : T(0);
	}
}

// Burden rows of group g = blockIdx.y, columns [c0, c0 + nc) of its n_cols: for sample i
//     out[(g * n_cols + c) * N + i] = sum over the entries e of the group, in order, with finite w[e][c], of
//         ok(x) ? t(x) * w[e][c] : mw[e][c],      x = rows[var_idx[e]][i],   t(x) = flip[e] ? 2 - x : x
// -- ds_mat_burden's `p[j] += ...`: the product rounded, then added (no contraction to an FMA), so a row of
// hard calls equals burden_collapse_kernel's row of the packed form of the same data bit for bit.  2 - x is
// integer arithmetic for u8 rows, as in the RAW / INTSXP branches.  Each dosage is read once and feeds all
// NC columns; a thread owns SPT consecutive samples with NC * SPT <= 32 accumulators in registers:
//     f64 rows: SPT = 4 (two 16-byte loads);   u8 rows: SPT = 16 / 16 / 8 / 4 for NC = 1 / 2 / 4 / 8 (the
//     collapsed rows written are 8 * NC bytes per byte read, so u8 traffic is the output's, not the load's).
// w and mw are the same for every lane: scalar loads.  grid = (ceil(N / (256 * SPT)), n_groups), block = 256.
template <typename T, int NC, int SPT>
__global__ void __launch_bounds__(256)
burden_collapse_ds_kernel(const T *__restrict__ rows, int N, const long long *__restrict__ grp_ptr,
	const int *__restrict__ var_idx, const uint8_t *__restrict__ flip, int n_cols, int c0, int nc,
	const double *__restrict__ w, const double *__restrict__ mw, double *__restrict__ out)
{
	static_assert(NC * SPT <= 32, "accumulators per thread");
	const int i0 = (blockIdx.x * 256 + threadIdx.x) * SPT;
	if (i0 >= N) return;
	const size_t g = blockIdx.y;
	constexpr int LB = SPT * (int)sizeof(T) < 16 ? SPT * (int)sizeof(T) : 16;
	const bool vec = ((size_t)N * sizeof(T)) % LB == 0;      // every row then starts on a multiple of LB (the base is 256-byte aligned)
	double acc[NC][SPT];
#pragma unroll
	for (int c = 0; c < NC; c++)
#pragma unroll
		for (int s = 0; s < SPT; s++) acc[c][s] = 0;
	for (long long e = grp_ptr[g]; e < grp_ptr[g + 1]; e++) {
		T v[SPT];
		ds_load<T, SPT>(rows + (size_t)var_idx[e] * (size_t)N, i0, N, vec, v);
		const bool fl = flip[e] != 0;
		double t[SPT]; bool ok[SPT];
#pragma unroll
		for (int s = 0; s < SPT; s++) {
			ok[s] = ds_ok(v[s]);
			if constexpr (sizeof(T) == 1) t[s] = (double)(fl ? 2 - (int)v[s] : (int)v[s]);
			else t[s] = fl ? __dsub_rn(2.0, (double)v[s]) : (double)v[s];
		}
#pragma unroll
		for (int c = 0; c < NC; c++) {
			if (c < nc) {
				const double wc = w[e * n_cols + c0 + c];
				if (isfinite(wc)) {
					const double mc = mw[e * n_cols + c0 + c];
#pragma unroll
					for (int s = 0; s < SPT; s++)
						acc[c][s] = __dadd_rn(acc[c][s], ok[s] ? __dmul_rn(t[s], wc) : mc);
				}
			}
		}
	}
#pragma unroll
	for (int c = 0; c < NC; c++) {
		if (c < nc) {
			double *o = out + (g * (size_t)n_cols + (size_t)(c0 + c)) * (size_t)N + i0;
#pragma unroll
			for (int s = 0; s < SPT; s++)
				if (i0 + s < N) o[s] = acc[c][s];
		}
	}
}
