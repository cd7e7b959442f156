// kern_kmat.h -- products K B of an explicit symmetric matrix (sgx_kmat, host_kmat.h): CSR and dense.
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.
//
// In both storages the bits of (K b)_i depend on row i's stored entries and on b only: not on the number of
// columns of the call, on which columns share it, on the other rows or on earlier calls.  Every sum has a fixed
// order and nothing is accumulated with atomics.

#define KM_WAVE_ROW SGX_KMAT_WAVE_ROW   /* CSR rows with at least this many entries take the wave form */
#define KM_WCOLS 16           /* columns a wave of the CSR wave form / a dense launch carries at once */
#define KM_SLAB 1024          /* dense: columns of K per wave (a multiple of 16)                       */
#define KM_ROWS 32            /* dense: rows of K per wave (two 16-row MFMA tiles share the B fragment) */

// ---- CSR, short rows: one thread per (row, column of the call), the row's entries in ascending column order as
// one fma chain from 0.  An empty row gives 0.  Rows of the wave form are left to kmat_csr_wave_kernel.
__global__ void __launch_bounds__(256)
kmat_csr_thread_kernel(int n, const int64_t *__restrict__ rp, const int *__restrict__ col,
	const double *__restrict__ val, const double *__restrict__ B, size_t ldb, GrmCols cols,
	double *__restrict__ Out, size_t ldo)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const int64_t e0 = rp[i], e1 = rp[i + 1];
	if (e1 - e0 >= KM_WAVE_ROW) return;
	const size_t c = (size_t)cols.c[blockIdx.y];
	const double *__restrict__ b = B + c * ldb;
	double s = 0;
	for (int64_t e = e0; e < e1; e++) s = fma(val[e], b[col[e]], s);
	Out[c * ldo + i] = s;
}

// ---- CSR, long rows: one wave per row of the list.  Lane l takes entries l, l + 64, .. of the row as an fma chain
// from 0, then the 64 lane sums go through a fixed xor butterfly (32, 16, .., 1: both partners add the same two
// numbers, so every lane holds the same bits).  The wave carries up to KM_WCOLS columns of the call together: the
// row's col / val are fetched once per KM_WCOLS columns.
__global__ void __launch_bounds__(256)
kmat_csr_wave_kernel(int n_long, const int *__restrict__ long_rows, const int64_t *__restrict__ rp,
	const int *__restrict__ col, const double *__restrict__ val, const double *__restrict__ B, size_t ldb,
	GrmCols cols, double *__restrict__ Out, size_t ldo)
{
	const int lane = threadIdx.x & (WAVE - 1);
	const int r = blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x / WAVE);
	if (r >= n_long) return;                   // (the whole wave)
	const int i = long_rows[r];
	const int64_t e0 = rp[i], e1 = rp[i + 1];
	for (int y0 = 0; y0 < cols.n; y0 += KM_WCOLS) {
		const int ny = min(KM_WCOLS, cols.n - y0);
		double acc[KM_WCOLS];
#pragma unroll
		for (int y = 0; y < KM_WCOLS; y++) acc[y] = 0;
		for (int64_t e = e0 + lane; e < e1; e += WAVE) {
			const int cj = col[e];
			const double v = val[e];
#pragma unroll
			for (int y = 0; y < KM_WCOLS; y++)
				if (y < ny) acc[y] = fma(v, B[(size_t)cols.c[y0 + y] * ldb + cj], acc[y]);
		}
#pragma unroll
		for (int y = 0; y < KM_WCOLS; y++) {
			double s = acc[y];
#pragma unroll
			for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, WAVE);
			if (lane == 0 && y < ny) Out[(size_t)cols.c[y0 + y] * ldo + i] = s;
		}
	}
}

// ---- dense.  K is held as [rpad][ldd] doubles, ldd = n rounded up to 16 and rpad = n rounded up to KM_ROWS, the
// padding zero; the up to KM_WCOLS columns of a launch are packed into Bp [KM_WCOLS][ldd], zero beyond n and in
// the unused columns, so the product kernel below has no edge to check.
__global__ void __launch_bounds__(256)
kmat_dense_pack_kernel(int n, size_t ldd, const double *__restrict__ B, size_t ldb, GrmCols cols, double *__restrict__ Bp)
{
	const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
	const int y = blockIdx.y;
	if (i >= ldd) return;
	Bp[(size_t)y * ldd + i] = (y < cols.n && i < (size_t)n) ? B[(size_t)cols.c[y] * ldb + i] : 0.0;
}

typedef double km_d4 __attribute__((ext_vector_type(4)));

// grid = (rpad / KM_ROWS, slabs of KM_SLAB columns), block = one wave.  v_mfma_f64_16x16x4_f64: lane (v = lane & 15,
// h = lane >> 4) gives A[row v][k = h] and B[k = h][col v], one double each, and holds D[row h + 4 reg][col v] in
// reg = 0..3.  Per 16 columns of K the lane loads columns c0 + 4 h .. + 3 of its row (the four h lanes of a row read
// one 128-byte line) and the same four entries of packed column v; step t = 0..3 multiplies K's column c0 + 4 h + t.
// K is read once for the KM_WCOLS columns.  An output's terms are added in an order K's column index fixes, and
// the slab's sums go to part[slab][column][rpad] by plain stores.
__global__ void __launch_bounds__(WAVE)
kmat_dense_kernel(const double *__restrict__ K, size_t ldd, const double *__restrict__ Bp, int rpad, int na,
	double *__restrict__ part)
{
	const int lane = threadIdx.x, v = lane & 15, h = lane >> 4;
	const size_t r0 = (size_t)blockIdx.x * KM_ROWS;
	const size_t c_beg = (size_t)blockIdx.y * KM_SLAB, c_end = min(c_beg + (size_t)KM_SLAB, ldd);
	const double *__restrict__ k0 = K + (r0 + v) * ldd + 4 * h;
	const double *__restrict__ k1 = k0 + 16 * ldd;
	const double *__restrict__ bp = Bp + (size_t)v * ldd + 4 * h;
	km_d4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
	for (size_t c0 = c_beg; c0 < c_end; c0 += 16) {
		const km_d4 a0 = *(const km_d4 *)(k0 + c0), a1 = *(const km_d4 *)(k1 + c0), b = *(const km_d4 *)(bp + c0);
#pragma unroll
		for (int t = 0; t < 4; t++) {
			acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[t], b[t], acc0, 0, 0, 0);
			acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[t], b[t], acc1, 0, 0, 0);
		}
	}
	if (v >= na) return;
	double *o = part + ((size_t)blockIdx.y * KM_WCOLS + v) * rpad + r0 + h;
#pragma unroll
	for (int r = 0; r < 4; r++) { o[4 * r] = acc0[r]; o[16 + 4 * r] = acc1[r]; }
}

// Out[:, cols.c[y]] = the slabs' sums of packed column y added in slab order.  One thread per (row, column).
__global__ void __launch_bounds__(256)
kmat_dense_reduce_kernel(int n, int rpad, int nslab, const double *__restrict__ part, GrmCols cols,
	double *__restrict__ Out, size_t ldo)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	const int y = blockIdx.y;
	if (i >= n) return;
	double s = part[(size_t)y * rpad + i];
	for (int sl = 1; sl < nslab; sl++) s += part[((size_t)sl * KM_WCOLS + y) * rpad + i];
	Out[(size_t)cols.c[y] * ldo + i] = s;
}
