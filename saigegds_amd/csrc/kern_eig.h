// kern_eig.h -- eigenvalues of the SKAT-O matrices of a unit: one workgroup per symmetric matrix runs a
// cyclic two-sided Jacobi iteration in FP64 and writes the eigenvalues ascending.  No eigenvectors are kept.
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.
//
// The matrices.  Problem u is a symmetric m x m matrix A (row-major, only its upper triangle is read).  With r = A 1 and
// c = 1'A 1 (row sums left to right, then their sum top to bottom: a fixed order), matrix k of the problem is
//     k < n_rho:   B_ij = a^2 A_ij + a b (r_i + r_j) + b^2 c       a = sqrt(1 - rho) = ab[2k] and rho = ab[2k + 1] from the
//                                                                  host, b = (sqrt(1 - rho + m rho) - a) / m made here
//     k = n_rho:   W_ij = A_ij - r_i (r_j / c), i <= j
// formed once for i <= j and mirrored, so the working matrix is exactly symmetric.  a = 1, b = 0 (rho = 0) gives A's bits.
//
// The iteration.  Indices 0 .. mp - 1 (mp = m rounded up to even; the last one idle when m is odd) meet in mp - 1 steps
// of mp / 2 disjoint pairs, the round-robin of a tournament: pair 0 of step s is (s, mp - 1), pair k >= 1 is
// ((s + k) mod (mp - 1), (s - k) mod (mp - 1)).  A step has three phases with a barrier after each:
//   1. a thread per pair reads a_pp, a_qq, a_pq and makes the rotation (Rutishauser's formulas); the pair is skipped
//      where |a_pq| <= eps sqrt|a_pp| sqrt|a_qq|;
//   2. the rotations are applied to the columns p, q of every row;
//   3. then to the rows p, q of every column, except that the 2 x 2 block of the pair itself gets its closed form:
//      a_pp - t a_pq, a_qq + t a_pq and an exact 0 off the diagonal.
// A sweep is all steps.  The iteration ends after a sweep that skipped every pair or after EIG_MAX_SWEEPS sweeps -- a
// bound that holds whatever the entries are; the count of sweeps that rotated is reported.  Every operation commutes
// with a scaling of A by a power of two, and nothing depends on the other matrices of the launch or on the block size.
//
// Storage.  The working matrix has the leading dimension ld = m | 1: FP64 accesses along a column then fall on distinct
// LDS banks (an even stride puts lanes l and l + 16 or closer on one bank pair).  IN_LDS: it lives in dynamic LDS behind
// the 3 mp + 2 doubles of the vectors below (m <= EIG_LDS_M: 132 KiB + 3 KiB of the CU's 160 KiB); otherwise in this
// workgroup's slice of `scratch` (global memory; phase 2 runs with the pair on the lane and phase 3 with the column on
// the lane, so both read whole lines), the vectors still in LDS.  A matrix with a non-finite entry, in A or as formed,
// gets NaN eigenvalues and the count -1.

static const int EIG_MAX_SWEEPS = 30;
static const int EIG_LDS_M = 128;

__host__ __device__ static constexpr int eig_ld(int m) { return m | 1; }
// doubles of LDS in front of the working matrix: r / the diagonal [mp], then c, s, a_pp', a_qq' of the step's pairs
// [mp / 2] each, then c = 1'A 1 and two ints (non-finite flag, "this sweep rotated")
__host__ __device__ static constexpr int eig_aux(int m) { return 3 * ((m + 1) & ~1) + 2; }

__device__ static inline void eig_pair(int s, int k, int mp, int &p, int &q)
{
	if (k == 0) { p = s; q = mp - 1; return; }
	const int n1 = mp - 1;
	p = s + k; if (p >= n1) p -= n1;
	q = s - k; if (q < 0) q += n1;
}

template <bool IN_LDS>
__global__ __launch_bounds__(1024) void eig_jacobi_kernel(const double *__restrict__ A_all, const long long *__restrict__ a_off,
	const int *__restrict__ m_of, const long long *__restrict__ e_off, const int *__restrict__ plist, int nmat,
	const double *__restrict__ ab, double *__restrict__ scratch, size_t slice, double *__restrict__ eig, int *__restrict__ sweeps)
{
	extern __shared__ __attribute__((aligned(16))) double eig_smem[];
	const int tid = threadIdx.x, nt = blockDim.x;
	const int u = plist[blockIdx.x / nmat], k_mat = blockIdx.x % nmat;
	const int m = m_of[u], ld = eig_ld(m), mp = (m + 1) & ~1, np = mp >> 1;
	const double *A = A_all + a_off[u];
	double *out = eig + e_off[u] + (long long)k_mat * m;
	double *r = eig_smem, *rc = r + mp, *rs = rc + np, *rpp = rs + np, *rqq = rpp + np, *csum = rqq + np;
	int *flag = reinterpret_cast<int *>(csum + 1);                  // [0] non-finite, [1] this sweep rotated
	double *M = IN_LDS ? csum + 2 : scratch + (size_t)blockIdx.x * slice;

	if (tid < 2) flag[tid] = 0;
	__syncthreads();
	// A into the working storage (upper triangle mirrored), r, c
	for (int t = tid; t < m * m; t += nt) {
		const int i = t / m, j = t - i * m;
		const double v = A[i <= j ? t : j * m + i];
		if (!isfinite(v)) flag[0] = 1;
		M[i * ld + j] = v;
	}
	__syncthreads();
	for (int i = tid; i < m; i += nt) {
		double x = 0;
		for (int j = 0; j < m; j++) x += M[i * ld + j];
		r[i] = x;
	}
	__syncthreads();
	if (tid == 0) {
		double x = 0;
		for (int i = 0; i < m; i++) x += r[i];
		csum[0] = x;
	}
	__syncthreads();
	{
		const double c = csum[0];
		const bool isW = k_mat == nmat - 1;
		const double a = isW ? 0 : ab[2 * k_mat], rho = isW ? 0 : ab[2 * k_mat + 1];
		const double b = (sqrt((1 - rho) + m * rho) - a) / m;
		const double a2 = a * a, a1b = a * b, b2c = b * b * c;
		for (int t = tid; t < m * m; t += nt) {
			const int i = t / m, j = t - i * m;
			if (i > j) continue;
			const double x = M[i * ld + j];
			const double v = isW ? x - r[i] * (r[j] / c) : a2 * x + a1b * (r[i] + r[j]) + b2c;
			if (!isfinite(v)) flag[0] = 1;
			M[i * ld + j] = v;
			M[j * ld + i] = v;
		}
	}
	__syncthreads();
	if (flag[0]) {
		for (int i = tid; i < m; i += nt) out[i] = __longlong_as_double(0x7ff8000000000000LL);
		if (tid == 0) sweeps[(size_t)u * nmat + k_mat] = -1;
		return;
	}

	int n_sweep = 0;
	for (int sweep = 0; sweep < EIG_MAX_SWEEPS; sweep++) {
		for (int s = 0; s < mp - 1; s++) {
			// 1. the rotations of the step
			for (int k = tid; k < np; k += nt) {
				int p, q;
				eig_pair(s, k, mp, p, q);
				double c = 1, sn = 0;
				if (q < m && p < m) {
					const double app = M[p * ld + p], aqq = M[q * ld + q], apq = M[p * ld + q];
					if (!(fabs(apq) <= 2.220446049250313e-16 * (sqrt(fabs(app)) * sqrt(fabs(aqq))))) {
						const double tau = (aqq - app) / (2 * apq);
						const double t = (tau >= 0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1 + tau * tau));
						c = 1 / sqrt(1 + t * t);
						sn = t * c;
						rpp[k] = app - t * apq;
						rqq[k] = aqq + t * apq;
						flag[1] = 1;
						if (sn == 0) c = 2;                      // |tau| beyond a double's square: only the 2 x 2 block changes
					}
				}
				rc[k] = c; rs[k] = sn;                           // (c = 1, s = 0): skipped
			}
			__syncthreads();
			// 2. columns: (A_ip, A_iq) <- (c A_ip - s A_iq, s A_ip + c A_iq)
			for (int t = tid; t < np * m; t += nt) {
				const int i = t / np, k = t - i * np;
				const double c = rc[k], sn = rs[k];
				if (sn == 0) continue;
				int p, q;
				eig_pair(s, k, mp, p, q);
				const double x = M[i * ld + p], y = M[i * ld + q];
				M[i * ld + p] = c * x - sn * y;
				M[i * ld + q] = sn * x + c * y;
			}
			__syncthreads();
			// 3. rows: (A_pj, A_qj) <- (c A_pj - s A_qj, s A_pj + c A_qj); the pair's own block in closed form
			for (int t = tid; t < np * m; t += nt) {
				const int k = t / m, j = t - k * m;
				const double c = rc[k], sn = rs[k];
				if (c == 1 && sn == 0) continue;
				int p, q;
				eig_pair(s, k, mp, p, q);
				if (j == p) { M[p * ld + p] = rpp[k]; M[q * ld + p] = 0; continue; }
				if (j == q) { M[q * ld + q] = rqq[k]; M[p * ld + q] = 0; continue; }
				if (sn == 0) continue;
				const double x = M[p * ld + j], y = M[q * ld + j];
				M[p * ld + j] = c * x - sn * y;
				M[q * ld + j] = sn * x + c * y;
			}
			__syncthreads();
		}
		const int rotated = flag[1];
		__syncthreads();
		if (!rotated) break;
		n_sweep++;
		if (tid == 0) flag[1] = 0;
		__syncthreads();
	}

	// the diagonal, ascending (rank by value, ties by index; a NaN that an overflow on the way left ranks last)
	for (int i = tid; i < m; i += nt) r[i] = M[i * ld + i];
	__syncthreads();
	for (int i = tid; i < m; i += nt) {
		const double x = r[i];
		int rank = 0;
		for (int j = 0; j < m; j++) {
			const double y = r[j];
			const bool tie = y == x || (y != y && x != x);
			rank += (y < x || (x != x && y == y) || (tie && j < i)) ? 1 : 0;
		}
		out[rank] = x;
	}
	if (tid == 0) sweeps[(size_t)u * nmat + k_mat] = n_sweep;
}
