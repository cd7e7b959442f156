// pca_check.cpp -- the two dense host routines of sgx_grm_pca (saigegds_amd/csrc/host_pca.h: Cholesky with the inverse
// factor, cyclic Jacobi) on their own, without HIP, against matrices whose answers are known in closed form: built and
// run by tests/test_pca_host.py with the host compiler under -fsanitize=address,undefined.  Every matrix lives in a heap
// buffer of exactly its size.
#define PCA_HOST_ONLY
#include "host_pca.h"
#include <stdio.h>
#include <stdlib.h>

static int g_fail = 0, g_done = 0;
#define CHECK(c) do { g_done++; if (!(c)) { g_fail++; fprintf(stderr, "line %d: %s\n", __LINE__, #c); } } while (0)

static const double PI = 3.14159265358979323846;

// |V' V - I| and |V diag(theta) V' - H0| (entrywise maxima)
static void eig_errors(int L, const std::vector<double> &H0, const std::vector<double> &V, const std::vector<double> &th,
	double *orth, double *recon)
{
	*orth = *recon = 0;
	for (int a = 0; a < L; a++)
		for (int b = 0; b < L; b++) {
			double o = 0, r = 0;
			for (int k = 0; k < L; k++) { o += V[k * L + a] * V[k * L + b]; r += V[a * L + k] * th[k] * V[b * L + k]; }
			*orth = std::max(*orth, std::fabs(o - (a == b)));
			*recon = std::max(*recon, std::fabs(r - H0[a * L + b]));
		}
}

static void jacobi_case(int L, const std::vector<double> &H0, const std::vector<double> &want /* descending */, double scale)
{
	std::vector<double> H(H0), V((size_t)L * L), th(L);
	pca_jacobi(L, H.data(), V.data(), th.data());
	double orth, recon;
	eig_errors(L, H0, V, th, &orth, &recon);
	CHECK(orth <= 8 * L * 0x1p-53);
	CHECK(recon <= 16 * L * 0x1p-53 * scale);
	for (int c = 0; c < L; c++) {
		CHECK(std::fabs(th[c] - want[c]) <= 16 * L * 0x1p-53 * scale);
		if (c) CHECK(th[c] <= th[c - 1]);
	}
}

int main()
{
	// ---- Jacobi
	for (int L : {1, 2, 3, 16, 17, 44, 64}) {
		// the second-difference matrix tridiag(-1, 2, -1): eigenvalues 2 - 2 cos(k pi / (L + 1)), k = 1 .. L
		std::vector<double> H((size_t)L * L, 0.0), want(L);
		for (int j = 0; j < L; j++) {
			H[j * L + j] = 2;
			if (j) H[j * L + j - 1] = H[(j - 1) * L + j] = -1;
		}
		for (int k = 0; k < L; k++) want[k] = 2 - 2 * std::cos((L - k) * PI / (L + 1));
		jacobi_case(L, H, want, 4.0);
		// a I + b 11': one eigenvalue a + b L, the others a (a repeated eigenvalue)
		std::vector<double> J((size_t)L * L, 0.5), wj(L, 3.0);
		for (int j = 0; j < L; j++) J[j * L + j] = 3.5;
		wj[0] = 3.0 + 0.5 * L;
		jacobi_case(L, J, wj, wj[0]);
		// a diagonal matrix out of order, with a zero and a negative entry: sorted, nothing rotated
		std::vector<double> D((size_t)L * L, 0.0), wd(L);
		for (int j = 0; j < L; j++) D[j * L + j] = wd[j] = (double)((j * 7) % L) - 1.0;
		std::sort(wd.begin(), wd.end(), [](double a, double b) { return a > b; });
		jacobi_case(L, D, wd, (double)L);
	}
	// the zero matrix: theta 0, V = I
	{
		std::vector<double> H(9, 0.0), V(9), th(3);
		pca_jacobi(3, H.data(), V.data(), th.data());
		CHECK(th[0] == 0 && th[1] == 0 && th[2] == 0 && V[0] == 1 && V[4] == 1 && V[8] == 1 && V[1] == 0);
	}

	// ---- Cholesky and the inverse factor
	for (int L : {1, 2, 5, 16, 33, 64}) {
		// C_ij = min(i, j) + 1 = R'R with R the upper triangle of ones; R^-1 has 1 on the diagonal, -1 above it
		std::vector<double> C((size_t)L * L), R((size_t)L * L), Ti((size_t)L * L);
		for (int i = 0; i < L; i++)
			for (int j = 0; j < L; j++) C[i * L + j] = std::min(i, j) + 1;
		CHECK(pca_chol_rinv(L, C.data(), R.data(), Ti.data()));
		bool ok = true;
		for (int i = 0; i < L; i++)
			for (int j = 0; j < L; j++) {
				ok = ok && R[i * L + j] == (i <= j ? 1.0 : 0.0);
				ok = ok && Ti[i * L + j] == (i == j ? 1.0 : (j == i + 1 ? -1.0 : 0.0));
			}
		CHECK(ok);
		// the lower triangle is not read
		for (int i = 0; i < L; i++)
			for (int j = 0; j < i; j++) C[i * L + j] = 1e300;
		CHECK(pca_chol_rinv(L, C.data(), R.data(), Ti.data()) && (L < 2 || Ti[1] == -1.0));
		// diag(d): R = sqrt(d), Ti = 1 / sqrt(d)
		for (int k = 0; k < L * L; k++) C[k] = 0;
		for (int j = 0; j < L; j++) C[j * L + j] = (j + 1.0) * (j + 1.0);
		CHECK(pca_chol_rinv(L, C.data(), R.data(), Ti.data()));
		for (int j = 0; j < L; j++) CHECK(R[j * L + j] == j + 1.0 && Ti[j * L + j] == 1 / (j + 1.0));
	}
	// rank breakdown: two equal columns; a pivot just under and just over the line L 2^-52 max diag; a zero matrix; a NaN
	{
		double C2[4] = {1, 1, 1, 1}, R[4], Ti[4];
		CHECK(!pca_chol_rinv(2, C2, R, Ti));
		double lo[4] = {1, 0, 0, 2 * 0x1p-52}, hi[4] = {1, 0, 0, 2 * 0x1p-52 * (1 + 0x1p-50)};
		CHECK(!pca_chol_rinv(2, lo, R, Ti));
		CHECK(pca_chol_rinv(2, hi, R, Ti));
		double z[4] = {0, 0, 0, 0}, nn[4] = {NAN, 0, 0, 1};
		CHECK(!pca_chol_rinv(2, z, R, Ti));
		CHECK(!pca_chol_rinv(2, nn, R, Ti));
	}
	if (g_fail) { fprintf(stderr, "%d of %d checks failed\n", g_fail, g_done); return 1; }
	printf("%d checks OK\n", g_done);
	return 0;
}
