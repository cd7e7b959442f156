// host_pcg.h -- the preconditioned conjugate-gradient loop of the null-model fit (PCG_diag_sigma) and its workspace,
// shared by the operators that have a product K b: the implicit GRM (host_grm.h) and the explicit matrix (host_kmat.h).
// The vector kernels (pcg_*_kernel, dot_partial_kernel) are in kern_grm.h.
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.

#define GRM_RED_BLOCKS 256

struct PcgWork {
	int device = 0;
	hipStream_t stream = nullptr;              // the operator's stream (not owned)
	int N = 0;
	DevBuf<double> part; PinBuf<double> h_part;      // [2 * GRM_MAX_RHS][GRM_RED_BLOCKS] block partials (device / pinned)
	DevBuf<double> minv, w;                          // [N]
	DevBuf<double> B, O;                             // [k][N] staging of host-pointer calls, k the largest seen (pcg_reserve)
	DevBuf<double> R, Z, P, X, AP, GP;               // [k][N]
	DevBuf<double> Wc, Mc;                           // [k][N]: weight rows and per-column minv of a per-column solve
};

// room for k columns (k <= GRM_MAX_RHS) in the [k][N] vectors
static hipError_t pcg_reserve(PcgWork *pw, int k)
{
	for (DevBuf<double> *b : {&pw->B, &pw->O, &pw->R, &pw->Z, &pw->P, &pw->X, &pw->AP, &pw->GP}) HIPPASS(b->reserve((size_t)k * pw->N));
	return hipSuccess;
}

// room for k columns in the per-column weights and preconditioners
static hipError_t pcg_reserve_w(PcgWork *pw, int k)
{
	for (DevBuf<double> *b : {&pw->Wc, &pw->Mc}) HIPPASS(b->reserve((size_t)k * pw->N));
	return hipSuccess;
}

// the workspace of an operator on n vectors' entries, on the operator's device (current) and stream
static hipError_t pcg_work_init(PcgWork *pw, int device, hipStream_t stream, int n)
{
	pw->device = device; pw->stream = stream; pw->N = n;
	HIPPASS(pw->minv.alloc((size_t)n));
	HIPPASS(pw->w.alloc((size_t)n));
	HIPPASS(pw->part.alloc(2 * GRM_MAX_RHS * GRM_RED_BLOCKS));
	HIPPASS(pw->h_part.alloc(2 * GRM_MAX_RHS * GRM_RED_BLOCKS));
	return pcg_reserve(pw, 1);
}

// per column y of cols: out[y] = sum a (* b) as GRM_RED_BLOCKS block partials summed on the host in
// fixed order; one host sync for up to two sets (a1/b1 over cols1, then a2/b2 over cols2; a2 == NULL: none)
static int pcg_sum(PcgWork *pw, const double *a1, const double *b1, size_t ld1, const GrmCols &c1,
	double *out1, const double *a2 = nullptr, const double *b2 = nullptr, size_t ld2 = 0, const GrmCols *c2 = nullptr,
	double *out2 = nullptr)
{
	hipStream_t st = pw->stream;
	const size_t n = (size_t)pw->N;
	auto launch = [&](const double *a, const double *b, size_t ld, const GrmCols &c, double *part) {
		if (b) hipLaunchKernelGGL((dot_partial_kernel<true>), dim3(GRM_RED_BLOCKS, c.n), dim3(256), 0, st, a, b, ld, c, n, part);
		else hipLaunchKernelGGL((dot_partial_kernel<false>), dim3(GRM_RED_BLOCKS, c.n), dim3(256), 0, st, a, b, ld, c, n, part);
	};
	const int n1 = c1.n, n2 = a2 ? c2->n : 0;
	if (n1 + n2 == 0) return SGX_OK;
	if (n1) launch(a1, b1, ld1, c1, pw->part);
	if (n2) launch(a2, b2, ld2, *c2, pw->part + (size_t)n1 * GRM_RED_BLOCKS);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(pw->h_part, pw->part, (size_t)(n1 + n2) * GRM_RED_BLOCKS * sizeof(double), hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	for (int y = 0; y < n1 + n2; y++) {
		double v = 0;
		for (int i = 0; i < GRM_RED_BLOCKS; i++) v += pw->h_part[(size_t)y * GRM_RED_BLOCKS + i];   // fixed order
		if (y < n1) out1[y] = v; else out2[y - n1] = v;
	}
	return SGX_OK;
}

// the argument rules of the k-column entry points of an operator on n entries
static int pcg_multi_args(const char *fn, const void *h, int n, const void *B, size_t ldb, int k, const void *Out)
{
	if (!h || !B || !Out) return fail(SGX_EINVAL, "%s: NULL argument", fn);
	if (k < 1 || k > SGX_GRM_MAX_RHS) return fail(SGX_EINVAL, "%s: k=%d outside 1..%d", fn, k, SGX_GRM_MAX_RHS);
	if (ldb < (size_t)n) return fail(SGX_EINVAL, "%s: ldb=%zu < N=%d", fn, ldb, n);
	return SGX_OK;
}

static GrmCols pcg_cols_iota(int k)
{
	GrmCols c{};
	c.n = k;
	for (int j = 0; j < k; j++) c.c[j] = j;
	return c;
}

// k columns of N doubles between a host array with columns ldh doubles apart and a packed [k][N] device array
// (one linear copy when the host columns are packed too)
static hipError_t pcg_copy_cols(PcgWork *pw, double *dst, const double *src, size_t ldh, int k, hipMemcpyKind kind)
{
	const size_t nb = (size_t)pw->N * sizeof(double);
	if (ldh == (size_t)pw->N || k == 1) return hipMemcpyAsync(dst, src, (size_t)k * nb, kind, pw->stream);
	const bool up = kind == hipMemcpyHostToDevice;
	return hipMemcpy2DAsync(dst, up ? nb : ldh * sizeof(double), src, up ? ldh * sizeof(double) : nb, nb, (size_t)k, kind, pw->stream);
}

// Out = K B for k host vectors, column j at B + j * ldb (and Out + j * ldb); product(B_dev, ld, cols, Out_dev, ldo)
// is the operator's product on device vectors
template <class Product>
static int pcg_crossprod_run(PcgWork *pw, const double *B, size_t ldb, int k, double *Out, Product product)
{
	HIPCHK(hipSetDevice(pw->device));
	HIPCHK(pcg_reserve(pw, k));
	const size_t N = (size_t)pw->N;
	HIPCHK(pcg_copy_cols(pw, pw->B, B, ldb, k, hipMemcpyHostToDevice));
	int rc = product(pw->B, N, pcg_cols_iota(k), pw->O, N);
	if (rc) return rc;
	HIPCHK(pcg_copy_cols(pw, Out, pw->O, ldb, k, hipMemcpyDeviceToHost));
	HIPCHK(hipStreamSynchronize(pw->stream));
	return SGX_OK;
}

// PCG_diag_sigma (saige_fitnull.cpp:581-614): solves (tau0 diag(1/w) + tau1 K) x = b for k right-hand
// sides in lockstep (host vectors, column j at B + j * ldb): every column takes the reference's steps on
// its own scalars; a column stops (and leaves the products) once rr <= tol or maxiter is reached.  Each
// reduction step is one host sync for all columns.  diag (device, [N]) is diag(K); product as above, called
// with the columns still active, and not at all when tau1 == 0.
// pc (NULL: one w and one diagonal for all columns, the plain kernels): column j has the weights pc->W row
// pc->w_idx[j] (w is not read) and is preconditioned with its own diagonal, row 1 + pc->drow[j] of pc->D.
struct PcgPerCol {
	const double *W; size_t ldw; int n_w;  // host [n_w][ldw]
	const int *w_idx, *drow;               // [k], checked by the caller
	const double *D;                       // device [rows][N]
};

// The loop on vectors that are resident: the right-hand sides at Bd + j * ldB and (pc == NULL) the weights wd are device
// arrays, the workspace has room for k columns (pcg_reserve), the device is current.  The iterates end in pw->X
// ([k][N], packed) behind the stream's last reduction; only the per-iteration scalars cross to the host.
template <class Product>
static int pcg_core(PcgWork *pw, const double *diag, const double *wd, const double *tau, const double *Bd, size_t ldB, int k,
	int maxiter, double tol, int *iters, Product product, const PcgPerCol *pc)
{
	hipStream_t st = pw->stream;
	const int n = pw->N;
	const size_t N = (size_t)n;
	const dim3 bl(256);
	const unsigned gx = (unsigned)((n + 255) / 256);
	const double tau0 = tau[0], tau1 = tau[1];
	const GrmCols all = pcg_cols_iota(k);
	GrmIdx widx{}, ex{};
	if (pc) {
		HIPCHK(pcg_reserve_w(pw, std::max(k, pc->n_w)));
		HIPCHK(pcg_copy_cols(pw, pw->Wc, pc->W, pc->ldw, pc->n_w, hipMemcpyHostToDevice));
		for (int j = 0; j < k; j++) { widx.v[j] = pc->w_idx[j]; ex.v[j] = pc->drow[j]; }
		hipLaunchKernelGGL(pcg_minv_cols_kernel, dim3(gx, k), bl, 0, st, n, pw->Wc, widx, pc->D, ex,
			tau0, tau1, pw->Mc, all);
		hipLaunchKernelGGL(pcg_init_kernel<true>, dim3(gx, k), bl, 0, st, n, Bd, ldB, pw->Mc, pw->R, pw->Z, pw->P, pw->X, all);
	} else {
		hipLaunchKernelGGL(pcg_minv_kernel, dim3(gx), bl, 0, st, n, wd, diag, tau0, tau1, pw->minv);
		hipLaunchKernelGGL(pcg_init_kernel<false>, dim3(gx, k), bl, 0, st, n, Bd, ldB, pw->minv, pw->R, pw->Z, pw->P, pw->X, all);
	}
	double rr[GRM_MAX_RHS], rz[GRM_MAX_RHS];
	int rc;
	if ((rc = pcg_sum(pw, pw->R, pw->R, N, all, rr, pw->R, pw->Z, N, &all, rz))) return rc;
	for (int j = 0; j < k; j++) iters[j] = 0;
	for (;;) {
		GrmCols act{};
		for (int j = 0; j < k; j++)
			if (iters[j] < maxiter && rr[j] > tol) act.c[act.n++] = j;
		if (act.n == 0) break;
		for (int y = 0; y < act.n; y++) iters[act.c[y]]++;
		const double *gp = nullptr;
		if (tau1 != 0) {                       // get_crossprod :569-575
			if ((rc = product(pw->P, N, act, pw->GP, N))) return rc;
			gp = pw->GP;
		}
		if (pc) hipLaunchKernelGGL(pcg_ap_kernel<true>, dim3(gx, act.n), bl, 0, st, n, pw->P, pw->Wc, gp, tau0, tau1, pw->AP, act, widx);
		else hipLaunchKernelGGL(pcg_ap_kernel<false>, dim3(gx, act.n), bl, 0, st, n, pw->P, wd, gp, tau0, tau1, pw->AP, act, widx);
		double pAp[GRM_MAX_RHS], rz1[GRM_MAX_RHS], rrn[GRM_MAX_RHS];
		if ((rc = pcg_sum(pw, pw->P, pw->AP, N, act, pAp))) return rc;
		GrmScal a{};
		for (int y = 0; y < act.n; y++) a.v[y] = rz[act.c[y]] / pAp[y];
		if (pc) hipLaunchKernelGGL(pcg_update_kernel<true>, dim3(gx, act.n), bl, 0, st, n, a, pw->P, pw->AP, pw->Mc, pw->X, pw->R, pw->Z, act);
		else hipLaunchKernelGGL(pcg_update_kernel<false>, dim3(gx, act.n), bl, 0, st, n, a, pw->P, pw->AP, pw->minv, pw->X, pw->R, pw->Z, act);
		if ((rc = pcg_sum(pw, pw->Z, pw->R, N, act, rz1, pw->R, pw->R, N, &act, rrn))) return rc;
		GrmScal bet{};
		for (int y = 0; y < act.n; y++) bet.v[y] = rz1[y] / rz[act.c[y]];
		hipLaunchKernelGGL(pcg_dir_kernel, dim3(gx, act.n), bl, 0, st, n, bet, pw->Z, pw->P, act);
		for (int y = 0; y < act.n; y++) { rz[act.c[y]] = rz1[y]; rr[act.c[y]] = rrn[y]; }
	}
	HIPCHK(hipGetLastError());
	return SGX_OK;
}

// pcg_core on host vectors (column j at B + j * ldb; w on the host, not read with pc): up, solve, down.
template <class Product>
static int pcg_run(PcgWork *pw, const double *diag, const double *w, const double *tau, const double *B, size_t ldb, int k,
	int maxiter, double tol, double *X_out, int *iters, Product product, const PcgPerCol *pc = nullptr)
{
	HIPCHK(hipSetDevice(pw->device));
	HIPCHK(pcg_reserve(pw, k));
	hipStream_t st = pw->stream;
	HIPCHK(pcg_copy_cols(pw, pw->B, B, ldb, k, hipMemcpyHostToDevice));
	if (!pc) HIPCHK(hipMemcpyAsync(pw->w, w, (size_t)pw->N * sizeof(double), hipMemcpyHostToDevice, st));
	int rc = pcg_core(pw, diag, pw->w, tau, pw->B, (size_t)pw->N, k, maxiter, tol, iters, product, pc);
	if (rc) return rc;
	HIPCHK(pcg_copy_cols(pw, X_out, pw->X, ldb, k, hipMemcpyDeviceToHost));
	HIPCHK(hipStreamSynchronize(st));
	return SGX_OK;
}
