// host_kmat.h -- operator of an explicit symmetric matrix K resident on one device (kern_kmat.h):
// the thresholded sparse GRM as CSR, or a dense matrix.  Products, and the solve of the null-model fit through
// pcg_run (host_pcg.h), the loop the implicit operator runs.
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.

#define KMAT_DENSE_BUDGET ((size_t)8 << 30)    /* bytes of a dense matrix (8 n^2): grm.DENSE_BUDGET_BYTES */

struct sgx_kmat {
	int device = 0;
	// (released in reverse order: buffers, events, the stream -- sgx_kmat_free waits for the stream first)
	DevStream stream;
	DevEvent ev0, ev1;                     // around the kernels of the last product
	int n = 0;
	bool dense = false;
	// CSR: the full symmetric pattern
	DevBuf<int64_t> rp; DevBuf<int> col; DevBuf<double> val;
	DevBuf<int> long_rows; int n_long = 0; // the rows of the wave form, ascending
	// dense: [rpad][ldd], zero padded; packed columns and slab sums of a launch
	DevBuf<double> K; size_t ldd = 0; int rpad = 0, nslab = 0;
	DevBuf<double> Bp, part;               // [KM_WCOLS][ldd], [nslab][KM_WCOLS][rpad]
	DevBuf<double> diag;                   // [n]
	std::vector<double> h_diag;
	PcgWork pw;
	bool timed = false;
};
static_assert(KM_SLAB % 16 == 0 && KM_ROWS == 32 && KM_WCOLS == 16, "kmat_dense_kernel's tile");

extern "C" void sgx_kmat_free(sgx_kmat *m)
{
	if (!m) return;
	(void)hipSetDevice(m->device);
	if (m->stream) (void)hipStreamSynchronize(m->stream);
	delete m;
}
typedef std::unique_ptr<sgx_kmat, void (*)(sgx_kmat *)> KmatHold;   // what an init function holds its new handle by

// device, stream, events, the diagonal and the solver's workspace of a new handle
static int kmat_open(const char *fn, sgx_kmat *m, int n, int device)
{
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SGX_ENODEV, "%s: no HIP device available", fn);
	if (device < 0 || device >= ndev) return fail(SGX_EINVAL, "%s: device %d out of range", fn, device);
	m->device = device; m->n = n;
	HIPCHK(hipSetDevice(device));
	HIPCHK(m->stream.create(hipStreamNonBlocking));
	HIPCHK(m->ev0.create());
	HIPCHK(m->ev1.create());
	HIPCHK(m->diag.alloc((size_t)n));
	HIPCHK(hipMemcpyAsync(m->diag, m->h_diag.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, m->stream));
	HIPCHK(pcg_work_init(&m->pw, device, m->stream, n));
	return SGX_OK;
}

extern "C" int sgx_kmat_init_csr(int32_t n, const int64_t *row_ptr, const int32_t *col, const double *val, int device,
	sgx_kmat **out)
{
	if (!row_ptr || !out) return fail(SGX_EINVAL, "sgx_kmat_init_csr: NULL argument");
	*out = nullptr;
	if (n < 1) return fail(SGX_EINVAL, "sgx_kmat_init_csr: n=%d < 1", n);
	if (row_ptr[0] != 0) return fail(SGX_EINVAL, "sgx_kmat_init_csr: row_ptr[0]=%lld, not 0", (long long)row_ptr[0]);
	for (int i = 0; i < n; i++)
		if (row_ptr[i + 1] < row_ptr[i]) return fail(SGX_EINVAL, "sgx_kmat_init_csr: row_ptr decreases at row %d", i);
	const size_t nnz = (size_t)row_ptr[n];
	if (nnz && (!col || !val)) return fail(SGX_EINVAL, "sgx_kmat_init_csr: NULL argument");
	KmatHold m(new sgx_kmat(), sgx_kmat_free);
	m->h_diag.assign((size_t)n, 0.0);
	std::vector<int> long_rows;
	for (int i = 0; i < n; i++) {
		for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; e++) {
			int rc = SGX_OK;
			if (col[e] < 0 || col[e] >= n)
				rc = fail(SGX_EINVAL, "sgx_kmat_init_csr: row %d has column %d outside 0..%d", i, (int)col[e], n - 1);
			else if (e > row_ptr[i] && col[e] <= col[e - 1])
				rc = fail(SGX_EINVAL, "sgx_kmat_init_csr: the columns of row %d are not strictly ascending", i);
			else if (!std::isfinite(val[e]))
				rc = fail(SGX_EINVAL, "sgx_kmat_init_csr: the entry (%d, %d) is not finite", i, (int)col[e]);
			if (rc) return rc;
			if (col[e] == i) m->h_diag[i] = val[e];
		}
		if (row_ptr[i + 1] - row_ptr[i] >= KM_WAVE_ROW) long_rows.push_back(i);
	}
	int rc = kmat_open("sgx_kmat_init_csr", m.get(), n, device);
	if (rc) return rc;
	m->n_long = (int)long_rows.size();
	hipStream_t st = m->stream;
	HIPCHK(m->rp.alloc((size_t)n + 1));
	HIPCHK(m->col.alloc(std::max<size_t>(nnz, 1)));
	HIPCHK(m->val.alloc(std::max<size_t>(nnz, 1)));
	HIPCHK(m->long_rows.alloc(std::max<size_t>(long_rows.size(), 1)));
	HIPCHK(hipMemcpyAsync(m->rp, row_ptr, (size_t)(n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
	if (nnz) {
		HIPCHK(hipMemcpyAsync(m->col, col, nnz * sizeof(int), hipMemcpyHostToDevice, st));
		HIPCHK(hipMemcpyAsync(m->val, val, nnz * sizeof(double), hipMemcpyHostToDevice, st));
	}
	if (m->n_long) HIPCHK(hipMemcpyAsync(m->long_rows, long_rows.data(), long_rows.size() * sizeof(int), hipMemcpyHostToDevice, st));
	HIPCHK(hipStreamSynchronize(st));
	*out = m.release();
	return SGX_OK;
}

extern "C" int sgx_kmat_init_dense(const double *K, size_t ld, int32_t n, int device, sgx_kmat **out)
{
	if (!K || !out) return fail(SGX_EINVAL, "sgx_kmat_init_dense: NULL argument");
	*out = nullptr;
	if (n < 1) return fail(SGX_EINVAL, "sgx_kmat_init_dense: n=%d < 1", n);
	if (ld < (size_t)n) return fail(SGX_EINVAL, "sgx_kmat_init_dense: ld=%zu < n=%d", ld, n);
	if ((size_t)n * (size_t)n * sizeof(double) > KMAT_DENSE_BUDGET)
		return fail(SGX_EINVAL, "sgx_kmat_init_dense: a dense matrix of %d samples is above the limit of %zu GiB", n,
			KMAT_DENSE_BUDGET >> 30);
	KmatHold m(new sgx_kmat(), sgx_kmat_free);
	m->dense = true;
	m->h_diag.resize((size_t)n);
	for (size_t i = 0; i < (size_t)n; i++) m->h_diag[i] = K[i * ld + i];
	int rc = kmat_open("sgx_kmat_init_dense", m.get(), n, device);
	if (rc) return rc;
	m->ldd = ((size_t)n + 15) / 16 * 16;
	m->rpad = (n + KM_ROWS - 1) / KM_ROWS * KM_ROWS;
	m->nslab = (int)((m->ldd + KM_SLAB - 1) / KM_SLAB);
	hipStream_t st = m->stream;
	const size_t kb = (size_t)m->rpad * m->ldd * sizeof(double);
	HIPCHK(m->K.alloc((size_t)m->rpad * m->ldd));
	HIPCHK(m->Bp.alloc(KM_WCOLS * m->ldd));
	HIPCHK(m->part.alloc((size_t)m->nslab * KM_WCOLS * m->rpad));
	HIPCHK(hipMemsetAsync(m->K, 0, kb, st));
	HIPCHK(hipMemcpy2DAsync(m->K, m->ldd * sizeof(double), K, ld * sizeof(double), (size_t)n * sizeof(double), (size_t)n,
		hipMemcpyHostToDevice, st));
	HIPCHK(hipStreamSynchronize(st));
	*out = m.release();
	return SGX_OK;
}

extern "C" int sgx_kmat_diag(sgx_kmat *m, double *diag_out)
{
	if (!m || !diag_out) return fail(SGX_EINVAL, "sgx_kmat_diag: NULL argument");
	memcpy(diag_out, m->h_diag.data(), (size_t)m->n * sizeof(double));
	return SGX_OK;
}

extern "C" int sgx_kmat_sync(sgx_kmat *m)
{
	if (!m) return fail(SGX_EINVAL, "sgx_kmat_sync: NULL handle");
	HIPCHK(hipSetDevice(m->device));
	HIPCHK(hipStreamSynchronize(m->stream));
	return SGX_OK;
}

// Out[:, c] = K B[:, c] for c in cols (columns at base + c * ld), device vectors, on the handle's stream
static int kmat_matvec_dev(sgx_kmat *m, const double *B, size_t ldb, const GrmCols &cols, double *Out, size_t ldo)
{
	hipStream_t st = m->stream;
	const int n = m->n;
	const unsigned gx = (unsigned)((n + 255) / 256);
	if (cols.n == 0) return SGX_OK;
	HIPCHK(hipEventRecord(m->ev0, st));
	if (!m->dense) {
		hipLaunchKernelGGL(kmat_csr_thread_kernel, dim3(gx, cols.n), dim3(256), 0, st, n, m->rp, m->col, m->val, B, ldb, cols,
			Out, ldo);
		if (m->n_long)
			hipLaunchKernelGGL(kmat_csr_wave_kernel, dim3((unsigned)((m->n_long + 3) / 4)), dim3(256), 0, st, m->n_long,
				m->long_rows, m->rp, m->col, m->val, B, ldb, cols, Out, ldo);
	} else {
		for (int y0 = 0; y0 < cols.n; y0 += KM_WCOLS) {
			GrmCols gc{};
			gc.n = std::min(KM_WCOLS, cols.n - y0);
			for (int y = 0; y < gc.n; y++) gc.c[y] = cols.c[y0 + y];
			hipLaunchKernelGGL(kmat_dense_pack_kernel, dim3((unsigned)((m->ldd + 255) / 256), KM_WCOLS), dim3(256), 0, st, n,
				m->ldd, B, ldb, gc, m->Bp);
			hipLaunchKernelGGL(kmat_dense_kernel, dim3((unsigned)(m->rpad / KM_ROWS), (unsigned)m->nslab), dim3(WAVE), 0, st,
				m->K, m->ldd, m->Bp, m->rpad, gc.n, m->part);
			hipLaunchKernelGGL(kmat_dense_reduce_kernel, dim3(gx, gc.n), dim3(256), 0, st, n, m->rpad, m->nslab, m->part, gc,
				Out, ldo);
		}
	}
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(m->ev1, st));
	m->timed = true;
	return SGX_OK;
}

// milliseconds the kernels of the last product took on the device (waits for them)
extern "C" int sgx_kmat_matvec_ms(sgx_kmat *m, double *ms_out)
{
	if (!m || !ms_out) return fail(SGX_EINVAL, "sgx_kmat_matvec_ms: NULL argument");
	*ms_out = 0;
	if (!m->timed) return SGX_OK;
	HIPCHK(hipSetDevice(m->device));
	HIPCHK(hipEventSynchronize(m->ev1));
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, m->ev0, m->ev1));
	*ms_out = ms;
	return SGX_OK;
}

static auto kmat_product(sgx_kmat *m)
{
	return [m](const double *Bd, size_t ld, const GrmCols &cols, double *Od, size_t ldo) {
		return kmat_matvec_dev(m, Bd, ld, cols, Od, ldo);
	};
}

extern "C" int sgx_kmat_crossprod_multi(sgx_kmat *m, const double *B, size_t ldb, int k, double *Out)
{
	int rc = pcg_multi_args("sgx_kmat_crossprod_multi", m, m ? m->n : 0, B, ldb, k, Out);
	if (rc) return rc;
	return pcg_crossprod_run(&m->pw, B, ldb, k, Out, kmat_product(m));
}

extern "C" int sgx_kmat_crossprod_multi_dev(sgx_kmat *m, const double *B_dev, size_t ldb, int k, double *Out_dev)
{
	int rc = pcg_multi_args("sgx_kmat_crossprod_multi_dev", m, m ? m->n : 0, B_dev, ldb, k, Out_dev);
	if (rc) return rc;
	HIPCHK(hipSetDevice(m->device));
	return kmat_matvec_dev(m, B_dev, ldb, pcg_cols_iota(k), Out_dev, ldb);
}

extern "C" int sgx_kmat_pcg_multi(sgx_kmat *m, const double *w, const double *tau, const double *B, size_t ldb, int k,
	int maxiter, double tol, double *X_out, int *iters)
{
	if (!w || !tau || !iters) return fail(SGX_EINVAL, "sgx_kmat_pcg_multi: NULL argument");
	int rc = pcg_multi_args("sgx_kmat_pcg_multi", m, m ? m->n : 0, B, ldb, k, X_out);
	if (rc) return rc;
	return pcg_run(&m->pw, m->diag, w, tau, B, ldb, k, maxiter, tol, X_out, iters, kmat_product(m));
}
