// host_burden_ds.h -- aggregate tests on dosage input: a batch of dosage rows resident on the device
// (sgx_dsblock) for the three things the drivers need from it -- per-variant counts, the single-variant
// test of every row, and the burden rows of all units and weight columns.
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.

// Rows as the dosage score kernels read them: row-major, stride N elements.  u8 rows stay u8; i32 rows are
// stored as doubles (NaN = NA_INTEGER), as sgx_scan_i32 converts them; f64 rows as they come.
struct sgx_dsblock {
	int device = 0;
	int N = 0, dtype = 0;
	size_t cap = 0, M = 0;
	DevBuf<uint8_t> rows;
	size_t row_bytes = 0;            // of a resident row: N (u8) or 8 N
	DevBuf<int> d_nv; DevBuf<double> d_sum; DevBuf<long long> d_trunc;   // [cap] ds_stats_kernel
	DevBuf<uint8_t> tabs;            // sgx_dsblock_burden: groups, entries, weights
};

extern "C" void sgx_dsblock_free(sgx_dsblock *b)
{
	if (!b) return;
	(void)hipSetDevice(b->device);
	delete b;
}

// The caller sizes the block: a failed allocation is SGX_ENOMEM.
extern "C" int sgx_dsblock_create(int32_t n_samp, int dtype, size_t max_variants, int device, sgx_dsblock **out)
{
	if (!out) return fail(SGX_EINVAL, "sgx_dsblock_create: NULL argument");
	*out = nullptr;
	if (n_samp <= 0 || max_variants == 0) return fail(SGX_EINVAL, "sgx_dsblock_create: no samples or no variants");
	if (dtype != SGX_DS_U8 && dtype != SGX_DS_I32 && dtype != SGX_DS_F64)
		return fail(SGX_EINVAL, "sgx_dsblock_create: unknown dtype %d", dtype);
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
		return fail(SGX_ENODEV, "sgx_dsblock_create: no device %d", device);
	HIPCHK(hipSetDevice(device));
	std::unique_ptr<sgx_dsblock, void (*)(sgx_dsblock *)> b(new sgx_dsblock(), sgx_dsblock_free);
	b->device = device; b->N = n_samp; b->dtype = dtype; b->cap = max_variants;
	b->row_bytes = (size_t)n_samp * (dtype == SGX_DS_U8 ? 1 : sizeof(double));
	const hipError_t e = [&]() -> hipError_t {
		HIPPASS(b->rows.alloc(b->cap * b->row_bytes + 16));
		HIPPASS(b->d_nv.alloc(b->cap));
		HIPPASS(b->d_sum.alloc(b->cap));
		HIPPASS(b->d_trunc.alloc(b->cap));
		return hipSuccess;
	}();
	if (e != hipSuccess)
		return fail(SGX_ENOMEM, "sgx_dsblock_create: %zu rows of %zu bytes: %s", max_variants, b->row_bytes, hipGetErrorString(e));
	*out = b.release();
	return SGX_OK;
}

static int dsblock_check(sgx_handle *h, const sgx_dsblock *b, const char *who)
{
	if (!h || !b) return fail(SGX_EINVAL, "%s: NULL argument", who);
	if (b->device != h->device) return fail(SGX_EINVAL, "%s: block and handle are on different devices", who);
	if (b->N != h->md.N) return fail(SGX_EINVAL, "Invalid length of dosages: %d.", b->N);
	return SGX_OK;
}

// ds_stats_kernel on the m rows just put into the block from row `first` on, their counts to the caller; the block holds
// first + m rows when they are back
static int dsblock_counts(sgx_handle *h, sgx_dsblock *b, size_t first, size_t m, int32_t *n_valid, double *sum, int64_t *sum_trunc)
{
	with_ds_rows(b->dtype, b->rows.p, [&](auto *rows, auto t) {
		hipLaunchKernelGGL((ds_stats_kernel<decltype(t)>), dim3((unsigned)m), dim3(256), 0, h->stream,
			rows + first * (size_t)b->N, b->N, b->d_nv.p + first, b->d_sum.p + first, b->d_trunc.p + first);
	});
	HIPCHK(hipGetLastError());
	static_assert(sizeof(long long) == sizeof(int64_t), "sum_trunc");
	HIPCHK(hipMemcpyAsync(n_valid, b->d_nv.p + first, m * sizeof(int), hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipMemcpyAsync(sum, b->d_sum.p + first, m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipMemcpyAsync(sum_trunc, b->d_trunc.p + first, m * sizeof(long long), hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipStreamSynchronize(h->stream));
	b->M = first + m;
	return SGX_OK;
}

// Rows in host memory into the block -- the one crossing of PCIe of a batch -- and their counts back.
// u8 / f64 rows are copied to where they stay, in chunks of the pipeline's size; i32 chunks land in the
// pipeline's two input buffers on the copy stream and are converted on the handle's stream meanwhile.
extern "C" int sgx_dsblock_load(sgx_handle *h, sgx_dsblock *b, const void *dosage, size_t M,
	int32_t *n_valid, double *sum, int64_t *sum_trunc)
{
	int rc = dsblock_check(h, b, "sgx_dsblock_load");
	if (rc) return rc;
	if (!dosage || !n_valid || !sum || !sum_trunc) return fail(SGX_EINVAL, "sgx_dsblock_load: NULL buffer");
	if (M == 0 || M > b->cap) return fail(SGX_EINVAL, "sgx_dsblock_load: %zu variants, the block holds up to %zu", M, b->cap);
	rc = sync_lane(h);                        // anything that still reads the block through this handle is done
	if (rc) return rc;
	b->M = 0;
	const int N = b->N;
	RowSrc src = plain_rows(dosage, (size_t)N * (b->dtype == SGX_DS_U8 ? 1 : b->dtype == SGX_DS_I32 ? sizeof(int32_t) : sizeof(double)));
	const size_t chunk = scan_chunk(h, src.row_bytes, M);
	if (b->dtype != SGX_DS_I32) {
		for (size_t off = 0; off < M; off += chunk)
			HIPCHK(hipMemcpyAsync(b->rows + off * b->row_bytes, src.rows + off * src.row_bytes, std::min(chunk, M - off) * src.row_bytes,
				hipMemcpyHostToDevice, h->stream));
	} else {
		rc = ensure_pipe(h, chunk * src.row_bytes, 0, 1);
		if (rc) return rc;
		rc = ingest(h, M, chunk,
			[&](int k, size_t off, size_t m) -> int { return src_upload(h, src, k, off, m, src.row_bytes); },
			[&](int k, size_t off, size_t m) -> int {
				hipLaunchKernelGGL(i32_rows_to_f64, dim3(1024), dim3(256), 0, h->stream,
					(const int *)h->pipe_in[k].p, m * (size_t)N, reinterpret_cast<double *>(b->rows + off * b->row_bytes));
				HIPCHK(hipGetLastError());
				return SGX_OK;
			});
		if (rc) return rc;
	}
	return dsblock_counts(h, b, 0, M, n_valid, sum, sum_trunc);
}

// The same block from packed-real rows as the file stores them (kern_unpack.h): raw chunks land in the pipeline's two
// raw buffers on the copy stream and are decoded and sample-selected into the block's float64 rows on the handle's
// stream meanwhile.  The counts are those of sgx_dsblock_load on the decoded rows.
extern "C" int sgx_ds_block_load_packed(sgx_handle *h, sgx_dsblock *b, const void *raw, int cls, size_t n_file_samp,
	double scale, double offset, const int32_t *sel, size_t M, int32_t *n_valid, double *sum, int64_t *sum_trunc)
{
	int rc = dsblock_check(h, b, "sgx_ds_block_load_packed");
	if (rc) return rc;
	if (b->dtype != SGX_DS_F64) return fail(SGX_EINVAL, "sgx_ds_block_load_packed: packed-real rows need a float64 block");
	RowSrc src;
	rc = packed_check("sgx_ds_block_load_packed", b->N, raw, cls, n_file_samp, scale, offset, sel, src);
	if (rc) return rc;
	if (!n_valid || !sum || !sum_trunc) return fail(SGX_EINVAL, "sgx_ds_block_load_packed: NULL buffer");
	if (M == 0 || M > b->cap) return fail(SGX_EINVAL, "sgx_ds_block_load_packed: %zu variants, the block holds up to %zu", M, b->cap);
	rc = sync_lane(h);                        // anything that still reads the block through this handle is done
	if (rc) return rc;
	b->M = 0;
	const size_t chunk = scan_chunk(h, src.row_bytes, M);
	rc = ensure_pipe(h, 0, 0, 1);
	if (rc) return rc;
	rc = src_prepare(h, src, M, chunk);
	if (rc) return rc;
	rc = ingest(h, M, chunk,
		[&](int k, size_t off, size_t m) -> int { return copy_raw(h, src, k, off, m); },
		[&](int k, size_t off, size_t m) -> int {
			return launch_unpack(h->stream, src, h->pipe_raw[k], b->N, m, reinterpret_cast<double *>(b->rows + off * b->row_bytes));
		});
	if (rc) return rc;
	return dsblock_counts(h, b, 0, M, n_valid, sum, sum_trunc);
}

// Single-variant test of the m resident rows from row `first` on, in scan_chunk's chunks, on a lane that begin_call
// made ready: a call's launches depend on m alone, not on where the rows lie in the block
static int dsblock_scan_rows(sgx_handle *h, const sgx_dsblock *b, size_t first, size_t m, double *out8, uint8_t *valid)
{
	const size_t N = (size_t)b->N;
	const size_t per_row = b->dtype == SGX_DS_U8 ? N : b->dtype == SGX_DS_I32 ? N * (sizeof(int32_t) + sizeof(double)) : N * sizeof(double);
	const size_t chunk = scan_chunk(h, per_row, m);
	int rc = ensure_stage(h, 0, chunk);
	if (rc) return rc;
	rc = ensure_recs(h, chunk);
	if (rc) return rc;
	sgx_stats total{};
	for (size_t off = 0; off < m; off += chunk) {
		const size_t mc = std::min(chunk, m - off);
		const uint8_t *rows = b->rows + (first + off) * b->row_bytes;
		if (b->dtype == SGX_DS_U8) rc = scan_staged<IN_U8>(h, rows, b->row_bytes, mc, out8 + off * 8, valid + off, total);
		else rc = scan_staged<IN_F64>(h, rows, b->row_bytes, mc, out8 + off * 8, valid + off, total);
		if (rc) return rc;
	}
	h->stats = total;
	return SGX_OK;
}

// Single-variant test of every resident row, in scan_chunk's chunks: results equal sgx_scan_u8 / _i32 / _f64 on rows
// that take the dosage kernels there bit for bit.  Hard-call u8 / i32 rows are NOT packed to 2-bit here (the
// host-buffer scans do that): they take the dosage kernels too, and agree with the fixed-point kernels within the
// scan's tolerance.
extern "C" int sgx_dsblock_scan(sgx_handle *h, const sgx_dsblock *b, double *out8, uint8_t *valid)
{
	int rc = dsblock_check(h, b, "sgx_dsblock_scan");
	if (rc) return rc;
	if (!out8 || !valid) return fail(SGX_EINVAL, "sgx_dsblock_scan: NULL buffer");
	if (b->M == 0) return fail(SGX_EINVAL, "sgx_dsblock_scan: nothing loaded");
	rc = begin_call(h);
	if (rc) return rc;
	return dsblock_scan_rows(h, b, 0, b->M, out8, valid);
}

template <typename T>
static void launch_collapse_ds(hipStream_t st, const T *rows, int N, size_t n_groups, const long long *grp_ptr,
	const int *var_idx, const uint8_t *flip, int n_cols, int c0, int nc, const double *w, const double *mw, double *out)
{
	auto go = [&](auto nct, auto spt) {
		constexpr int NC = decltype(nct)::value, SPT = decltype(spt)::value;
		const dim3 grid((unsigned)((N + 256 * SPT - 1) / (256 * SPT)), (unsigned)n_groups);
		hipLaunchKernelGGL((burden_collapse_ds_kernel<T, NC, SPT>), grid, dim3(256), 0, st,
			rows, N, grp_ptr, var_idx, flip, n_cols, c0, nc, w, mw, out);
	};
	using std::integral_constant;
	constexpr bool U8 = sizeof(T) == 1;
	if (nc <= 1) go(integral_constant<int, 1>{}, integral_constant<int, U8 ? 16 : 4>{});
	else if (nc <= 2) go(integral_constant<int, 2>{}, integral_constant<int, U8 ? 16 : 4>{});
	else if (nc <= 4) go(integral_constant<int, 4>{}, integral_constant<int, U8 ? 8 : 4>{});
	else go(integral_constant<int, 8>{}, integral_constant<int, 4>{});
}

// Burden rows of n_groups units x n_cols weight columns from the resident rows, then the single-variant test on
// each (ds_mat_burden + single_test_bin/quant of saige_burden_test_*, saige_acatv_test_bin, saige_acato_test_bin,
// src/saige_main.cpp:526-976, for INTSXP / REALSXP dosages).  Whole groups per chunk of STAGE_BYTES of collapsed rows;
// the collapse kernel takes up to SGX_DS_COLS_PER_PASS columns per pass over a group's rows.
#define SGX_DS_COLS_PER_PASS 8
extern "C" int sgx_dsblock_burden(sgx_handle *h, const sgx_dsblock *b, size_t n_groups, const int64_t *grp_ptr,
	const int32_t *var_idx, const uint8_t *flip, int n_cols, const double *w, const double *mw,
	double *out8, uint8_t *valid)
{
	int rc = dsblock_check(h, b, "sgx_dsblock_burden");
	if (rc) return rc;
	if (n_groups == 0) return SGX_OK;
	if (!grp_ptr || !var_idx || !flip || !w || !mw || !out8 || !valid)
		return fail(SGX_EINVAL, "sgx_dsblock_burden: NULL buffer");
	if (n_cols < 1 || n_cols > SGX_DS_MAX_COLS)
		return fail(SGX_EINVAL, "sgx_dsblock_burden: n_cols = %d, 1 .. %d are supported", n_cols, SGX_DS_MAX_COLS);
	if (b->M == 0) return fail(SGX_EINVAL, "sgx_dsblock_burden: nothing loaded");
	const int32_t *bad;
	rc = csr_check("sgx_dsblock_burden", "grp_ptr", n_groups, grp_ptr, var_idx, b->M, &bad);
	if (rc) return rc;
	if (bad) return fail(SGX_EINVAL, "sgx_dsblock_burden: variant index %d outside the block's %zu rows", *bad, b->M);
	const int64_t nnz = grp_ptr[n_groups];
	rc = begin_call(h);
	if (rc) return rc;
	// device copies of the tables (those of the entries are empty slots where no group has one)
	std::vector<long long> gp(grp_ptr, grp_ptr + n_groups + 1);
	TabLayout tl;
	const auto s_gp = tl.add(gp.size(), gp.data());
	const auto s_idx = tl.add(nnz, var_idx);
	const auto s_w = tl.add((size_t)nnz * n_cols, w), s_mw = tl.add((size_t)nnz * n_cols, mw);
	const auto s_flip = tl.add(nnz, flip);
	rc = grow(const_cast<sgx_dsblock *>(b)->tabs, tl.bytes());
	if (!rc) rc = tabs_upload(b->tabs, h->stream, s_gp, s_idx, s_w, s_mw, s_flip);
	if (rc) return rc;
	HIPCHK(hipStreamSynchronize(h->stream));      // gp is a local
	const int N = b->N;
	const size_t row_bytes = (size_t)N * sizeof(double);
	size_t gchunk = std::max<size_t>(1, STAGE_BYTES / (row_bytes * (size_t)n_cols));
	gchunk = std::min<size_t>(std::min(gchunk, n_groups), 65535);       // grid.y of the collapse kernel
	rc = ensure_stage(h, gchunk * n_cols * row_bytes, gchunk * n_cols);
	if (rc) return rc;
	rc = ensure_recs(h, gchunk * n_cols);
	if (rc) return rc;
	sgx_stats total{};
	for (size_t off = 0; off < n_groups; off += gchunk) {
		const size_t ng = std::min(gchunk, n_groups - off), m = ng * (size_t)n_cols;
		for (int c0 = 0; c0 < n_cols; c0 += SGX_DS_COLS_PER_PASS) {
			const int nc = std::min(SGX_DS_COLS_PER_PASS, n_cols - c0);
			with_ds_rows(b->dtype, b->rows.p, [&](auto *rows, auto) {
				launch_collapse_ds(h->stream, rows, N, ng, tl.at(b->tabs, s_gp) + off, tl.at(b->tabs, s_idx), tl.at(b->tabs, s_flip),
					n_cols, c0, nc, tl.at(b->tabs, s_w), tl.at(b->tabs, s_mw), reinterpret_cast<double *>(h->stage_in.p));
			});
			HIPCHK(hipGetLastError());
		}
		rc = scan_staged<IN_F64>(h, h->stage_in, row_bytes, m, out8 + off * n_cols * 8, valid + off * n_cols, total);
		if (rc) return rc;
	}
	h->stats = total;
	return SGX_OK;
}
