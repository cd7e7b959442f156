// host_firth.h -- Firth bias-reduced effect sizes of binary-trait rows (kern_firth.h): sgx_firth_2bit_dev
// queues the kernel for rows in device memory, sgx_firth_2bit is its wrapper for rows in host memory, sgx_ds_block_firth
// serves the dosage rows of a resident sgx_dsblock (kern_firth_ds.h).
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.

static int firth_check(const sgx_handle *h, const char *who, int maxit)
{
	int rc = binary_check(h, who, "the Firth fit");
	if (rc) return rc;
	if (maxit < 1) return fail(SGX_EINVAL, "%s: maxit=%d, need at least 1", who, maxit);
	return SGX_OK;
}

// M rows in device memory -> out4, queued on the handle's stream.  The grid, and with it the scratch of the lists that
// do not fit LDS (allocated on first use, kept), follows the handle, not M: what a row gets depends on neither.
static int firth_rows_dev(sgx_handle *h, const uint8_t *rows, size_t bpv, size_t M, const double *lut, int maxit, double *out4)
{
	const int N = h->md.N, grid = std::max(1, h->spa_grid);
	int rc = ensure_buf(h, h->firth_scr, firth_slice_bytes(N) * (size_t)grid);
	if (rc) return rc;
	hipLaunchKernelGGL(firth_kernel, dim3((unsigned)std::min<size_t>(M, (size_t)grid)), dim3(FIRTH_BLOCK), 0, h->stream,
		rows, bpv, N, M, lut, h->md.mu, h->md.y, maxit, (uint8_t *)h->firth_scr, out4);
	HIPCHK(hipGetLastError());
	return SGX_OK;
}

extern "C" int sgx_firth_2bit_dev(sgx_handle *h, const uint8_t *packed_dev, size_t bpv, size_t M,
	const double *lut_dev, int maxit, double *out4_dev)
{
	int rc = firth_check(h, "sgx_firth_2bit_dev", maxit);
	if (!rc) rc = out4_dev_check(h, "sgx_firth_2bit_dev", packed_dev, bpv, M, lut_dev, out4_dev);
	if (rc || M == 0) return rc;
	return firth_rows_dev(h, packed_dev, bpv, M, lut_dev, maxit, out4_dev);
}

extern "C" int sgx_firth_2bit(sgx_handle *h, const uint8_t *packed, size_t bpv, size_t M,
	const double *lut, int maxit, double *out4)
{
	int rc = firth_check(h, "sgx_firth_2bit", maxit);
	if (rc) return rc;
	if (M == 0) return SGX_OK;
	if (!packed || !lut || !out4) return fail(SGX_EINVAL, "sgx_firth_2bit: NULL buffer");
	rc = bpv_check(bpv, h->md.N);
	if (!rc) rc = sync_lane(h);             // (not begin_call: this entry leaves last_issued as it is)
	if (rc) return rc;
	return rows_2bit_host(h, packed, bpv, M, lut, {{out4, 4}},
		[&](const uint8_t *rows, size_t dbpv, size_t m, const double *d_lut, double *const *d_out) {
			return firth_rows_dev(h, rows, dbpv, m, d_lut, maxit, d_out[0]);
		});
}

// Bound on the scratch of the dosage kernel's long lists.  A slice is (N - FIRTH_DS_LDS_N) entries of 17 bytes (double
// rows) or 10 (u8 rows) -- 7.3 MB at N = 430 000, about twice the 2-bit kernel's -- so the grid is capped where the
// handle's own would ask for more: 293 workgroups of double rows at that N, still more than one a CU.  Results do not
// depend on the grid.
static const size_t FIRTH_DS_SCR_MAX = (size_t)2 << 30;

extern "C" int sgx_ds_block_firth(sgx_handle *h, const sgx_dsblock *b, size_t n_rows, const int32_t *var_idx,
	const uint8_t *flip, const double *mean, int maxit, double *out4)
{
	int rc = firth_check(h, "sgx_ds_block_firth", maxit);
	if (rc) return rc;
	rc = dsblock_check(h, b, "sgx_ds_block_firth");
	if (rc) return rc;
	if (n_rows == 0) return SGX_OK;
	if (!var_idx || !flip || !mean || !out4) return fail(SGX_EINVAL, "sgx_ds_block_firth: NULL buffer");
	if (b->M == 0) return fail(SGX_EINVAL, "sgx_ds_block_firth: nothing loaded");
	rc = block_idx_check("sgx_ds_block_firth", var_idx, n_rows, b->M);
	if (!rc) rc = begin_call(h);
	if (rc) return rc;

	const int N = b->N;
	const size_t slice = b->dtype == SGX_DS_U8 ? firth_ds_slice_bytes<uint8_t>(N) : firth_ds_slice_bytes<double>(N);
	size_t grid = (size_t)std::max(1, h->spa_grid);
	if (slice) grid = std::max<size_t>(1, std::min(grid, FIRTH_DS_SCR_MAX / slice));
	rc = ensure_buf(h, h->firth_scr, slice * grid);
	if (rc) return rc;

	// tables and results on the device: means, results, then the indices and the flips
	TabLayout tl;
	const auto s_mean = tl.add(n_rows, mean);
	const auto s_out = tl.add<double>(n_rows * 4);
	const auto s_idx = tl.add(n_rows, var_idx);
	const auto s_flip = tl.add(n_rows, flip);
	rc = grow(h->stage_pk, tl.bytes());
	if (!rc) rc = tabs_upload(h->stage_pk, h->stream, s_mean, s_idx, s_flip);
	if (rc) return rc;
	double *d_out = tl.at(h->stage_pk, s_out);
	with_ds_rows(b->dtype, b->rows.p, [&](auto *rows, auto t) {
		hipLaunchKernelGGL((firth_ds_kernel<decltype(t)>), dim3((unsigned)std::min(n_rows, grid)), dim3(FIRTH_BLOCK), 0, h->stream,
			rows, N, n_rows, tl.at(h->stage_pk, s_idx), tl.at(h->stage_pk, s_flip), tl.at(h->stage_pk, s_mean), h->md.mu, h->md.y,
			maxit, (uint8_t *)h->firth_scr, d_out);
	});
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(out4, d_out, n_rows * 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipStreamSynchronize(h->stream));
	return SGX_OK;
}
