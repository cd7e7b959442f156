// host_exact.h -- exact p-values of binary-trait rows with few minor alleles (kern_exact.h):
// sgx_exact_2bit_dev queues the kernel for rows in device memory, sgx_exact_2bit is its wrapper for rows in host memory.
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.

static int exact_check(const sgx_handle *h, const char *who, int max_mac)
{
	if (!h) return fail(SGX_EINVAL, "%s: NULL handle", who);
	if (h->owner) return fail(SGX_EINVAL, "%s: not on a twin", who);
	if (h->md.quant) return fail(SGX_EINVAL, "%s: the exact test is for binary traits", who);
	if (max_mac < 1 || max_mac > SGX_EXACT_MAX_MAC)
		return fail(SGX_EINVAL, "%s: max_mac=%d, need 1..%d", who, max_mac, SGX_EXACT_MAX_MAC);
	return SGX_OK;
}

// M rows in device memory -> out4, queued on the handle's stream: a wave per row, eight workgroups a CU at most (the
// waves loop over the rows; what a row gets depends on neither M nor the grid).  No scratch.
static int exact_rows_dev(sgx_handle *h, const uint8_t *rows, size_t bpv, size_t M, const double *lut, int max_mac, double *out4)
{
	constexpr size_t NW = EXACT_BLOCK / WAVE;
	const size_t grid = std::min((M + NW - 1) / NW, (size_t)std::max(1, h->n_cu) * 8);
	hipLaunchKernelGGL(exact_kernel, dim3((unsigned)grid), dim3(EXACT_BLOCK), 0, h->stream,
		rows, bpv, h->md.N, M, lut, h->md.mu, h->md.y, max_mac, out4);
	HIPCHK(hipGetLastError());
	return SGX_OK;
}

extern "C" int sgx_exact_2bit_dev(sgx_handle *h, const uint8_t *packed_dev, size_t bpv, size_t M,
	const double *lut_dev, int max_mac, double *out4_dev)
{
	int rc = exact_check(h, "sgx_exact_2bit_dev", max_mac);
	if (rc) return rc;
	if (M == 0) return SGX_OK;
	if (!packed_dev || !lut_dev || !out4_dev) return fail(SGX_EINVAL, "sgx_exact_2bit_dev: NULL buffer");
	rc = dev_rows_check("sgx_exact_2bit_dev", packed_dev, bpv, h->md.N);
	if (rc) return rc;
	if (((uintptr_t)lut_dev & 7u) != 0 || ((uintptr_t)out4_dev & 7u) != 0)
		return fail(SGX_EINVAL, "sgx_exact_2bit_dev: lut_dev and out4_dev must be 8-byte aligned");
	rc = set_dev(h);
	if (rc) return rc;
	return exact_rows_dev(h, packed_dev, bpv, M, lut_dev, max_mac, out4_dev);
}

extern "C" int sgx_exact_2bit(sgx_handle *h, const uint8_t *packed, size_t bpv, size_t M,
	const double *lut, int max_mac, double *out4)
{
	int rc = exact_check(h, "sgx_exact_2bit", max_mac);
	if (rc) return rc;
	if (M == 0) return SGX_OK;
	if (!packed || !lut || !out4) return fail(SGX_EINVAL, "sgx_exact_2bit: NULL buffer");
	const int N = h->md.N;
	rc = bpv_check(bpv, N);
	if (!rc) rc = sync_lane(h);             // (not begin_call: this entry leaves last_issued as it is)
	if (rc) return rc;

	// the chunks of sgx_firth_2bit: rows at the device stride, then tables and results
	const size_t dbpv = sgx_row_stride(N);
	const size_t rchunk = scan_chunk(h, dbpv, M);
	TabLayout tl;
	tl.add<uint8_t>(rchunk * dbpv);
	const auto s_lut = tl.add<double>(rchunk * 4), s_out = tl.add<double>(rchunk * 4);
	rc = grow(h->stage_pk, tl.bytes());
	if (rc) return rc;
	double *d_lut = tl.at(h->stage_pk, s_lut), *d_out = tl.at(h->stage_pk, s_out);
	for (size_t off = 0; off < M; off += rchunk) {
		const size_t m = std::min(rchunk, M - off);
		rc = copy_rows_h2d(h->stage_pk, dbpv, packed + off * bpv, bpv, m, h->stream);
		if (!rc) rc = tab_copy(h->stage_pk, s_lut, lut + 4 * off, 4 * m, h->stream);
		if (!rc) rc = exact_rows_dev(h, h->stage_pk, dbpv, m, d_lut, max_mac, d_out);
		if (rc) return rc;
		HIPCHK(hipMemcpyAsync(out4 + 4 * off, d_out, m * 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
		HIPCHK(hipStreamSynchronize(h->stream));
	}
	return SGX_OK;
}
