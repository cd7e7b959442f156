// host_exact.h -- exact p-values of binary-trait rows with few minor alleles (kern_exact.h):
// sgx_exact_2bit_dev queues the kernel for rows in device memory, sgx_exact_2bit is its wrapper for rows in host memory.
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.

static int exact_check(const sgx_handle *h, const char *who, int max_mac)
{
	int rc = binary_check(h, who, "the exact test");
	if (rc) return rc;
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
	if (!rc) rc = out4_dev_check(h, "sgx_exact_2bit_dev", packed_dev, bpv, M, lut_dev, out4_dev);
	if (rc || M == 0) return rc;
	return exact_rows_dev(h, packed_dev, bpv, M, lut_dev, max_mac, out4_dev);
}

extern "C" int sgx_exact_2bit(sgx_handle *h, const uint8_t *packed, size_t bpv, size_t M,
	const double *lut, int max_mac, double *out4)
{
	int rc = exact_check(h, "sgx_exact_2bit", max_mac);
	if (rc) return rc;
	if (M == 0) return SGX_OK;
	if (!packed || !lut || !out4) return fail(SGX_EINVAL, "sgx_exact_2bit: NULL buffer");
	rc = bpv_check(bpv, h->md.N);
	if (!rc) rc = sync_lane(h);             // (not begin_call: this entry leaves last_issued as it is)
	if (rc) return rc;
	return rows_2bit_host(h, packed, bpv, M, lut, {{out4, 4}},
		[&](const uint8_t *rows, size_t dbpv, size_t m, const double *d_lut, double *const *d_out) {
			return exact_rows_dev(h, rows, dbpv, m, d_lut, max_mac, d_out[0]);
		});
}
