// host_rows.h -- the chunk loop over rows in host memory and the argument checks that the per-row follow-ups on 2-bit
// rows share (sgx_firth_2bit, sgx_exact_2bit, sgx_cond_2bit, the _dev forms of the first two).
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.

struct RowOut { double *host; size_t per_row; };      // a result array in host memory: per_row doubles a row

// M 2-bit rows in host memory with one 4-entry table each, in the chunks of the host-buffer scans: in h->stage_pk the
// rows at the device stride, then the tables, then the results in the order of outs.  Per chunk rows and tables go up,
// run(rows_dev, dbpv, m, lut_dev, outs_dev) queues the device work on h->stream, the results come down and the stream is
// waited for.  The caller has checked its arguments and made its own lane call.
template <size_t R, class Run>
static int rows_2bit_host(sgx_handle *h, const uint8_t *packed, size_t bpv, size_t M, const double *lut,
	const RowOut (&outs)[R], Run run)
{
	const size_t dbpv = sgx_row_stride(h->md.N), rchunk = scan_chunk(h, dbpv, M);
	TabLayout tl;
	tl.add<uint8_t>(rchunk * dbpv);
	const auto s_lut = tl.add<double>(rchunk * 4);
	TabSlot<double> s_out[R];
	for (size_t r = 0; r < R; r++) s_out[r] = tl.add<double>(rchunk * outs[r].per_row);
	int rc = grow(h->stage_pk, tl.bytes());
	if (rc) return rc;
	double *d_lut = tl.at(h->stage_pk, s_lut), *d_out[R];
	for (size_t r = 0; r < R; r++) d_out[r] = tl.at(h->stage_pk, s_out[r]);
	for (size_t off = 0; off < M; off += rchunk) {
		const size_t m = std::min(rchunk, M - off);
		rc = copy_rows_h2d(h->stage_pk, dbpv, packed + off * bpv, bpv, m, h->stream);
		if (!rc) rc = tab_copy(h->stage_pk, s_lut, lut + 4 * off, 4 * m, h->stream);
		if (!rc) rc = run(h->stage_pk, dbpv, m, d_lut, d_out);
		if (rc) return rc;
		for (size_t r = 0; r < R; r++)
			HIPCHK(hipMemcpyAsync(outs[r].host + off * outs[r].per_row, d_out[r], m * outs[r].per_row * sizeof(double),
				hipMemcpyDeviceToHost, h->stream));
		HIPCHK(hipStreamSynchronize(h->stream));
	}
	return SGX_OK;
}

// All n 2-bit rows of a grouped call (sgx_skat_2bit, sgx_skat_kmat_2bit, sgx_collapse_2bit: an entry may name any row)
// from host memory to dst at the device stride, queued on st in the chunks of the host-buffer scans.
static int rows_2bit_upload(const sgx_handle *h, uint8_t *dst, size_t dbpv, const uint8_t *packed, size_t bpv, size_t n, hipStream_t st)
{
	const size_t rchunk = scan_chunk(h, dbpv, n);
	for (size_t off = 0; off < n; off += rchunk) {
		const int rc = copy_rows_h2d(dst + off * dbpv, dbpv, packed + off * bpv, bpv, std::min(rchunk, n - off), st);
		if (rc) return rc;
	}
	return SGX_OK;
}

// the head of the checks of the entries for binary traits; what: "the Firth fit", "the exact test"
static int binary_check(const sgx_handle *h, const char *who, const char *what)
{
	if (!h) return fail(SGX_EINVAL, "%s: NULL handle", who);
	if (h->owner) return fail(SGX_EINVAL, "%s: not on a twin", who);
	if (h->md.quant) return fail(SGX_EINVAL, "%s: %s is for binary traits", who, what);
	return SGX_OK;
}

// after the entry's own check: M rows, their tables and their out4 in device memory; nothing is asked of no rows
static int out4_dev_check(sgx_handle *h, const char *who, const uint8_t *packed_dev, size_t bpv, size_t M,
	const double *lut_dev, const double *out4_dev)
{
	if (M == 0) return SGX_OK;
	if (!packed_dev || !lut_dev || !out4_dev) return fail(SGX_EINVAL, "%s: NULL buffer", who);
	int rc = dev_rows_check(who, packed_dev, bpv, h->md.N);
	if (rc) return rc;
	if (((uintptr_t)lut_dev & 7u) != 0 || ((uintptr_t)out4_dev & 7u) != 0)
		return fail(SGX_EINVAL, "%s: lut_dev and out4_dev must be 8-byte aligned", who);
	return set_dev(h);
}
