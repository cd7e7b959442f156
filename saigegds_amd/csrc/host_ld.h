// host_ld.h -- the LD handle (kern_ld.h): pair counts of host rows, and the pruning pass's resident
// block of candidates against a ring of kept rows.
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.

#define LD_WINDOW_BYTES ((size_t)8 << 30)     /* the ring's default byte budget                       */
#define LD_MIN_WAVES 4096                     /* the samples are cut into slabs until a call has these */

struct sgx_ld {
	int device = 0;
	int n_samp = 0;
	size_t bpv = 0, nb = 0, stride = 0;       // the caller's row stride, ceil(n_samp / 4), the device's (whole units)
	int n_units = 0;
	size_t max_rows = 0;                      // rows the ring may grow to
	DevStream stream;
	DevEvent ev0, ev1;
	DevBuf<uint8_t> blk, win, ca, cb, flags;
	DevBuf<int> sums, idx;
	int blk_m = 0;                            // rows of the resident block
	size_t head = 0, W = 0, cap = 0;          // the ring: first row, rows held, rows of room
	double ms = 0;
};

extern "C" int sgx_ld_create(int device, int32_t n_samp, size_t bytes_per_variant, size_t window_bytes, sgx_ld **out)
{
	if (!out) return fail(SGX_EINVAL, "sgx_ld_create: NULL argument");
	*out = nullptr;
	if (n_samp < 1 || n_samp >= (1 << 29)) return fail(SGX_EINVAL, "sgx_ld_create: n_samp = %d outside [1, 2^29)", n_samp);
	if (bytes_per_variant < ((size_t)n_samp + 3) / 4)
		return fail(SGX_EINVAL, "Invalid length of dosages: bytes_per_variant=%zu < ceil(N/4)", bytes_per_variant);
	HIPCHK(hipSetDevice(device));
	std::unique_ptr<sgx_ld> l(new sgx_ld);
	l->device = device;
	l->n_samp = n_samp;
	l->bpv = bytes_per_variant;
	l->nb = ((size_t)n_samp + 3) / 4;
	l->n_units = (int)(((size_t)n_samp + LD_UNIT - 1) / LD_UNIT);
	l->stride = (size_t)l->n_units * (LD_UNIT / 4);
	l->max_rows = std::max<size_t>(1, (window_bytes ? window_bytes : LD_WINDOW_BYTES) / l->stride);
	HIPCHK(l->stream.create(hipStreamNonBlocking));
	HIPCHK(l->ev0.create());
	HIPCHK(l->ev1.create());
	int rc = dev_room(l->blk, (size_t)SGX_LD_BLOCK * l->stride, "the candidate block", "sgx_ld_create");
	if (rc) return rc;
	*out = l.release();
	return SGX_OK;
}

extern "C" void sgx_ld_free(sgx_ld *l)
{
	if (!l) return;
	(void)hipSetDevice(l->device);
	if (l->stream) (void)hipStreamSynchronize(l->stream);
	delete l;
}

// m host rows -> canonical device rows at dst (kern_ld.h): bytes past ceil(n_samp / 4) and the last byte's unused
// fields become code 3, whatever the caller's hold
static int ld_upload(sgx_ld *l, uint8_t *dst, const uint8_t *rows, size_t m)
{
	HIPCHK(hipMemsetAsync(dst, 0xFF, m * l->stride, l->stream));
	HIPCHK(hipMemcpy2DAsync(dst, l->stride, rows, l->bpv, l->nb, m, hipMemcpyHostToDevice, l->stream));
	hipLaunchKernelGGL(ld_tail_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, l->stream, dst, l->stride, (int)m,
		l->n_samp);
	HIPCHK(hipGetLastError());
	return SGX_OK;
}

// the sums of ma rows of A against mb rows of B (a ring: b_head, b_cap) into out[i][col0 + j][6], added to what is there
static int ld_launch(sgx_ld *l, const uint8_t *A, int ma, const uint8_t *B, int mb, size_t b_head, size_t b_cap, int lower,
	int *out, int ldo, int col0)
{
	const unsigned gx = (unsigned)((mb + LD_TILE * LD_WAVES - 1) / (LD_TILE * LD_WAVES));
	const unsigned gy = (unsigned)((ma + LD_TILE - 1) / LD_TILE);
	const size_t waves = (size_t)gx * LD_WAVES * gy;
	int slabs = (int)std::min<size_t>((size_t)l->n_units, std::max<size_t>(1, LD_MIN_WAVES / waves));
	slabs = std::min(slabs, 65535);
	const int per = (l->n_units + slabs - 1) / slabs;
	slabs = (l->n_units + per - 1) / per;
	hipLaunchKernelGGL(ld_counts_kernel, dim3(gx, gy, (unsigned)slabs), dim3(64 * LD_WAVES), 0, l->stream, A, ma, B, mb,
		(int)b_head, (int)b_cap, l->stride, l->n_units, per, lower, out, ldo, col0);
	HIPCHK(hipGetLastError());
	return SGX_OK;
}

static int ld_done(sgx_ld *l)
{
	HIPCHK(hipStreamSynchronize(l->stream));
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, l->ev0, l->ev1));
	l->ms = ms;
	return SGX_OK;
}

extern "C" int sgx_ld_counts_2bit(sgx_ld *l, const uint8_t *a, size_t ma, const uint8_t *b, size_t mb, int32_t *out)
{
	if (!l) return fail(SGX_EINVAL, "sgx_ld_counts_2bit: NULL handle");
	if (ma == 0 || mb == 0) return SGX_OK;
	if (!a || !b || !out) return fail(SGX_EINVAL, "sgx_ld_counts_2bit: NULL buffer");
	if (ma > SGX_LD_MAX_ROWS || mb > SGX_LD_MAX_ROWS)
		return fail(SGX_EINVAL, "sgx_ld_counts_2bit: %zu x %zu rows, at most %d a side", ma, mb, SGX_LD_MAX_ROWS);
	HIPCHK(hipSetDevice(l->device));
	l->ms = 0;
	int rc;
	if ((rc = dev_room(l->ca, ma * l->stride, "the rows of a", "sgx_ld_counts_2bit"))) return rc;
	if ((rc = dev_room(l->cb, mb * l->stride, "the rows of b", "sgx_ld_counts_2bit"))) return rc;
	if ((rc = dev_room(l->sums, ma * mb * 6, "the sums", "sgx_ld_counts_2bit"))) return rc;
	if ((rc = ld_upload(l, l->ca, a, ma))) return rc;
	if ((rc = ld_upload(l, l->cb, b, mb))) return rc;
	HIPCHK(hipMemsetAsync(l->sums, 0, ma * mb * 6 * sizeof(int), l->stream));
	HIPCHK(hipEventRecord(l->ev0, l->stream));
	if ((rc = ld_launch(l, l->ca, (int)ma, l->cb, (int)mb, 0, mb, 0, l->sums, (int)mb, 0))) return rc;
	HIPCHK(hipEventRecord(l->ev1, l->stream));
	HIPCHK(hipMemcpyAsync(out, l->sums, ma * mb * 6 * sizeof(int), hipMemcpyDeviceToHost, l->stream));
	return ld_done(l);
}

extern "C" int sgx_ld_block_2bit(sgx_ld *l, const uint8_t *rows, size_t mb, double t2, uint8_t *flags)
{
	if (!l) return fail(SGX_EINVAL, "sgx_ld_block_2bit: NULL handle");
	if (!rows || !flags) return fail(SGX_EINVAL, "sgx_ld_block_2bit: NULL buffer");
	if (mb < 1 || mb > SGX_LD_BLOCK) return fail(SGX_EINVAL, "sgx_ld_block_2bit: %zu rows, 1 to %d a block", mb, SGX_LD_BLOCK);
	if (!(t2 >= 0.0)) return fail(SGX_EINVAL, "sgx_ld_block_2bit: t2 = %g", t2);
	HIPCHK(hipSetDevice(l->device));
	l->ms = 0;
	const size_t W = l->W, ld = W + mb, n_pairs = mb * ld;
	int rc;
	if ((rc = dev_room(l->sums, n_pairs * 6, "the sums", "sgx_ld_block_2bit"))) return rc;
	if ((rc = dev_room(l->flags, n_pairs, "the flags", "sgx_ld_block_2bit"))) return rc;
	l->blk_m = 0;                                  // (the block is not valid until its upload is queued)
	if ((rc = ld_upload(l, l->blk, rows, mb))) return rc;
	l->blk_m = (int)mb;
	HIPCHK(hipMemsetAsync(l->sums, 0, n_pairs * 6 * sizeof(int), l->stream));
	HIPCHK(hipEventRecord(l->ev0, l->stream));
	if (W && (rc = ld_launch(l, l->blk, (int)mb, l->win, (int)W, l->head, l->cap, 0, l->sums, (int)ld, 0))) return rc;
	if (mb > 1 && (rc = ld_launch(l, l->blk, (int)mb, l->blk, (int)mb, 0, SGX_LD_BLOCK, 1, l->sums, (int)ld, (int)W))) return rc;
	hipLaunchKernelGGL(ld_flags_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, l->stream, l->sums, n_pairs,
		t2, l->flags);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(l->ev1, l->stream));
	HIPCHK(hipMemcpyAsync(flags, l->flags, n_pairs, hipMemcpyDeviceToHost, l->stream));
	return ld_done(l);
}

extern "C" int sgx_ld_window_push(sgx_ld *l, const int32_t *keep_idx, size_t n_keep, size_t drop_oldest)
{
	const char *who = "sgx_ld_window_push";
	if (!l) return fail(SGX_EINVAL, "%s: NULL handle", who);
	if (n_keep && !keep_idx) return fail(SGX_EINVAL, "%s: NULL buffer", who);
	if (drop_oldest > l->W) return fail(SGX_EINVAL, "%s: drop_oldest = %zu of %zu rows", who, drop_oldest, l->W);
	if (n_keep > (size_t)l->blk_m) return fail(SGX_EINVAL, "%s: %zu rows of a block of %d", who, n_keep, l->blk_m);
	for (size_t k = 0; k < n_keep; k++)
		if (keep_idx[k] < 0 || keep_idx[k] >= l->blk_m || (k && keep_idx[k] <= keep_idx[k - 1]))
			return fail(SGX_EINVAL, "%s: keep_idx must ascend within the block's %d rows", who, l->blk_m);
	HIPCHK(hipSetDevice(l->device));
	const size_t W = l->W - drop_oldest, need = W + n_keep;
	if (need > l->max_rows)
		return fail(SGX_ENOMEM, "%s: a window of %zu rows is over the budget of %zu rows", who, need, l->max_rows);
	int rc;
	if (n_keep && (rc = dev_room(l->idx, SGX_LD_BLOCK, "the row indices", who))) return rc;
	if (need > l->cap) {
		// Grow by doubling.  ALL rows the ring holds move to the front of the new one in their order (up to two pieces
		// when the ring is wrapped), so the window is the same window in a new place; the drop comes below, with the
		// append.  Nothing is in flight: every entry ends with a synchronisation.
		size_t cap = std::max<size_t>(l->cap, SGX_LD_BLOCK);
		while (cap < need) cap *= 2;
		cap = std::max(std::min(cap, l->max_rows), l->W);
		DevBuf<uint8_t> nw;
		if ((rc = dev_room(nw, cap * l->stride, "the window", who))) return rc;
		const size_t first = l->cap ? std::min(l->W, l->cap - l->head) : 0;
		if (first)
			HIPCHK(hipMemcpyAsync(nw, l->win + l->head * l->stride, first * l->stride, hipMemcpyDeviceToDevice, l->stream));
		if (l->W > first)
			HIPCHK(hipMemcpyAsync(nw + first * l->stride, l->win, (l->W - first) * l->stride, hipMemcpyDeviceToDevice, l->stream));
		HIPCHK(hipStreamSynchronize(l->stream));
		l->win = std::move(nw);
		l->cap = cap;
		l->head = 0;
	}
	// head and W change only once the append is done
	const size_t head = l->cap ? (l->head + drop_oldest) % l->cap : 0;
	if (n_keep) {
		HIPCHK(hipMemcpyAsync(l->idx, keep_idx, n_keep * sizeof(int), hipMemcpyHostToDevice, l->stream));
		const unsigned gx = (unsigned)std::min<size_t>(64, (l->stride / 16 + 255) / 256);
		hipLaunchKernelGGL(ld_push_kernel, dim3(gx, (unsigned)n_keep), dim3(256), 0, l->stream, l->blk, l->idx, l->win,
			head + W, l->cap, l->stride);
		HIPCHK(hipGetLastError());
		HIPCHK(hipStreamSynchronize(l->stream));
	}
	l->head = head;
	l->W = need;
	return SGX_OK;
}

extern "C" int sgx_ld_window_reset(sgx_ld *l)
{
	if (!l) return fail(SGX_EINVAL, "sgx_ld_window_reset: NULL handle");
	l->head = l->W = 0;
	return SGX_OK;
}

extern "C" int64_t sgx_ld_window_len(const sgx_ld *l) { return l ? (int64_t)l->W : -1; }

extern "C" int sgx_ld_kernel_ms(sgx_ld *l, double *ms_out)
{
	if (!l || !ms_out) return fail(SGX_EINVAL, "sgx_ld_kernel_ms: NULL argument");
	*ms_out = l->ms;
	return SGX_OK;
}
