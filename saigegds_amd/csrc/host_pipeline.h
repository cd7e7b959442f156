// host_pipeline.h -- host-buffer scans: the PCIe pipeline, block loads from host rows, dosage inputs, burden rows.
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.

static const size_t STAGE_BYTES = (size_t)1 << 30;    // burden rows are made and scanned in chunks of this size

static int ensure_stage(sgx_handle *h, size_t in_bytes, size_t M)
{
	int rc = grow(h->stage_in, in_bytes);
	if (!rc) rc = grow(h->stage_out, M * 8);
	if (!rc) rc = grow(h->stage_valid, M);
	return rc;
}

// launch_scan of m rows on the device, the table and the flags to the caller's out8 / valid through the stage's
// result buffers, the call's statistics added to total; returns when they are home
template <int INPUT>
static int scan_staged(sgx_handle *h, const void *rows, size_t row_bytes, size_t m, double *out8, uint8_t *valid, sgx_stats &total)
{
	int rc = launch_scan<INPUT>(h, rows, row_bytes, m, h->stage_out, h->stage_valid);
	if (rc) return rc;
	HIPCHK(hipMemcpyAsync(out8, h->stage_out, m * 8 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipMemcpyAsync(valid, h->stage_valid, m, hipMemcpyDeviceToHost, h->stream));
	rc = sgx_sync(h);
	if (rc) return rc;
	stats_add(total, h->stats);
	return SGX_OK;
}

// the CSR arguments of the burden calls (name: "row_ptr" / "grp_ptr"): ptr[0] = 0, ascending, every index below
// limit.  *bad: the first index out of range, which the caller reports in its own words, else nullptr
static int csr_check(const char *who, const char *name, size_t n, const int64_t *ptr, const int32_t *idx, size_t limit, const int32_t **bad)
{
	const int64_t nnz = ptr[n];
	if (ptr[0] != 0 || nnz < 0) return fail(SGX_EINVAL, "%s: bad %s", who, name);
	for (size_t r = 0; r < n; r++)
		if (ptr[r + 1] < ptr[r]) return fail(SGX_EINVAL, "%s: %s not ascending", who, name);
	*bad = nullptr;
	for (int64_t e = 0; e < nnz && !*bad; e++)
		if (idx[e] < 0 || (size_t)idx[e] >= limit) *bad = idx + e;
	return SGX_OK;
}

// m host rows of src_stride bytes -> device rows of dst_stride bytes (what a wider device row has more is zeroed)
static int copy_rows_h2d(uint8_t *dst, size_t dst_stride, const uint8_t *src, size_t src_stride, size_t m, hipStream_t st)
{
	if (src_stride == dst_stride) {
		HIPCHK(hipMemcpyAsync(dst, src, m * dst_stride, hipMemcpyHostToDevice, st));
		return SGX_OK;
	}
	if (dst_stride > src_stride) HIPCHK(hipMemsetAsync(dst, 0, m * dst_stride, st));
	HIPCHK(hipMemcpy2DAsync(dst, dst_stride, src, src_stride, std::min(src_stride, dst_stride), m, hipMemcpyHostToDevice, st));
	return SGX_OK;
}

// ---------------------------------------------------------------------------
// Host rows to the device (the buffers: host_state.h): chunk i + 1 crosses PCIe on the copy stream while
// chunk i is read on the handle's stream.  Scans (scan_host) bring results back through pinned memory, so no copy of
// the caller's pageable buffers ever waits for a kernel; loaders (ingest) leave the rows on the device.  RAW / INTEGER
// dosages that are hard calls (0, 1, 2, missing) are packed to 2-bit rows on the device (kern_pack.h) and take the MFMA path.
enum { IN_I32 = 3 };
static const size_t PIPE_BYTES = (size_t)512 << 20;      // device bytes of one chunk's input rows ("pipe_mb" option)

static size_t pipe_budget(const sgx_handle *h) { return h->pipe_bytes ? h->pipe_bytes : PIPE_BYTES; }

// Rows per chunk of a scan of M rows that take per_row device bytes each.  scan_host and sgx_dsblock_scan both cut
// here: the tiled score kernel splits the samples by the number of rows of a launch, so the same chunks give the same
// sums, and the scan of a dosage block equals the host-buffer scan of the same rows bit for bit.
static size_t scan_chunk(const sgx_handle *h, size_t per_row, size_t M)
{
	return std::min(M, std::max<size_t>(1, pipe_budget(h) / per_row));
}

// rows per chunk of a block load of M rows of dev_row bytes: a multiple of 16 (block_put_rows' v_first), at least 16
static size_t load_chunk(const sgx_handle *h, size_t dev_row, size_t M)
{
	return std::min(std::max<size_t>(16, (pipe_budget(h) / dev_row) & ~(size_t)15), (M + 15) & ~(size_t)15);
}

static int ensure_pipe(sgx_handle *h, size_t in_bytes, size_t pk_bytes, size_t M)
{
	if (!h->cstream) {
		HIPCHK(h->cstream.create(hipStreamNonBlocking));
		HIPCHK(h->ev_h2d.create(hipEventDisableTiming));
		for (int k = 0; k < 2; k++) { HIPCHK(h->ev_copy[k].create(hipEventDisableTiming)); HIPCHK(h->ev_done[k].create(hipEventDisableTiming)); }
		HIPCHK(h->pipe_flag.alloc(1));
		HIPCHK(h->h_pipe_flag.alloc(1));
	}
	int rc = SGX_OK;
	for (int b = 0; b < 2 && !rc; b++) {
		rc = grow(h->pipe_in[b], in_bytes);
		if (!rc) rc = grow(h->pipe_pk[b], pk_bytes);
		if (!rc) rc = grow(h->pipe_out[b], M * 8);
		if (!rc) rc = grow(h->pipe_valid[b], M);
		if (!rc) rc = grow(h->pin_out[b], M * 8);
		if (!rc) rc = grow(h->pin_valid[b], M);
	}
	return rc;
}

// ---------------------------------------------------------------------------
// Where the rows of a call come from.
//  SRC_ROWS    rows the kernels read as they are (2-bit, u8, i32, f64), row_bytes apart in the caller's buffer.
//  SRC_PACKED  packed-real rows (kern_unpack.h): they cross PCIe as the file stores them -- 1, 2 or 4 bytes a sample,
//              the file's samples in the file's order -- and are decoded and sample-selected on the device into the
//              float64 rows the dosage kernels read.
//  SRC_DBIT2   genotype/data rows (kern_dbit2.h): the dBit2 allele codes cross PCIe as the file stores them -- 4 bits a
//              sample, the file's samples in the file's order, rows back to back in one bit stream -- and are folded
//              into 2-bit dosage rows and sample-selected on the device.
enum SrcKind { SRC_ROWS, SRC_PACKED, SRC_DBIT2 };
struct RowSrc {
	SrcKind kind = SRC_ROWS;
	const uint8_t *rows = nullptr;    // the caller's buffer
	size_t row_bytes = 0;             // SRC_ROWS, SRC_PACKED: of a row of it
	size_t nfs = 0;                   // stored rows: samples per row of the file
	const int32_t *sel = nullptr;     // ... the model's samples among them, or nullptr: the file's samples as they are
	const int *sel_dev = nullptr;     // ... its device copy (h->pk_sel), made by src_prepare
	int cls = 0;                      // SRC_PACKED: SGX_PR_*, bytes per value, value = raw * scale + offset
	size_t esz = 0;
	double scale = 1, offset = 0;
	size_t nib0 = 0;                  // SRC_DBIT2: nibble of the first byte the first row starts at
	std::vector<unsigned> row0;       // [M + 1] row offsets where a variant of the call has more than one row, else empty
	const unsigned *row0_dev = nullptr;   // ... its device copy (h->db2_row0)
	size_t row_of(size_t j) const { return row0.empty() ? j : row0[j]; }
	// SRC_DBIT2, variants [off, off + m): the bytes that hold them, the nibble of the first byte they start at
	void span(size_t off, size_t m, size_t &byte0, size_t &bytes, unsigned &nib) const
	{
		const size_t a = nib0 + row_of(off) * nfs, b = nib0 + row_of(off + m) * nfs;
		byte0 = a >> 1; bytes = ((b + 1) >> 1) - byte0; nib = (unsigned)(a & 1);
	}
};

static RowSrc plain_rows(const void *rows, size_t row_bytes)
{
	RowSrc s;
	s.rows = reinterpret_cast<const uint8_t *>(rows); s.row_bytes = row_bytes;
	return s;
}

static size_t packed_esz(int cls)
{
	return cls == SGX_PR_U8 || cls == SGX_PR_I8 ? 1 : cls == SGX_PR_U16 || cls == SGX_PR_I16 ? 2 : cls == SGX_PR_F32 ? 4 : 0;
}

// the model's N samples among the nfs of the file
static int sel_check(const char *who, int N, size_t nfs, const int32_t *sel)
{
	if (nfs < (size_t)N) return fail(SGX_EINVAL, "%s: n_file_samp = %zu < %d samples of the model", who, nfs, N);
	if (!sel && nfs != (size_t)N)
		return fail(SGX_EINVAL, "%s: n_file_samp = %zu but the model has %d samples and there is no selection", who, nfs, N);
	if (sel) for (int i = 0; i < N; i++)
		if (sel[i] < 0 || (size_t)sel[i] >= nfs)
			return fail(SGX_EINVAL, "%s: sample index %d outside the file's %zu samples", who, sel[i], nfs);
	return SGX_OK;
}

// the argument checks of sgx_scan_packed / sgx_ds_block_load_packed, and their source: nothing is launched on a bad argument
static int packed_check(const char *who, int N, const void *raw, int cls, size_t nfs, double scale, double offset,
	const int32_t *sel, RowSrc &src)
{
	if (!packed_esz(cls)) return fail(SGX_EINVAL, "%s: unknown class %d", who, cls);
	if (!raw) return fail(SGX_EINVAL, "%s: NULL buffer", who);
	int rc = sel_check(who, N, nfs, sel);
	if (rc) return rc;
	src = plain_rows(raw, nfs * packed_esz(cls));
	src.kind = SRC_PACKED; src.nfs = nfs; src.sel = sel;
	src.cls = cls; src.esz = packed_esz(cls); src.scale = scale; src.offset = offset;
	return SGX_OK;
}

#define SGX_DBIT2_MAX_ROWS 16     /* rows of one variant: allele indices below 4^16 */

// the same of sgx_scan_dbit2 / sgx_block_load_dbit2
static int dbit2_check(const char *who, int N, const uint8_t *alleles, size_t bit0, size_t nfs, const int32_t *n_rows,
	const int32_t *sel, size_t M, RowSrc &src)
{
	if (!alleles) return fail(SGX_EINVAL, "%s: NULL buffer", who);
	if (bit0 != 0 && bit0 != 4) return fail(SGX_EINVAL, "%s: bit0 = %zu, must be 0 or 4", who, bit0);
	int rc = sel_check(who, N, nfs, sel);
	if (rc) return rc;
	if (M > 0xFFFFFFFFu / SGX_DBIT2_MAX_ROWS) return fail(SGX_EINVAL, "%s: too many variants in one call", who);
	bool multi = false;
	if (n_rows) for (size_t j = 0; j < M; j++) {
		if (n_rows[j] < 1 || n_rows[j] > SGX_DBIT2_MAX_ROWS)
			return fail(SGX_EINVAL, "%s: n_rows[%zu] = %d, a variant has 1 to %d rows", who, j, n_rows[j], SGX_DBIT2_MAX_ROWS);
		multi |= n_rows[j] > 1;
	}
	src = plain_rows(alleles, 0);
	src.kind = SRC_DBIT2; src.nfs = nfs; src.sel = sel; src.nib0 = bit0 / 4;
	if (multi) {
		src.row0.resize(M + 1);
		src.row0[0] = 0;
		for (size_t j = 0; j < M; j++) src.row0[j + 1] = src.row0[j] + (unsigned)n_rows[j];
	}
	return SGX_OK;
}

// What a stored source needs on the device for chunks of `chunk` of its M rows: the two raw buffers, and on the copy
// stream, ahead of the chunks, the call's selection and row offsets (src outlives the call's chunks)
static int src_prepare(sgx_handle *h, RowSrc &src, size_t M, size_t chunk)
{
	if (src.kind == SRC_ROWS) return SGX_OK;
	size_t need = chunk * src.row_bytes;
	if (src.kind == SRC_DBIT2) for (size_t off = 0; off < M; off += chunk) {
		size_t byte0, bytes; unsigned nib;
		src.span(off, std::min(chunk, M - off), byte0, bytes, nib);
		need = std::max(need, bytes);
	}
	int rc = grow(h->pipe_raw[0], need);
	if (!rc) rc = grow(h->pipe_raw[1], need);
	if (rc) return rc;
	src.sel_dev = nullptr; src.row0_dev = nullptr;
	if (src.sel) {
		const size_t N = (size_t)h->md.N;
		rc = grow(h->pk_sel, N);
		if (rc) return rc;
		static_assert(sizeof(int) == sizeof(int32_t), "sel");
		HIPCHK(hipMemcpyAsync(h->pk_sel, src.sel, N * sizeof(int), hipMemcpyHostToDevice, h->cstream));
		src.sel_dev = h->pk_sel;
	}
	if (!src.row0.empty()) {
		rc = grow(h->db2_row0, M + 1);
		if (rc) return rc;
		HIPCHK(hipMemcpyAsync(h->db2_row0, src.row0.data(), (M + 1) * sizeof(unsigned), hipMemcpyHostToDevice, h->cstream));
		src.row0_dev = h->db2_row0;
	}
	return SGX_OK;
}

// rows [off, off + m) of a stored source, as stored, to raw buffer k on the copy stream
static int copy_raw(sgx_handle *h, const RowSrc &src, int k, size_t off, size_t m)
{
	size_t byte0 = off * src.row_bytes, bytes = m * src.row_bytes; unsigned nib;
	if (src.kind == SRC_DBIT2) src.span(off, m, byte0, bytes, nib);
	HIPCHK(hipMemcpyAsync(h->pipe_raw[k], src.rows + byte0, bytes, hipMemcpyHostToDevice, h->cstream));
	return SGX_OK;
}

// m packed-real rows in raw_dev -> float64 rows of N samples
static int launch_unpack(hipStream_t st, const RowSrc &pk, const void *raw_dev, int N, size_t m, double *out)
{
	// a thread: one sample of up to 4 rows (selection) or one 16-byte load of up to 4 rows
	const size_t per_thread = pk.sel_dev ? 1 : 16 / pk.esz, items = ((size_t)N + per_thread - 1) / per_thread + 1;
	const dim3 g((unsigned)std::min<size_t>((items + 255) / 256, 4096), (unsigned)std::min<size_t>((m + 3) / 4, 65535));
#define SGX_UNPACK(T) hipLaunchKernelGGL((unpack_real_rows<T>), g, dim3(256), 0, st, \
		(const T *)raw_dev, pk.nfs, pk.sel_dev, N, m, pk.scale, pk.offset, out)
	switch (pk.cls) {
	case SGX_PR_U8: SGX_UNPACK(uint8_t); break;
	case SGX_PR_I8: SGX_UNPACK(int8_t); break;
	case SGX_PR_U16: SGX_UNPACK(uint16_t); break;
	case SGX_PR_I16: SGX_UNPACK(int16_t); break;
	default: SGX_UNPACK(float); break;
	}
#undef SGX_UNPACK
	HIPCHK(hipGetLastError());
	return SGX_OK;
}

// variants [off, off + m) of the call from their raw bytes on the device -> m rows of out_stride bytes
static int launch_dbit2(hipStream_t st, const RowSrc &db, const uint8_t *raw_dev, size_t off, size_t m, int N, uint8_t *out, size_t out_stride)
{
	size_t byte0, bytes; unsigned nib;
	db.span(off, m, byte0, bytes, nib);
	// a thread: one output dword of the variants of its stride (selection) or 8 output bytes of one variant
	const size_t items = out_stride / (db.sel_dev ? 4 : 8);
	const dim3 g((unsigned)std::min<size_t>((items + 255) / 256, 4096), (unsigned)std::min<size_t>(m, db.sel_dev ? 64 : 65535));
	hipLaunchKernelGGL(decode_dbit2_rows, g, dim3(256), 0, st, raw_dev, bytes, nib, db.nfs,
		db.row0_dev ? db.row0_dev + off : (const unsigned *)nullptr, (unsigned)db.row_of(off), db.sel_dev, N, m, out, out_stride);
	HIPCHK(hipGetLastError());
	return SGX_OK;
}

// The two operations of a source on chunk [off, off + m) and pipeline buffer b (rows of dev_row bytes in pipe_in[b]).
// On the copy stream: plain rows to pipe_in[b]; packed-real rows to pipe_raw[b] and decoded into pipe_in[b] there (the
// dosage-block loader decodes on its compute stream and calls copy_raw itself); dBit2 bytes to pipe_raw[b], still raw.
static int src_upload(sgx_handle *h, const RowSrc &src, int b, size_t off, size_t m, size_t dev_row)
{
	if (src.kind == SRC_ROWS) return copy_rows_h2d(h->pipe_in[b], dev_row, src.rows + off * src.row_bytes, src.row_bytes, m, h->cstream);
	int rc = copy_raw(h, src, b, off, m);
	if (rc || src.kind == SRC_DBIT2) return rc;
	return launch_unpack(h->cstream, src, h->pipe_raw[b], h->md.N, m, reinterpret_cast<double *>(h->pipe_in[b].p));
}

// On the compute stream, behind the upload: dBit2 bytes -> the 2-bit rows of pipe_in[b] (the link goes on with the next
// chunk meanwhile); nothing for the other kinds.
static int src_finish(sgx_handle *h, const RowSrc &src, int b, size_t off, size_t m, size_t dev_row)
{
	if (src.kind != SRC_DBIT2) return SGX_OK;
	return launch_dbit2(h->stream, src, h->pipe_raw[b], off, m, h->md.N, h->pipe_in[b], dev_row);
}

// The loaders' loop: chunks [off, off + m) of M rows through the pipeline's two buffers.  upload(k, off, m) issues on
// the copy stream what brings the chunk into buffer k, consume(k, off, m) on the handle's stream what reads it from
// there; the copy into a buffer waits for the consumer of the chunk before last.  Returns when the last chunk has left
// the caller's memory (the consumers may still be running).
template <class Upload, class Consume>
static int ingest(sgx_handle *h, size_t M, size_t chunk, Upload upload, Consume consume)
{
	int i = 0;
	for (size_t off = 0; off < M; off += chunk, i++) {
		const size_t m = std::min(chunk, M - off);
		const int k = i & 1;
		if (i >= 2) HIPCHK(hipStreamWaitEvent(h->cstream, h->ev_done[k], 0));      // the buffer's previous chunk has been read
		int rc = upload(k, off, m);
		if (rc) return rc;
		HIPCHK(hipEventRecord(h->ev_copy[k], h->cstream));
		HIPCHK(hipStreamWaitEvent(h->stream, h->ev_copy[k], 0));      // (what src_prepare sent went first on the same stream)
		rc = consume(k, off, m);
		if (rc) return rc;
		HIPCHK(hipEventRecord(h->ev_done[k], h->stream));
	}
	HIPCHK(hipStreamSynchronize(h->cstream));
	return SGX_OK;
}

// The scans' loop: as ingest, with the results of chunk i - 1 collected between the upload of chunk i and its compute.
// dev_row_bytes: of a row in pipe_in -- as it arrives (SRC_ROWS), of the float64 rows packed-real rows become, of the
// 2-bit rows genotype/data rows become.
template <int INPUT>
static int scan_host(sgx_handle *h, RowSrc &src, size_t dev_row_bytes, size_t M, double *out8, uint8_t *valid)
{
	if (!h) return fail(SGX_EINVAL, "scan: NULL handle");
	if (M == 0) return SGX_OK;
	if (!src.rows || !out8 || !valid) return fail(SGX_EINVAL, "scan: NULL buffer");
	if (src.kind == SRC_DBIT2 && dev_row_bytes % 8 != 0) return fail(SGX_EINVAL, "scan: row stride %zu", dev_row_bytes);
	int rc = set_dev(h);
	if (rc) return rc;
	rc = sync_lane(h);                        // anything queued on this handle before is done
	if (rc) return rc;
	h->last_issued = h;                       // sgx_get_stats: this call, not an earlier one on the twin lane
	const int N = h->md.N;
	const size_t pk_row = sgx_row_stride(N);
	const bool can_pack = (INPUT == IN_U8 || INPUT == IN_I32) && h->mf_ok && !h->force_v1;
	// a chunk's rows on the device: as they arrive (+ the doubles INTEGER rows may have to become)
	size_t chunk = scan_chunk(h, dev_row_bytes + (INPUT == IN_I32 ? (size_t)N * sizeof(double) : 0), M);
	if (can_pack) chunk = std::min<size_t>(chunk, 65535);       // pack_rows_2bit: grid.y = rows
	const size_t f64_off = (chunk * dev_row_bytes + 15) & ~(size_t)15;   // INTEGER rows that are not hard calls: their doubles
	rc = ensure_pipe(h, f64_off + (INPUT == IN_I32 ? chunk * (size_t)N * sizeof(double) : 0), can_pack ? chunk * pk_row : 0, chunk);
	if (rc) return rc;
	rc = ensure_recs(h, chunk);
	if (rc) return rc;
	rc = src_prepare(h, src, M, chunk);
	if (rc) return rc;
	// 2-bit rows (as they come, or packed from hard calls) take the MFMA path, the lists of a chunk per pipeline buffer
	const bool blocks = (INPUT == IN_2BIT || can_pack) && h->mf_ok && !h->force_v1;
	if (blocks) for (int b = 0; b < 2; b++) { rc = ensure_tmp_block(h, b, chunk); if (rc) return rc; }
	sgx_stats total{};
	auto harvest = [&](size_t off, size_t m, int b) -> int {       // chunk [off, off + m) of buffer b is done
		int r2 = sync_lane(h);
		if (r2) return r2;
		memcpy(out8 + off * 8, h->pin_out[b], m * 8 * sizeof(double));
		memcpy(valid + off, h->pin_valid[b], m);
		const uint32_t three_plane = std::max(total.three_plane, h->stats.three_plane);   // (any chunk)
		stats_add(total, h->stats);
		total.three_plane = three_plane;
		return SGX_OK;
	};
	size_t prev_off = 0, prev_m = 0;
	int i = 0;
	for (size_t off = 0; off < M; off += chunk, i++) {
		const size_t m = std::min(chunk, M - off);
		const int b = i & 1;
		// ---- chunk i over PCIe on the copy stream (buffer b was last used by chunk i - 2: done)
		if (i >= 2 && src.kind == SRC_DBIT2) HIPCHK(hipStreamWaitEvent(h->cstream, h->ev_done[b], 0));   // pipe_raw[b]'s reader, the decoder, ran on the compute stream
		rc = src_upload(h, src, b, off, m, dev_row_bytes);
		if (rc) return rc;
		bool packed_ok = false;
		if (can_pack) {
			HIPCHK(hipMemsetAsync(h->pipe_flag, 0, sizeof(int), h->cstream));
			const dim3 g((unsigned)std::min<size_t>(64, (pk_row / 4 + 255) / 256), (unsigned)m);
			if (INPUT == IN_U8)
				hipLaunchKernelGGL((pack_rows_2bit<uint8_t>), g, dim3(256), 0, h->cstream,
					(const uint8_t *)h->pipe_in[b], N, h->pipe_pk[b], pk_row, h->pipe_flag);
			else
				hipLaunchKernelGGL((pack_rows_2bit<int>), g, dim3(256), 0, h->cstream,
					(const int *)h->pipe_in[b].p, N, h->pipe_pk[b], pk_row, h->pipe_flag);
			HIPCHK(hipGetLastError());
			HIPCHK(hipMemcpyAsync(h->h_pipe_flag, h->pipe_flag, sizeof(int), hipMemcpyDeviceToHost, h->cstream));
			HIPCHK(hipStreamSynchronize(h->cstream));
			packed_ok = *h->h_pipe_flag == 0;
		}
		double *as_f64 = nullptr;
		if (INPUT == IN_I32 && !packed_ok) {
			as_f64 = reinterpret_cast<double *>(h->pipe_in[b] + f64_off);
			hipLaunchKernelGGL(i32_rows_to_f64, dim3(1024), dim3(256), 0, h->cstream,
				(const int *)h->pipe_in[b].p, m * (size_t)N, as_f64);
			HIPCHK(hipGetLastError());
		}
		const bool as_block = blocks && (INPUT == IN_2BIT || packed_ok);
		HIPCHK(hipEventRecord(h->ev_h2d, h->cstream));
		// ---- chunk i - 1 has been computing meanwhile: collect it
		if (prev_m) { rc = harvest(prev_off, prev_m, b ^ 1); if (rc) return rc; }
		// ---- compute chunk i, results to pinned memory.  The chunk's 2-bit rows go into the buffer's block on
		// the COMPUTE stream: on the copy stream the 2.5 ms of ingest sat between two 9.5-ms copies and the
		// link idled a fifth of the time (43 GB/s; the next copy now starts as this one ends).
		HIPCHK(hipStreamWaitEvent(h->stream, h->ev_h2d, 0));
		HIPCHK(hipStreamWaitEvent(h->hstream, h->ev_h2d, 0));
		rc = src_finish(h, src, b, off, m, dev_row_bytes);
		if (rc) return rc;
		if (src.kind == SRC_DBIT2) {
			// the score chain of a block scan runs on the lane's other stream and waits for the decoded rows
			HIPCHK(hipEventRecord(h->ev_done[b], h->stream));
			HIPCHK(hipStreamWaitEvent(h->hstream, h->ev_done[b], 0));
		}
		if (as_block) rc = scan_rows_dev(h, b, INPUT == IN_2BIT ? h->pipe_in[b] : h->pipe_pk[b], INPUT == IN_2BIT ? dev_row_bytes : pk_row, m,
			h->pipe_out[b], h->pipe_valid[b], false);
		else if (INPUT == IN_2BIT) rc = launch_scan<IN_2BIT>(h, h->pipe_in[b], dev_row_bytes, m, h->pipe_out[b], h->pipe_valid[b]);
		else if (packed_ok) rc = launch_scan<IN_2BIT>(h, h->pipe_pk[b], pk_row, m, h->pipe_out[b], h->pipe_valid[b]);
		else if (INPUT == IN_U8) rc = launch_scan<IN_U8>(h, h->pipe_in[b], dev_row_bytes, m, h->pipe_out[b], h->pipe_valid[b]);
		else if (INPUT == IN_I32) rc = launch_scan<IN_F64>(h, as_f64, (size_t)N * sizeof(double), m, h->pipe_out[b], h->pipe_valid[b]);
		else rc = launch_scan<IN_F64>(h, h->pipe_in[b], dev_row_bytes, m, h->pipe_out[b], h->pipe_valid[b]);
		if (rc) return rc;
		HIPCHK(hipMemcpyAsync(h->pin_out[b], h->pipe_out[b], m * 8 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
		HIPCHK(hipMemcpyAsync(h->pin_valid[b], h->pipe_valid[b], m, hipMemcpyDeviceToHost, h->stream));
		prev_off = off; prev_m = m;
	}
	rc = harvest(prev_off, prev_m, (i - 1) & 1);
	if (rc) return rc;
	h->stats = total;
	return SGX_OK;
}

// Page-locked host memory for the caller's block buffers: copies from it run at the full PCIe rate
// and truly asynchronously (a pageable source is staged by the runtime at ~50 GB/s).
extern "C" void *sgx_host_alloc(size_t bytes)
{
	void *p = nullptr;
	if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
		(void)fail(SGX_ENOMEM, "sgx_host_alloc: cannot pin %zu bytes", bytes);
		return nullptr;
	}
	return p;
}

extern "C" void sgx_host_free(void *p)
{
	if (p) (void)hipHostFree(p);
}

// Rows of M variants from src into a resident block: chunks cross PCIe on the copy stream while the previous chunk is
// being decoded (genotype/data rows) and rearranged on the handle's stream; the lists are made once at the end.
// Returns when the block is loaded: ready for sgx_scan_block on this handle (same stream).  Each chunk goes through
// the pipeline's input buffer and block_put_rows copies it into the block's rows in its one pass (decoding straight
// into the block's rows would have that pass read and write the same addresses).
static int block_load_host(sgx_handle *h, sgx_block *b, RowSrc &src, size_t M)
{
	int rc = set_dev(h);
	if (rc) return rc;
	const size_t dev_row = (size_t)b->ntile * 64, chunk = load_chunk(h, dev_row, M);
	rc = ensure_pipe(h, chunk * dev_row, 0, 1);
	if (rc) return rc;
	rc = src_prepare(h, src, M, chunk);
	if (rc) return rc;
	rc = block_begin_load(h, b, h->stream);
	if (rc) return rc;
	rc = ingest(h, M, chunk,
		[&](int k, size_t off, size_t m) -> int { return src_upload(h, src, k, off, m, dev_row); },
		[&](int k, size_t off, size_t m) -> int {
			int r2 = src_finish(h, src, k, off, m, dev_row);
			return r2 ? r2 : block_put_rows(b, h->pipe_in[k], dev_row, off, m, h->stream);
		});
	if (rc) return rc;                          // (the caller's buffers are free)
	rc = block_finish(b, M, h->stream);
	if (rc) return rc;
	HIPCHK(hipStreamSynchronize(h->stream));
	return SGX_OK;
}

extern "C" int sgx_block_load(sgx_handle *h, sgx_block *b, const uint8_t *packed, size_t bpv, size_t M)
{
	if (!h || !b) return fail(SGX_EINVAL, "sgx_block_load: NULL argument");
	if (!packed) return fail(SGX_EINVAL, "sgx_block_load: NULL buffer");
	if (b->lists_only) return fail(SGX_EINVAL, "sgx_block_load: not a resident block");
	if (b->device != h->device) return fail(SGX_EINVAL, "sgx_block_load: block and handle are on different devices");
	if (M == 0 || M > b->cap) return fail(SGX_EINVAL, "sgx_block_load: %zu variants, the block holds up to %zu", M, b->cap);
	const int rc = bpv_check(bpv, b->N);
	if (rc) return rc;
	RowSrc src = plain_rows(packed, bpv);
	return block_load_host(h, b, src, M);
}

// The same block from genotype/data rows as the file stores them, in sgx_block_load's chunks.
extern "C" int sgx_block_load_dbit2(sgx_handle *h, sgx_block *b, const uint8_t *alleles, size_t bit0, size_t n_file_samp,
	const int32_t *n_rows, const int32_t *sel, size_t M)
{
	if (!h || !b) return fail(SGX_EINVAL, "sgx_block_load_dbit2: NULL argument");
	if (b->lists_only) return fail(SGX_EINVAL, "sgx_block_load_dbit2: not a resident block");
	if (b->device != h->device) return fail(SGX_EINVAL, "sgx_block_load_dbit2: block and handle are on different devices");
	if (b->N != h->md.N) return fail(SGX_EINVAL, "sgx_block_load_dbit2: the block holds rows of %d samples, the model has %d", b->N, h->md.N);
	if (M == 0 || M > b->cap) return fail(SGX_EINVAL, "sgx_block_load_dbit2: %zu variants, the block holds up to %zu", M, b->cap);
	RowSrc src;
	int rc = dbit2_check("sgx_block_load_dbit2", b->N, alleles, bit0, n_file_samp, n_rows, sel, M, src);
	if (rc) return rc;
	return block_load_host(h, b, src, M);
}

extern "C" int sgx_scan_2bit(sgx_handle *h, const uint8_t *packed, size_t bpv, size_t M,
	double *out8, uint8_t *valid)
{
	const int rc = h ? bpv_check(bpv, h->md.N) : SGX_OK;
	if (rc) return rc;
	RowSrc src = plain_rows(packed, bpv);
	return scan_host<IN_2BIT>(h, src, h ? sgx_row_stride(h->md.N) : 0, M, out8, valid);
}

extern "C" int sgx_scan_u8(sgx_handle *h, const uint8_t *dosage, size_t M, double *out8, uint8_t *valid)
{
	RowSrc src = plain_rows(dosage, h ? (size_t)h->md.N : 0);
	return scan_host<IN_U8>(h, src, src.row_bytes, M, out8, valid);
}

extern "C" int sgx_scan_i32(sgx_handle *h, const int32_t *dosage, size_t M, double *out8, uint8_t *valid)
{
	RowSrc src = plain_rows(dosage, h ? (size_t)h->md.N * sizeof(int32_t) : 0);
	return scan_host<IN_I32>(h, src, src.row_bytes, M, out8, valid);
}

extern "C" int sgx_scan_f64(sgx_handle *h, const double *dosage, size_t M, double *out8, uint8_t *valid)
{
	RowSrc src = plain_rows(dosage, h ? (size_t)h->md.N * sizeof(double) : 0);
	return scan_host<IN_F64>(h, src, src.row_bytes, M, out8, valid);
}

extern "C" int sgx_scan_packed(sgx_handle *h, const void *raw, int cls, size_t n_file_samp, double scale, double offset,
	const int32_t *sel, size_t M, double *out8, uint8_t *valid)
{
	if (!h) return fail(SGX_EINVAL, "sgx_scan_packed: NULL handle");
	RowSrc src;
	int rc = packed_check("sgx_scan_packed", h->md.N, raw, cls, n_file_samp, scale, offset, sel, src);
	if (rc) return rc;
	return scan_host<IN_F64>(h, src, (size_t)h->md.N * sizeof(double), M, out8, valid);
}

extern "C" int sgx_scan_dbit2(sgx_handle *h, const uint8_t *alleles, size_t bit0, size_t n_file_samp, const int32_t *n_rows,
	const int32_t *sel, size_t M, double *out8, uint8_t *valid)
{
	if (!h) return fail(SGX_EINVAL, "sgx_scan_dbit2: NULL handle");
	RowSrc src;
	int rc = dbit2_check("sgx_scan_dbit2", h->md.N, alleles, bit0, n_file_samp, n_rows, sel, M, src);
	if (rc) return rc;
	return scan_host<IN_2BIT>(h, src, sgx_row_stride(h->md.N), M, out8, valid);
}

// Burden rows from 2-bit genotypes, then the single-variant test on each row
// (saige_burden_test_bin/quant and the burden halves of ACAT-V / ACAT-O, saige_main.cpp:615-976)
extern "C" int sgx_burden_2bit(sgx_handle *h, const uint8_t *packed, size_t bpv, size_t n_variants,
	size_t n_rows, const int64_t *row_ptr, const int32_t *var_idx, const double *lut,
	double *out8, uint8_t *valid)
{
	if (!h) return fail(SGX_EINVAL, "sgx_burden_2bit: NULL handle");
	if (n_rows == 0) return SGX_OK;
	if (!packed || !row_ptr || !var_idx || !lut || !out8 || !valid)
		return fail(SGX_EINVAL, "sgx_burden_2bit: NULL buffer");
	const int N = h->md.N;
	const int32_t *bad;
	int rc = bpv_check(bpv, N);
	if (!rc) rc = csr_check("sgx_burden_2bit", "row_ptr", n_rows, row_ptr, var_idx, n_variants, &bad);
	if (rc) return rc;
	if (bad) return fail(SGX_EINVAL, "sgx_burden_2bit: variant index %d out of range", *bad);
	const int64_t nnz = row_ptr[n_rows];
	rc = set_dev(h);
	if (rc) return rc;
	h->last_issued = h;
	// device copies: packed rows (4-byte aligned stride), CSR, tables
	const size_t dbpv = ((size_t)(N + 15) / 16) * 4;
	const size_t o_ptr = (n_variants * dbpv + 15) & ~(size_t)15;
	const size_t o_idx = (o_ptr + (n_rows + 1) * sizeof(long long) + 15) & ~(size_t)15;
	const size_t o_lut = (o_idx + (size_t)std::max<int64_t>(nnz, 1) * sizeof(int) + 15) & ~(size_t)15;
	const size_t need = o_lut + (size_t)std::max<int64_t>(nnz, 1) * 4 * sizeof(double);
	if (need > h->stage_pk.cap) HIPCHK(hipStreamSynchronize(h->stream));
	rc = grow(h->stage_pk, need);
	if (rc) return rc;
	rc = copy_rows_h2d(h->stage_pk, dbpv, packed, bpv, n_variants, h->stream);
	if (rc) return rc;
	std::vector<long long> rp(row_ptr, row_ptr + n_rows + 1);
	HIPCHK(hipMemcpyAsync(h->stage_pk + o_ptr, rp.data(), rp.size() * sizeof(long long), hipMemcpyHostToDevice, h->stream));
	if (nnz > 0) {
		HIPCHK(hipMemcpyAsync(h->stage_pk + o_idx, var_idx, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice, h->stream));
		HIPCHK(hipMemcpyAsync(h->stage_pk + o_lut, lut, (size_t)nnz * 4 * sizeof(double), hipMemcpyHostToDevice, h->stream));
	}
	HIPCHK(hipStreamSynchronize(h->stream));      // rp is a local
	const size_t row_bytes = (size_t)N * sizeof(double);
	size_t chunk = std::max<size_t>(1, STAGE_BYTES / row_bytes);
	chunk = std::min<size_t>(std::min(chunk, n_rows), 65535);       // grid.y of burden_collapse_kernel
	rc = ensure_stage(h, chunk * row_bytes, chunk);
	if (rc) return rc;
	rc = ensure_recs(h, chunk);
	if (rc) return rc;
	sgx_stats total{};
	const int ndw = (N + 15) >> 4;
	for (size_t off = 0; off < n_rows; off += chunk) {
		const size_t m = std::min(chunk, n_rows - off);
		hipLaunchKernelGGL(burden_collapse_kernel, dim3((unsigned)((ndw + 255) / 256), (unsigned)m), dim3(256), 0, h->stream,
			h->stage_pk, dbpv, N, reinterpret_cast<const long long *>(h->stage_pk + o_ptr) + off,
			reinterpret_cast<const int *>(h->stage_pk + o_idx), reinterpret_cast<const double *>(h->stage_pk + o_lut),
			reinterpret_cast<double *>(h->stage_in.p), (size_t)N);
		HIPCHK(hipGetLastError());
		rc = scan_staged<IN_F64>(h, h->stage_in, row_bytes, m, out8 + off * 8, valid + off, total);
		if (rc) return rc;
	}
	h->stats = total;
	return SGX_OK;
}
