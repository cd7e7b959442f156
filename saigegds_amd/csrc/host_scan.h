// host_scan.h -- the block scan (contraction kernel forms, sparse pass, epilogue), lanes, the row-major device call.
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.

// a lane's buffer that a call in flight may still read: the lane's streams are brought to their end before it regrows
template <typename T>
static int ensure_buf(sgx_handle *lane, DevBuf<T> &buf, size_t need)
{
	if (need <= buf.cap) return SGX_OK;
	for (hipStream_t st : {(hipStream_t)lane->stream, (hipStream_t)lane->hstream, (hipStream_t)lane->s3_side}) if (st) HIPCHK(hipStreamSynchronize(st));
	return grow(buf, need);
}

// The shapes of the contraction kernel's forms (kern_score3.h): [0] two planes, [1] three planes; entries in table order
struct S3Shape { int nbf, naf, nc, nla, nlb, da, db; };
#define S3_SHAPE(...) S3Shape{__VA_ARGS__},
static constexpr S3Shape s3_shapes[2][15] = {{S3_FOR_EACH_NBF(S3_SHAPE)}, {S3_FOR_EACH_NBF_MISS(S3_SHAPE)}};
#undef S3_SHAPE

// The contraction kernel of the two-plane (MISS = false) or three-plane form, in the shape of its table's entry I,
// on the lane's score stream.  slots: fragment slots of a variant's row of limb sums.
template <bool MISS, int I>
static int launch_score3(sgx_handle *h, const sgx_block *b, RowsRef rr, size_t M, int grid, int slots, S3Plan &pl)
{
	constexpr S3Shape s = s3_shapes[MISS][I];
	hipStream_t st = h->hstream;
	pl = s3_plan(M, b->ntile, grid, s.naf * s.nc, rr.bpv);
	int rc = ensure_buf(h, h->s3_slabs, (size_t)pl.ng * pl.ipg * s.nc * s.naf * slots * 256);
	if (rc) return rc;
	const size_t lds = s3_lds_bytes(s.nbf, s.naf, s.nc, s.da, s.db);
	auto kern = score3_kernel<s.nbf, s.naf, s.nc, s.nla, s.nlb, s.da, s.db, MISS>;
	bool &attr = (MISS ? h->s3_attr_miss : h->s3_attr)[s.nbf];
	if (!attr) {
		HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
		attr = true;
	}
	HIPCHK(hipEventRecord(h->evk[0], st));
	hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(64 * (s.nc + s.nla + s.nlb)), lds, st,
		rr.base, h->mf[0].Fl, pl, h->s3_slabs);
	HIPCHK(hipEventRecord(h->evk[1], st));
	h->evk_set = true;
	return SGX_OK;
}

// Scan of a block (resident, or the lists of a row-major call with the caller's rows) on this lane's score stream by
// the fixed-point chain: the sums over the missing genotypes (form FORM_LISTS: the sparse pass over the block's lists;
// FORM_ROWS: the fused list + T3 pass over the rows; FORM_THREE: none, they come out of the contraction kernel, the
// block's lists are not read and need not exist), contraction, reduction, epilogue, the FP64 kernel for what the lists
// do not cover, SPA stage.
static int launch_block_scan(sgx_handle *h, const sgx_block *b, size_t M, double *out8, uint8_t *valid, bool lazy_dense, ScanForm form)
{
	const DevModel &md = h->md;
	hipStream_t st = h->hstream;
	const RowsRef rr = block_rows(b);
	const S3Lists L = block_lists(b);
	int rc = ensure_buf(h, h->s3_t3, (size_t)b->nr * M * md.P * 2);   // per-range sums over the missing samples (the epilogue adds them up)
	if (rc) return rc;
	if (form == FORM_ROWS) {
		// one pass over the rows: the missing genotypes of every (range, variant), their sums of Q gathered on the spot
		// (no kernel between this pass and the contraction: the epilogue adds up the ranges' sums and counts itself)
		HIPCHK(hipEventRecord(h->ev_lists, st));
		h->lists_timed = true;
		const dim3 g((unsigned)((M + 3) / 4), (unsigned)b->nr);
		with_pp(md.P, [&](auto pp) {
			hipLaunchKernelGGL((s3_lists_t3_kernel<8, decltype(pp)::value>), g, dim3(256), 0, st,
				rr.base, rr.bpv, b->N, (int)M, b->ntile, L, md.P, h->dQ, h->s3_t3);
		});
		HIPCHK(hipGetLastError());
	}
	rc = scan_begin(h, st, form, b);
	if (rc) return rc;
	rc = ensure_buf(h, h->s3_ovf, M);
	if (rc) return rc;
	if (form == FORM_LISTS) {
		// Sums over the missing samples, on the side stream, FIRST; the contraction kernel waits for them:
		//  * with few fragments (3 waves of ~154 registers per SIMD) the pass finds no room beside a resident
		//    contraction workgroup; launched second it would wait for the kernel's end;
		//  * from 7 fragments on (2 waves of <= 216 registers) one wave of the pass fits per SIMD, but in the kernel's
		//    shadow it slows the kernel by what it saves (K = 13, same box: 6.13 / 6.20 ms per step first, 6.23 / 6.23 after);
		//  * launched together onto an idle GPU the pass's 25 000 small workgroups and the kernel's 256 persistent ones
		//    fight for the CUs (kernel traces: 1.9 ms for the kernel and 1.1 ms for the pass in those steps).
		// (round 3, tools/README.md: the three orders measured)
		HIPCHK(hipEventRecord(h->s3_fork, st));                  // (the side stream starts where this stream stands NOW)
		HIPCHK(hipStreamWaitEvent(h->s3_side, h->s3_fork, 0));
		with_pp(md.P, [&](auto pp) {
			constexpr int tpw = 64 / decltype(pp)::value;
			const unsigned chunks = (unsigned)((M + 4 * tpw - 1) / (4 * tpw));
			hipLaunchKernelGGL(s3_t3_kernel<decltype(pp)::value>, dim3(chunks * (unsigned)b->nr), dim3(256), 0, h->s3_side,
				(int)M, md.P, h->dQ, L, h->s3_t3);
		});
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(h->s3_join, h->s3_side));
		HIPCHK(hipStreamWaitEvent(st, h->s3_join, 0));
	}
	const bool miss = form == FORM_THREE;
	const int NBF = h->mf_nbfv[0] + 1;
	const int slots = miss ? 2 * NBF - 1 : NBF;
	const int grid = std::max(8, h->n_cu & ~7);
	constexpr int NSHAPE = (int)(sizeof s3_shapes[0] / sizeof s3_shapes[0][0]);
	int i = 0;
	while (i < NSHAPE && s3_shapes[miss][i].nbf != NBF) i++;
	S3Plan pl{};
	const auto shapes = std::make_integer_sequence<int, NSHAPE>();
	const bool found = miss ? with_int<0>(i, [&](auto I) { rc = launch_score3<true, decltype(I)::value>(h, b, rr, M, grid, slots, pl); }, shapes)
		: with_int<0>(i, [&](auto I) { rc = launch_score3<false, decltype(I)::value>(h, b, rr, M, grid, slots, pl); }, shapes);
	if (!found) return fail(SGX_EINVAL, "score3: %d B fragments not supported", NBF);
	if (rc) return rc;
	HIPCHK(hipGetLastError());
	const S3Shape &sh = s3_shapes[miss][i];
	const int acc_stride = 16 * slots;
	const int per = sh.nc * sh.naf * slots * 256;
	hipLaunchKernelGGL(s3_reduce_kernel, dim3((unsigned)((per / 4 + 255) / 256), (unsigned)pl.vt), dim3(256), 0, st,
		pl, (int)M, sh.nc, sh.naf, slots, h->s3_slabs, h->mf_acc, acc_stride, h->counters, h->cur5);
	const int btop = md.quant ? 0 : (int)(2 * M);
	if (!with_k(md.K, [&](auto kk) {
		constexpr int KK = decltype(kk)::value;
		hipLaunchKernelGGL((score3_epilogue<KK>), dim3((unsigned)((M + s3e_vb(KK) - 1) / s3e_vb(KK))), dim3(s3e_vb(KK)), 0, st,
			(int)M, md, h->mfe, h->mf_acc, acc_stride, miss ? 16 * NBF : 0, h->s3_t3, b->nr, L.lcnt, L.ld, h->s3_ovf, h->recs,
			h->counters, btop, h->fb_spa2, h->fb_x2, out8, valid, h->guard_tol);
		hipLaunchKernelGGL((score2b_kernel<2 * KK + 2, 256>), dim3((unsigned)std::min<size_t>(M, 4 * (size_t)h->n_cu)), dim3(256), 0, st,
			rr, (int)M, md, h->recs, h->counters, out8, valid, (const int *)h->s3_ovf, 23, btop, h->fb_spa2, h->fb_x2);
	}))
		return fail(SGX_EINVAL, "score3: unsupported K=%d", md.K);
	HIPCHK(hipGetLastError());
	return scan_end<IN_2BIT>(h, st, b, rr, M, out8, lazy_dense);
}

// picks the lane of the next device-resident call (two lanes alternate) and makes it ready for M variants
static int next_lane(sgx_handle *h, size_t M, sgx_handle **lane_out)
{
	sgx_handle *lane = h, *other = nullptr;
	if (h->n_lanes > 1) {
		lane = h->next_lane ? h->twins[h->next_lane - 1] : h;
		other = h->last_issued;                    // the lane of the previous call
		h->next_lane = (h->next_lane + 1) % h->n_lanes;
	}
	int rc = sync_lane(lane);            // the lane's previous call is done: keep its stats (events are reused)
	if (rc) return rc;
	h->last_issued = lane;
	rc = ensure_recs(lane, M);
	if (rc) return rc;
	// score stages do not overlap: this one starts after the other lane's has ended
	if (other && other != lane && other->stats_pending) HIPCHK(hipStreamWaitEvent(lane->hstream, other->ev[1], 0));
	*lane_out = lane;
	return SGX_OK;
}

// Which form a call takes.  b: the resident block of an sgx_scan_block call (its census, read on first use: a block
// with many missing genotypes, or variants its pool had no room for, takes the three-plane form); nullptr: row-major
// rows.  For those the two-plane form needs the positions of the missing genotypes -- a pass over the rows
// (s3_lists_t3_kernel) whose cost grows with their number; the three-plane form needs none, at ~1.7 x the MFMAs.  Large
// kernels of different streams do not share the machine (tools/README.md, round 4: a kernel that holds every CU keeps
// the other queue's out), so what counts is the sum of the two kernels' times:
//   K = 3 binary (4 B fragments), N = 430 000: list pass 0.89 + two planes 1.04 ms against three planes 1.55-1.75 ms:
//     step 3.19-3.23 -> 2.88-3.01 ms (same box), N = 50 000: 0.676 -> 0.620; K = 2: 3.11 -> 2.84
//   K = 4 (5 fragments): 3.56 against 3.63, K = 5: 3.94 against 4.02 ms: the two-plane form, until more than ~0.5 % of
//     the genotypes are missing -- where the sparse sums have grown to the difference and the segments' room
//     (S3_LT_CAP entries) is about to overflow (dense_mode, set and cleared by sync_lane).
static int scan_form(const sgx_handle *lane, const sgx_block *b, ScanForm *form)
{
	const sgx_handle *p = lane->owner ? lane->owner : lane;
	*form = FORM_FP64;
	if (!p->mf_ok || p->force_v1) return SGX_OK;
	if (b && !b->info_read) {
		HIPCHK(hipEventSynchronize(b->ready));
		sgx_block *bw = const_cast<sgx_block *>(b);
		const double frac = 64.0 * (double)b->h_info[0] / ((double)b->M * (double)b->N);
		bw->dense = frac > SGX_DENSE_ON || (size_t)b->h_info[1] * 32 > b->M;
		bw->info_read = true;
	}
	const bool three = p->dense_opt >= 0 ? p->dense_opt != 0 : b ? b->dense : lane->mf_nbfv[0] + 1 <= 4 || p->dense_mode;
	*form = three ? FORM_THREE : b ? FORM_LISTS : FORM_ROWS;
	return SGX_OK;
}

extern "C" int sgx_scan_block(sgx_handle *h, const sgx_block *b, double *out8_dev, uint8_t *valid_dev)
{
	if (!h || !b) return fail(SGX_EINVAL, "sgx_scan_block: NULL argument");
	if (!out8_dev || !valid_dev) return fail(SGX_EINVAL, "sgx_scan_block: NULL buffer");
	if (b->lists_only) return fail(SGX_EINVAL, "sgx_scan_block: not a resident block");
	if (b->M == 0) return SGX_OK;
	if (b->device != h->device) return fail(SGX_EINVAL, "sgx_scan_block: block and handle are on different devices");
	if (b->N != h->md.N) return fail(SGX_EINVAL, "sgx_scan_block: the block holds rows of %d samples, the model has %d", b->N, h->md.N);
	int rc = set_dev(h);
	if (rc) return rc;
	sgx_handle *lane = nullptr;
	rc = next_lane(h, b->M, &lane);
	if (rc) return rc;
	ScanForm form;
	rc = scan_form(lane, b, &form);
	if (rc) return rc;
	if (form == FORM_FP64) {       // the block's rows, without its carrier lists
		const RowsRef rr = block_rows(b);
		return launch_scan<IN_2BIT>(lane, rr.base, rr.bpv, b->M, out8_dev, valid_dev, b);
	}
	return launch_block_scan(lane, b, b->M, out8_dev, valid_dev, true, form);
}

// the lists of this lane's row-major calls (the rows stay where the caller has them)
static int ensure_tmp_block(sgx_handle *lane, int which, size_t M)
{
	sgx_block *&tb = lane->tmp_blk[which];
	if (tb && tb->cap >= M) return SGX_OK;
	HIPCHK(hipStreamSynchronize(lane->stream));
	HIPCHK(hipStreamSynchronize(lane->hstream));
	if (tb) { sgx_block_free(tb); tb = nullptr; }
	return block_create(lane->md.N, M, lane->device, true, 0, &tb);
}

// row-major 2-bit rows on the device -> table: the scan reads the rows where they are
static int scan_rows_dev(sgx_handle *lane, int which, const uint8_t *rows_dev, size_t bpv, size_t M, double *out8, uint8_t *valid, bool lazy_dense)
{
	ScanForm form;
	int rc = scan_form(lane, nullptr, &form);
	if (rc) return rc;
	if (form == FORM_FP64) return launch_scan<IN_2BIT>(lane, rows_dev, bpv, M, out8, valid);
	rc = ensure_tmp_block(lane, which, M);
	if (rc) return rc;
	sgx_block *tb = lane->tmp_blk[which];
	tb->ext_rows = rows_dev; tb->ext_bpv = bpv;
	return launch_block_scan(lane, tb, M, out8, valid, lazy_dense, form);
}

extern "C" int sgx_scan_2bit_dev(sgx_handle *h, const uint8_t *packed_dev, size_t bpv,
	size_t M, double *out8_dev, uint8_t *valid_dev)
{
	if (!h) return fail(SGX_EINVAL, "sgx_scan_2bit_dev: NULL handle");
	if (M == 0) return SGX_OK;
	if (!packed_dev || !out8_dev || !valid_dev)
		return fail(SGX_EINVAL, "sgx_scan_2bit_dev: NULL buffer");
	if (M > 0x7fffffffu / S3_NR) return fail(SGX_EINVAL, "sgx_scan_2bit_dev: too many variants in one call");
	int rc = dev_rows_check("sgx_scan_2bit_dev", packed_dev, bpv, h->md.N);
	if (!rc) rc = set_dev(h);
	if (rc) return rc;
	sgx_handle *lane = nullptr;
	rc = next_lane(h, M, &lane);
	if (rc) return rc;
	return scan_rows_dev(lane, 0, packed_dev, bpv, M, out8_dev, valid_dev, true);
}
