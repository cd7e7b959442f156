// host_spa.h -- kernel dispatch over the compile-time K, the SPA stage of a call, the frame of a call, the FP64 score kernels.
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.

// ---- kernel dispatch over the compile-time K ------------------------------

// f(std::integral_constant<int, V>()) for the V of LO .. LO + sizeof...(I) - 1 that equals v; false when none does
template <int LO, typename F, int... I>
static bool with_int(int v, F &&f, std::integer_sequence<int, I...>)
{
	return ((v == LO + I && (f(std::integral_constant<int, LO + I>()), true)) || ...);
}
// ... for the model's K = 1 .. KMAX
template <typename F>
static bool with_k(int K, F &&f) { return with_int<1>(K, f, std::make_integer_sequence<int, KMAX>()); }
// ... for the width PP = 8, 16, 32, 64 that holds P score values
template <typename F>
static void with_pp(int P, F &&f)
{
	if (P <= 8) f(std::integral_constant<int, 8>());
	else if (P <= 16) f(std::integral_constant<int, 16>());
	else if (P <= 32) f(std::integral_constant<int, 32>());
	else f(std::integral_constant<int, 64>());
}

// Sample splits of the MFMA kernels: a few rounds of the workgroups a CU holds (wg_per_cu), and a
// multiple of 8 splits when there are that many, so that each XCD works on whole splits
// (grm_contract_kernel, kern_grm.h).  vpb: rows per workgroup.
static dim3 mf_grid(int n_cu, size_t rows, int ntile, int *tps, int vpb = MF_VPB, int wg_per_cu = 2)
{
	const int vt = (int)((rows + vpb - 1) / vpb);
	int sk = std::max(1, (n_cu * wg_per_cu * 4 + vt / 2) / vt);
	sk = std::min(sk, std::max(1, ntile / 24));   // a split shorter than ~24 tiles is mostly prologue and atomics
	if (sk >= 6) sk = (sk + 7) & ~7;
	sk = std::min(sk, std::max(1, ntile / 2));
	*tps = (ntile + sk - 1) / sk;
	*tps += *tps & 1;                         // even tile ranges (wide-row kernel)
	sk = (ntile + *tps - 1) / *tps;
	return dim3((unsigned)vt, (unsigned)sk);
}

// the series moments kernel of the input type (dosage rows: spa4_moments_ds)
template <int KK, int NCX, int INPUT>
static const void *spa4_moments_fn()
{
	if constexpr (INPUT == IN_2BIT) return (const void *)spa4_moments<KK, NCX>;
	else return (const void *)spa4_moments_ds<KK, NCX, INPUT>;
}

// the exact dense pass (spa_kernel, kern_spa.h) over counters[slot] variants of a call of M: the records of `list`, or,
// without one, the records in order
template <int KK, int INPUT>
static void launch_dense(sgx_handle *h, RowsRef rr, size_t M, int slot, const int *list, double *out8)
{
	const dim3 sgrid((unsigned)std::min<size_t>(M, (size_t)h->spa_grid));
	hipLaunchKernelGGL((spa_kernel<KK, 512, INPUT>), sgrid, dim3(512), 0, h->stream, rr,
		h->md, h->recs, h->counters, slot, list, h->scratch, h->scratch_stride, out8);
}

// the SPA stage's launches for K = KK (launch_spa)
template <int KK, int INPUT>
static int launch_spa_k(sgx_handle *h, RowsRef rr, size_t M, double *out8, bool lazy_dense)
{
	const DevModel &md = h->md;
	hipStream_t st = h->stream;
	if (h->force_v1 && INPUT != IN_2BIT) {
		launch_dense<KK, INPUT>(h, rr, M, 0, nullptr, out8);
		return SGX_OK;
	}
	// series SPA stage (kern_spa4.h): rounds of at most vcap4 flagged variants; tier A (short series), then tier B
	// with what tier A handed on
	const size_t fl = spa4_lds_bytes(KK);
	if (!h->mom_attr_set[INPUT]) {
		HIPCHK(hipFuncSetAttribute(spa4_moments_fn<KK, SPA4_NCA, INPUT>(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fl));
		HIPCHK(hipFuncSetAttribute(spa4_moments_fn<KK, SPA4_NCB, INPUT>(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fl));
		h->mom_attr_set[INPUT] = true;
	}
	const int nround = (int)((M + h->vcap4 - 1) / h->vcap4);
	const int btop = (int)(2 * M);
	const dim3 gsolve((unsigned)std::min((h->vcap4 + 3) / 4, 4 * h->n_cu));   // a wave per variant, grid-stride
	// what the series does not cover: exact exp/log sums, one workgroup per variant; then the exact dense g_pos / g_neg pass
	// a packed row in LDS when it fits; short rows: 128 threads per variant, 4 workgroups per CU
	const size_t rowb5 = (size_t)((md.N + 63) / 64) * 16;
	const size_t l5 = (INPUT == IN_2BIT && rowb5 <= 120 * 1024) ? rowb5 : 0;
	const bool small5 = INPUT == IN_2BIT && rowb5 <= 32 * 1024;
	if (l5 > 48 * 1024 && !h->spa5_attr_set[INPUT]) {
		HIPCHK(hipFuncSetAttribute((const void *)spa5_kernel<KK, INPUT, 0, 512>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l5));
		HIPCHK(hipFuncSetAttribute((const void *)spa5_kernel<KK, INPUT, 1, 512>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l5));
		h->spa5_attr_set[INPUT] = true;
	}
	auto moments = [&](auto ncx, int tier, int rd) {
		constexpr int NCX = decltype(ncx)::value;
		if constexpr (INPUT == IN_2BIT)
			hipLaunchKernelGGL((spa4_moments<KK, NCX>), dim3((unsigned)h->n_cu), dim3(WAVE * spa4_waves(KK)), fl, st, rr, md, h->nseg,
				tier, btop, rd * h->vcap4, h->vcap4, h->recs, h->counters, h->seg4, h->cur5 + 2);
		else
			hipLaunchKernelGGL((spa4_moments_ds<KK, NCX, INPUT>), dim3((unsigned)h->n_cu), dim3(WAVE * spa4_waves(KK)), fl, st,
				(const void *)rr.base, rr.bpv, md, h->nseg, tier, btop, rd * h->vcap4, h->vcap4, h->recs, h->counters, h->seg4, h->cur5 + 2);
		hipLaunchKernelGGL((spa4_solve<KK, NCX>), gsolve, dim3(256), 0, st, md, h->nseg, tier, btop, rd * h->vcap4, h->vcap4,
			h->recs, h->counters, h->seg4, h->fallback, h->fb_x2, out8, h->force_dense ? 1 : 0, h->force_exact ? 1 : 0);
	};
	for (int rd = 0; rd < nround; rd++) moments(std::integral_constant<int, SPA4_NCA>(), 0, rd);
	for (int rd = 0; rd < nround; rd++) moments(std::integral_constant<int, SPA4_NCB>(), 1, rd);
	// (genotype blocks carry the carrier lists of the rare variants, rr.cptr: the kernels walk those instead of scanning
	// the row; the "spa_scan_rows" hook makes them scan, as for row-major input)
	const size_t ws5 = spa5_wg_bytes(md.N);
	auto spa5 = [&](auto threads, int nwg) {
		constexpr int T5 = decltype(threads)::value;
		if constexpr (T5 == 512 || INPUT == IN_2BIT) {     // (the 128-thread forms: 2-bit rows only)
			hipLaunchKernelGGL((spa5_kernel<KK, INPUT, 0, T5>), dim3((unsigned)nwg), dim3(T5), l5, st, rr, md, h->recs, h->counters,
				h->fb_spa2, h->fb_x2, h->cur5, h->fallback, h->scr5, out8, h->force_dense ? 1 : 0, h->force_exact ? 1 : 0, l5,
				h->spa_scan_rows, ws5, 3);
			hipLaunchKernelGGL((spa5_kernel<KK, INPUT, 1, T5>), dim3((unsigned)nwg), dim3(T5), l5, st, rr, md, h->recs, h->counters,
				h->fb_x2, h->fb_x2, h->cur5 + 1, h->fallback, h->scr5, out8, h->force_dense ? 1 : 0, h->force_exact ? 1 : 0, l5,
				h->spa_scan_rows, ws5, 4);
		}
	};
	if (small5) spa5(std::integral_constant<int, 128>(), h->nwg5);
	else spa5(std::integral_constant<int, 512>(), h->n_cu);
	if (!lazy_dense) launch_dense<KK, INPUT>(h, rr, M, 2, h->fallback, out8);
	return SGX_OK;
}

// SPA stage of the flagged variants of a call (their records are in h->recs): the series kernels
// (kern_spa4.h), the per-variant kernels and the exact dense pass.  rr: the call's rows.
// lazy_dense (device-resident calls, whose results are read after a sync): the exact dense pass -- normally
// without a single variant -- is not launched here.  An empty launch of its 512-thread workgroups at the end of
// every step still has to wait for room on a CU beside the other lane's contraction kernel or cumulant pass
// (0.1-1.2 ms in kernel traces), and with it the lane's completion and its next step.  The next sync of the lane
// reads the step's counters and launches the pass if a variant asked for it (sync_lane).
template <int INPUT>
static int launch_spa(sgx_handle *h, RowsRef rr, size_t M, double *out8, bool lazy_dense = false)
{
	h->stats.spa_launches = 0;
	if (h->md.quant) return SGX_OK;
	int rc = SGX_OK;
	with_k(h->md.K, [&](auto kk) { rc = launch_spa_k<decltype(kk)::value, INPUT>(h, rr, M, out8, lazy_dense); });
	if (rc) return rc;
	HIPCHK(hipGetLastError());
	const bool v1 = h->force_v1 && INPUT != IN_2BIT;
	h->stats.spa_launches = v1 ? 1u : (uint32_t)(4 * ((M + h->vcap4 - 1) / h->vcap4) + 3);
	if (lazy_dense && !v1) { h->pend_dense.active = true; h->pend_dense.rr = rr; h->pend_dense.M = M; h->pend_dense.out8 = out8; }
	return SGX_OK;
}

// the dense pass a lazy call left out, for the variants on its fallback list (counters[2] of that call)
static int launch_pending_dense(sgx_handle *h)
{
	with_k(h->md.K, [&](auto kk) {
		launch_dense<decltype(kk)::value, IN_2BIT>(h, h->pend_dense.rr, h->pend_dense.M, 2, h->fallback, h->pend_dense.out8);
	});
	HIPCHK(hipGetLastError());
	return SGX_OK;
}

// The frame of every call, around its score stage on stream sst.  b: the block the call reads, or nullptr.
// Begin: the block's load is done; counters and queue cursors zeroed (the fixed-point chain's s3_reduce_kernel zeroes
// them itself); ev[0].
static int scan_begin(sgx_handle *h, hipStream_t sst, ScanForm form, const sgx_block *b)
{
	h->form = form;
	if (b) HIPCHK(hipStreamWaitEvent(sst, b->ready, 0));
	if (form == FORM_FP64) {
		HIPCHK(hipMemsetAsync(h->counters, 0, 24 * sizeof(int), sst));
		if (h->cur5) HIPCHK(hipMemsetAsync(h->cur5, 0, 8 * sizeof(int), sst));
	}
	HIPCHK(hipEventRecord(h->ev[0], sst));
	return SGX_OK;
}

// End: ev[1] behind the score stage; the SPA stage on h->stream (low priority, behind the score chain), ev[2]; the
// block's last read; the counters to the host for sync_lane.
template <int INPUT>
static int scan_end(sgx_handle *h, hipStream_t sst, const sgx_block *b, RowsRef rr, size_t M, double *out8, bool lazy_dense)
{
	HIPCHK(hipEventRecord(h->ev[1], sst));
	h->stats.score_launches = h->form == FORM_FP64 ? 1 : 5;
	if (sst != h->stream) HIPCHK(hipStreamWaitEvent(h->stream, h->ev[1], 0));
	int rc = launch_spa<INPUT>(h, rr, M, out8, lazy_dense);
	if (rc) return rc;
	if (lazy_dense) h->pend_dense.blk = b;
	HIPCHK(hipEventRecord(h->ev[2], h->stream));
	if (b) {
		HIPCHK(hipEventRecord(b->last_read, h->stream));
		const_cast<sgx_block *>(b)->was_read = true;
	}
	HIPCHK(hipMemcpyAsync(h->h_counters, h->counters, 24 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
	h->stats.n_variants = M;
	h->stats_pending = true;
	return SGX_OK;
}

// the FP64 score kernels for K = KK (launch_scan)
template <int KK, int INPUT>
static int launch_score_fp64(sgx_handle *h, RowsRef rr, size_t M, double *out8, uint8_t *valid)
{
	const DevModel &md = h->md;
	constexpr int SB = 256, P = 2 * KK + 2;
	hipStream_t st = h->stream;
	const dim3 grid((unsigned)M);
	if constexpr (INPUT == IN_2BIT) {
		hipLaunchKernelGGL((score2b_kernel<P, SB>), grid, dim3(SB), 0, st,
			rr, (int)M, md, h->recs, h->counters, out8, valid, (const int *)nullptr, 0, 0, (int *)nullptr, (int *)nullptr);
	} else {
		using T = std::conditional_t<INPUT == IN_U8, uint8_t, double>;
		const T *rows = reinterpret_cast<const T *>(rr.base);
		if constexpr (KK <= 8) {
			if (!h->force_v1) {
				// tiled one-pass kernels: 32 variants x a sample range per workgroup
				const int vb = (int)((M + DS_TILE_VB - 1) / DS_TILE_VB);
				int ns = std::max(1, std::min((4 * h->n_cu + vb - 1) / vb, (md.N + 4095) / 4096));
				int per = (((md.N + ns - 1) / ns) + 63) & ~63;
				ns = (md.N + per - 1) / per;
				const size_t need = (size_t)ns * M * (3 * P + 2);
				if (need > h->ds_part.cap) {
					HIPCHK(hipStreamSynchronize(st));
					HIPCHK(h->ds_part.reserve(need));
				}
				hipLaunchKernelGGL((score_ds_tile_kernel<P, T>), dim3((unsigned)vb, (unsigned)ns), dim3(256), 0, st,
					rows, (int)M, md, per, h->ds_part);
				hipLaunchKernelGGL((score_ds_tile_epilogue<P>), dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st,
					(int)M, md, ns, h->ds_part, h->recs, h->counters, out8, valid);
				return SGX_OK;
			}
		}
		hipLaunchKernelGGL((score_ds_kernel<P, SB, T>), grid, dim3(SB), 0, st, rows, (int)M, md, h->recs, h->counters, out8, valid);
	}
	return SGX_OK;
}

// Score stage by the FP64 kernels (dosage rows; 2-bit rows of the "score_v1" hook or of a model the fixed-point form
// does not hold), then the SPA stage.  Row-major rows.  b: the resident block whose rows these are, or nullptr.
template <int INPUT>
static int launch_scan(sgx_handle *h, const void *rows, size_t row_bytes, size_t M, double *out8, uint8_t *valid,
	const sgx_block *b = nullptr)
{
	const RowsRef rr{reinterpret_cast<const uint8_t *>(rows), row_bytes, 0, nullptr, nullptr, nullptr};
	int rc = scan_begin(h, h->stream, FORM_FP64, b);
	if (rc) return rc;
	if (!with_k(h->md.K, [&](auto kk) { rc = launch_score_fp64<decltype(kk)::value, INPUT>(h, rr, M, out8, valid); }))
		return fail(SGX_EINVAL, "unsupported K=%d", h->md.K);
	if (rc) return rc;
	HIPCHK(hipGetLastError());
	return scan_end<INPUT>(h, h->stream, b, rr, M, out8, false);
}
