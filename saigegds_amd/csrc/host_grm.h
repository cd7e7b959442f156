// host_grm.h -- implicit-GRM operator of the null-model fit (kern_grm.h): sgx_grm on the owners of host_mem.h.
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.

// ===========================================================================
// Implicit-GRM operator of the null-model fit (kern_grm.h)
// Products and solves work on k right-hand sides at once; the single-vector entry points are k = 1.
// Pass 1 puts two columns' limbs side by side in each 16-column B fragment (7 + 7 limbs) and runs
// the contraction kernel with up to GRM_MAXF = 3 value fragments (GRM_GROUP = 6 columns); pass 2 needs
// x and gam limbs of a column (7 + 7) in one fragment and runs with up to 3 (GRM_GROUP2).  A group of 6
// columns thus streams the genotypes three times (G once, Gt twice) where 6 single products stream
// them 12 times.

struct sgx_grm {
	int device = 0;
	// (released in reverse order: buffers, events, the stream -- sgx_grm_free waits for the stream first)
	DevStream stream;
	DevEvent gd_ev0, gd_ev1;               // host_grm_dense.h: around the kernels of a piece of sgx_grm_dense
	DevEvent kg_ev0, kg_ev1;               // host_king.h: around the kernel of sgx_grm_king_pairs
	int N = 0; size_t M = 0;
	size_t bpvN = 0, bpvM = 0;             // row strides of G (marker-major) and Gt (sample-major)
	DevBuf<uint8_t> G, Gt;
	DevBuf<double> af, inv, l0, diag;
	int ntileN = 0, ntileM = 0;            // 256-entry limb tiles over samples / over markers
	DevBuf<uint8_t> FlN, FlM;              // limb tile images, 16 GRM_MAXF columns wide
	DevBuf<int> accV, accS;                // [M][32 GRM_MAXF], [N][32 GRM_MAXF]
	DevBuf<double> xv, gv;                 // [GRM_GROUP][M]
	DevBuf<unsigned long long> maxb;       // [GRM_MAX_RHS][3]: b, x, gam
	PcgWork pw;                            // block partials, staging and solver vectors (host_pcg.h)
	int n_cu = 256;
	// marker groups (sgx_grm_set_groups): a column of a *_loco call leaves one group out
	int n_groups = 0;
	DevBuf<int> grp;                       // [M] group id per marker
	size_t gsize[GRM_MAX_GROUPS] = {};     // markers per group
	DevBuf<double> diagx;                  // [1 + n_groups][N]: row 0 = diag, row 1 + c = diag(GRM without group c)
	// explicit GRM (host_grm_dense.h): scratch of sgx_grm_dense / sgx_grm_sparse, allocated on first use
	DevBuf<double> gd_part, gd_out;        // slab tiles [nslab][tiles][256]; a rectangle of K
	bool gd_ready = false;                 // the screen's tables below are built
	int gd_s = 0;                          // Q = round(g 2^s)
	DevBuf<uint2> gd_lut;                  // [markers padded to 512] limb bytes per code
	DevBuf<double> gd_A, gd_R;             // [N] bound terms per sample
	DevBuf<unsigned long long> gd_cnt;     // [2]: flagged sub-tiles, entries (also the table maximum)
	DevBuf<GdTile> gd_list;
	DevBuf<int> gd_i, gd_j; DevBuf<double> gd_v;
	double gd_ms_kernel = 0;               // the kernels' time over the last sgx_grm_dense call
	// marker-side output and principal components (host_pca.h): scratch allocated on first use
	DevBuf<double> md_out;                 // [k][M]: dot_v of k columns
	DevBuf<double> ts_part, ts_C, ts_T;    // ts_gram partials [slabs][64][64], its result and the matrix of ts_apply [64][64]
	DevBuf<double> pca_X0, pca_X1, pca_Y, pca_W;   // [n_block][N] blocks of sgx_grm_pca
	// KING-robust kinship (host_king.h): scratch of sgx_grm_king_counts / sgx_grm_king_pairs, allocated on first use
	DevBuf<int> kg_out;                    // [5][ni][nj] counts of a piece of a rectangle
	DevBuf<unsigned long long> kg_cnt;     // [1] pairs listed
	DevBuf<int> kg_i, kg_j, kg_c5;         // the pair list: indices and [pairs][5] counts
	DevBuf<double> kg_kin, kg_ibs;         // ... kinship and IBS0
};
static_assert(GRM_MAX_RHS == SGX_GRM_MAX_RHS, "kern_grm.h and saigehip.h disagree on the column limit");
static_assert(GRM_MAX_GROUPS == SGX_GRM_MAX_GROUPS, "kern_grm.h and saigehip.h disagree on the group limit");

extern "C" void sgx_grm_free(sgx_grm *g)
{
	if (!g) return;
	(void)hipSetDevice(g->device);
	if (g->stream) (void)hipStreamSynchronize(g->stream);
	delete g;
}

// saige_store_2b_geno (saige_fitnull.cpp:159-230): packed = n_markers rows of
// bytes_per_marker bytes (>= ceil(N/4)), 2-bit codes 0/1/2 = allele count, 3 = missing
static int grm_init_impl(const uint8_t *packed, size_t bytes_per_marker, int32_t n_samp,
	size_t n_markers, int device, sgx_grm **out, hipMemcpyKind kind);

extern "C" int sgx_grm_init(const uint8_t *packed, size_t bytes_per_marker, int32_t n_samp,
	size_t n_markers, int device, sgx_grm **out)
{
	return grm_init_impl(packed, bytes_per_marker, n_samp, n_markers, device, out, hipMemcpyHostToDevice);
}

// same, the packed matrix already resident in this GPU's HBM (it is copied)
extern "C" int sgx_grm_init_dev(const uint8_t *packed_dev, size_t bytes_per_marker, int32_t n_samp,
	size_t n_markers, int device, sgx_grm **out)
{
	return grm_init_impl(packed_dev, bytes_per_marker, n_samp, n_markers, device, out, hipMemcpyDeviceToDevice);
}

static int grm_init_impl(const uint8_t *packed, size_t bytes_per_marker, int32_t n_samp,
	size_t n_markers, int device, sgx_grm **out, hipMemcpyKind kind)
{
	if (!packed || !out) return fail(SGX_EINVAL, "sgx_grm_init: NULL argument");
	*out = nullptr;
	if (n_samp <= 0 || n_markers == 0) return fail(SGX_EINVAL, "sgx_grm_init: empty genotype matrix");
	if (bytes_per_marker < (size_t)(n_samp + 3) / 4)
		return fail(SGX_EINVAL, "sgx_grm_init: bytes_per_marker=%zu < ceil(N/4)", bytes_per_marker);
	if ((double)n_markers * 384.0 >= 2147483647.0 || (double)n_samp * 384.0 >= 2147483647.0)
		return fail(SGX_EINVAL, "sgx_grm_init: matrix too large for int32 limb sums");
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SGX_ENODEV, "sgx_grm_init: no HIP device available");
	if (device < 0 || device >= ndev) return fail(SGX_EINVAL, "sgx_grm_init: device %d out of range", device);
	std::unique_ptr<sgx_grm, void (*)(sgx_grm *)> hold(new sgx_grm(), sgx_grm_free);   // released on every early return
	sgx_grm *g = hold.get();
	g->device = device;
	HIPCHK(hipSetDevice(device));
	hipDeviceProp_t prop;
	HIPCHK(hipGetDeviceProperties(&prop, device));
	g->n_cu = prop.multiProcessorCount;
	const size_t N = (size_t)n_samp, M = n_markers;
	g->N = n_samp; g->M = M;
	g->bpvN = sgx_row_stride(n_samp);
	g->bpvM = (size_t)((M + 511) / 512) * 128;
	g->ntileN = 2 * (int)((N + 511) / 512);
	g->ntileM = 2 * (int)((M + 511) / 512);
	HIPCHK(g->stream.create(hipStreamNonBlocking));
	HIPCHK(g->G.alloc(M * g->bpvN));
	HIPCHK(g->Gt.alloc(N * g->bpvM));
	HIPCHK(hipMemsetAsync(g->G, 0, M * g->bpvN, g->stream));
	HIPCHK(hipMemsetAsync(g->Gt, 0, N * g->bpvM, g->stream));
	HIPCHK(hipMemcpy2DAsync(g->G, g->bpvN, packed, bytes_per_marker, std::min(bytes_per_marker, g->bpvN), M,
		kind, g->stream));
	for (DevBuf<double> *p : {&g->af, &g->inv, &g->l0}) HIPCHK(p->alloc(M));
	HIPCHK(g->diag.alloc(N));
	// scratch of a product: every launch zeroes what it reads of it
	HIPCHK(g->FlN.alloc((size_t)g->ntileN * 16 * (16 * GRM_MAXF) * 16));
	HIPCHK(g->FlM.alloc((size_t)g->ntileM * 16 * (16 * GRM_MAXF) * 16));
	HIPCHK(g->accV.alloc(M * 32 * GRM_MAXF));
	HIPCHK(g->accS.alloc(N * 32 * GRM_MAXF));
	HIPCHK(g->xv.alloc(GRM_GROUP * M));
	HIPCHK(g->gv.alloc(GRM_GROUP * M));
	HIPCHK(g->maxb.alloc(GRM_MAX_RHS * 3));
	HIPCHK(pcg_work_init(&g->pw, device, g->stream, n_samp));
	// marker statistics, transpose, diag(GRM)
	hipLaunchKernelGGL(grm_marker_stats, dim3((unsigned)M), dim3(256), 0, g->stream, g->G, g->bpvN, g->N, M, g->af, g->inv, g->l0);
	hipLaunchKernelGGL(transpose_2bit, dim3((unsigned)((N + 255) / 256), (unsigned)((M + 63) / 64)), dim3(256), 0, g->stream,
		g->G, g->bpvN, M, g->N, g->Gt, g->bpvM);
	hipLaunchKernelGGL(grm_diag_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, g->stream, g->Gt, g->bpvM, g->N, M,
		g->inv, g->l0, g->diag);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(g->stream));
	*out = hold.release();
	return SGX_OK;
}

extern "C" int sgx_grm_diag(sgx_grm *g, double *diag_out)
{
	if (!g || !diag_out) return fail(SGX_EINVAL, "sgx_grm_diag: NULL argument");
	HIPCHK(hipSetDevice(g->device));
	HIPCHK(hipMemcpy(diag_out, g->diag, (size_t)g->N * sizeof(double), hipMemcpyDeviceToHost));
	return SGX_OK;
}

// the marker table the operator standardises with: af_v and inv_v = 1 / sqrt(2 af_v (1 - af_v)) (0: monomorphic)
extern "C" int sgx_grm_marker_table(sgx_grm *g, double *af_out, double *inv_out)
{
	if (!g || !af_out || !inv_out) return fail(SGX_EINVAL, "sgx_grm_marker_table: NULL argument");
	HIPCHK(hipSetDevice(g->device));
	HIPCHK(hipMemcpy(af_out, g->af, g->M * sizeof(double), hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(inv_out, g->inv, g->M * sizeof(double), hipMemcpyDeviceToHost));
	return SGX_OK;
}

extern "C" int sgx_grm_sync(sgx_grm *g)
{
	if (!g) return fail(SGX_EINVAL, "sgx_grm_sync: NULL handle");
	HIPCHK(hipSetDevice(g->device));
	HIPCHK(hipStreamSynchronize(g->stream));
	return SGX_OK;
}

template <int NBFV>
static void grm_contract_launch(sgx_grm *g, const uint8_t *packed, size_t bpv, int rows, const uint8_t *Fl, int ntile, int *acc)
{
	MfTab tb{};
	tb.Fl = Fl; tb.ntile = ntile;
	int tps = 0;
	const dim3 grid = mf_grid(g->n_cu, (size_t)rows, ntile, &tps);
	const size_t lds = (size_t)2 * 16 * (16 * NBFV) * 16;
	hipLaunchKernelGGL((grm_contract_kernel<NBFV>), grid, dim3(WAVE * GRM_WAVES), lds, g->stream, packed, bpv, rows, tb, tps, acc, 32 * NBFV);
}

static void grm_contract(sgx_grm *g, int nbfv, const uint8_t *packed, size_t bpv, int rows, const uint8_t *Fl, int ntile, int *acc)
{
	switch (nbfv) {
	case 1: grm_contract_launch<1>(g, packed, bpv, rows, Fl, ntile, acc); break;
	case 2: grm_contract_launch<2>(g, packed, bpv, rows, Fl, ntile, acc); break;
	default: grm_contract_launch<GRM_MAXF>(g, packed, bpv, rows, Fl, ntile, acc); break;
	}
}

// ---- pass 1 up to its exact sums: per marker, over samples; column y of gc (at most GRM_GROUP) in fragment y / 2,
// limbs 7 (y % 2) ..  Leaves the columns' scales in g->maxb slot 0 and the sums in g->accV, for grm_dot_epilogue
// (the product) or grm_dot_out_kernel (sgx_grm_marker_dots): both read what the same launches wrote.
static int grm_pass1_sums(sgx_grm *g, const double *B, size_t ldb, const GrmCols &gc)
{
	hipStream_t st = g->stream;
	const size_t N = (size_t)g->N, M = g->M;
	const dim3 bl(256);
	const int nb1 = (gc.n + 1) / 2;
	HIPCHK(hipMemsetAsync(g->maxb, 0, (size_t)gc.n * 3 * sizeof(unsigned long long), st));
	hipLaunchKernelGGL(absmax_kernel, dim3(GRM_RED_BLOCKS, gc.n), bl, 0, st, B, ldb, gc, N, 0, g->maxb);
	HIPCHK(hipMemsetAsync(g->FlN, 0, (size_t)g->ntileN * 16 * (16 * nb1) * 16, st));
	hipLaunchKernelGGL(limbs_kernel, dim3(512, gc.n), bl, 0, st, B, ldb, gc, N, (size_t)g->ntileN * 256,
		16 * nb1, 2, 0, g->maxb, 0, g->FlN);
	HIPCHK(hipMemsetAsync(g->accV, 0, M * 32 * nb1 * sizeof(int), st));
	grm_contract(g, nb1, g->G, g->bpvN, (int)M, g->FlN, g->ntileN, g->accV);
	return SGX_OK;
}

// Out[:, c] = G'(G B[:, c])/M for c in cols (columns at base + c * ld), device vectors
// (get_crossprod_b_grm, saige_fitnull.cpp:435-536).  A column's result does not depend on the other
// columns of the call: its limbs, its exact integer sums and its reductions are its own.
// excl (NULL: the whole GRM, the plain kernels): excl[c] is the marker group column c leaves out, -1 for none
// (checked by grm_excl_args).  Only the two epilogues differ: the contraction and the limb steps are the same.
static int grm_matvec_dev(sgx_grm *g, const double *B, size_t ldb, const GrmCols &cols, double *Out, size_t ldo,
	const int *excl = nullptr)
{
	hipStream_t st = g->stream;
	const size_t N = (size_t)g->N, M = g->M;
	const dim3 bl(256);
	double sum_b[GRM_MAX_RHS];
	int rc = pcg_sum(&g->pw, B, nullptr, ldb, cols, sum_b);
	if (rc) return rc;
	for (int g0 = 0; g0 < cols.n; g0 += GRM_GROUP) {
		GrmCols gc{};
		gc.n = std::min(GRM_GROUP, cols.n - g0);
		GrmScal sb{};
		GrmIdx ex{};
		for (int y = 0; y < gc.n; y++) { gc.c[y] = cols.c[g0 + y]; sb.v[y] = sum_b[g0 + y]; ex.v[y] = excl ? excl[gc.c[y]] : -1; }
		const int nb1 = (gc.n + 1) / 2;
		if ((rc = grm_pass1_sums(g, B, ldb, gc))) return rc;
		if (excl)
			hipLaunchKernelGGL(grm_dot_epilogue<true>, dim3(GRM_RED_BLOCKS, gc.n), bl, 0, st, M, nb1, g->accV, g->maxb, sb,
				g->af, g->inv, g->l0, g->xv, g->gv, g->pw.part, g->grp, ex);
		else
			hipLaunchKernelGGL(grm_dot_epilogue<false>, dim3(GRM_RED_BLOCKS, gc.n), bl, 0, st, M, nb1, g->accV, g->maxb, sb,
				g->af, g->inv, g->l0, g->xv, g->gv, g->pw.part, g->grp, ex);
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpyAsync(g->pw.h_part, g->pw.part, (size_t)gc.n * GRM_RED_BLOCKS * sizeof(double), hipMemcpyDeviceToHost, st));
		HIPCHK(hipStreamSynchronize(st));
		GrmScal C0{};
		for (int y = 0; y < gc.n; y++) {
			double c0 = 0;
			for (int i = 0; i < GRM_RED_BLOCKS; i++) c0 += g->pw.h_part[(size_t)y * GRM_RED_BLOCKS + i];   // fixed order
			C0.v[y] = c0;
		}
		// ---- pass 2: per sample, over markers; column y of a sub-group in fragment y (x limbs 0.., gam limbs 7..)
		GrmCols all{};
		all.n = gc.n;
		for (int y = 0; y < gc.n; y++) all.c[y] = y;
		hipLaunchKernelGGL(absmax_kernel, dim3(GRM_RED_BLOCKS, gc.n), bl, 0, st, g->xv, M, all, M, 1, g->maxb);
		hipLaunchKernelGGL(absmax_kernel, dim3(GRM_RED_BLOCKS, gc.n), bl, 0, st, g->gv, M, all, M, 2, g->maxb);
		for (int s0 = 0; s0 < gc.n; s0 += GRM_GROUP2) {
			GrmCols sc{}, oc{};
			sc.n = oc.n = std::min(GRM_GROUP2, gc.n - s0);
			GrmScal c0s{}, msub{};
			GrmIdx ex2{};
			for (int y = 0; y < sc.n; y++) {
				sc.c[y] = s0 + y; oc.c[y] = gc.c[s0 + y]; c0s.v[y] = C0.v[s0 + y];
				ex2.v[y] = ex.v[s0 + y];
				msub.v[y] = (double)(M - (ex2.v[y] >= 0 ? g->gsize[ex2.v[y]] : 0));
			}
			const int nb2 = sc.n;
			const unsigned long long *mb = g->maxb + 3 * s0;
			HIPCHK(hipMemsetAsync(g->FlM, 0, (size_t)g->ntileM * 16 * (16 * nb2) * 16, st));
			hipLaunchKernelGGL(limbs_kernel, dim3(512, sc.n), bl, 0, st, g->xv, M, sc, M, (size_t)g->ntileM * 256,
				16 * nb2, 1, 0, mb, 1, g->FlM);
			hipLaunchKernelGGL(limbs_kernel, dim3(512, sc.n), bl, 0, st, g->gv, M, sc, M, (size_t)g->ntileM * 256,
				16 * nb2, 1, MF_NLIMB, mb, 2, g->FlM);
			HIPCHK(hipMemsetAsync(g->accS, 0, N * 32 * nb2 * sizeof(int), st));
			grm_contract(g, nb2, g->Gt, g->bpvM, g->N, g->FlM, g->ntileM, g->accS);
			if (excl)      // (no groups on the handle: every excl is -1 and only row 0 of the table is read)
				hipLaunchKernelGGL(grm_out_epilogue<true>, dim3((unsigned)((N + 255) / 256), sc.n), bl, 0, st, g->N, M, nb2,
					g->accS, mb, c0s, g->diagx ? g->diagx : g->diag, Out, ldo, oc, msub, ex2);
			else
				hipLaunchKernelGGL(grm_out_epilogue<false>, dim3((unsigned)((N + 255) / 256), sc.n), bl, 0, st, g->N, M, nb2,
					g->accS, mb, c0s, g->diag, Out, ldo, oc, msub, ex2);
			HIPCHK(hipGetLastError());
		}
	}
	return SGX_OK;
}

// Out = GRM B for k host vectors, column j at B + j * ldb (and Out + j * ldb)
static int grm_crossprod_run(sgx_grm *g, const double *B, size_t ldb, int k, double *Out, const int *excl = nullptr)
{
	return pcg_crossprod_run(&g->pw, B, ldb, k, Out,
		[&](const double *Bd, size_t ld, const GrmCols &cols, double *Od, size_t ldo) {
			return grm_matvec_dev(g, Bd, ld, cols, Od, ldo, excl);
		});
}

static int grm_multi_args(const char *fn, sgx_grm *g, const void *B, size_t ldb, int k, const void *Out)
{
	return pcg_multi_args(fn, g, g ? g->N : 0, B, ldb, k, Out);
}

// get_crossprod_b_grm: out = GRM b, host vectors of length N
extern "C" int sgx_grm_crossprod(sgx_grm *g, const double *b, double *out)
{
	if (!g || !b || !out) return fail(SGX_EINVAL, "sgx_grm_crossprod: NULL argument");
	return grm_crossprod_run(g, b, (size_t)g->N, 1, out);
}

extern "C" int sgx_grm_crossprod_multi(sgx_grm *g, const double *B, size_t ldb, int k, double *Out)
{
	int rc = grm_multi_args("sgx_grm_crossprod_multi", g, B, ldb, k, Out);
	if (rc) return rc;
	return grm_crossprod_run(g, B, ldb, k, Out);
}

// out = GRM b with b, out device vectors of N doubles (asynchronous until sgx_grm_sync)
extern "C" int sgx_grm_crossprod_dev(sgx_grm *g, const double *b_dev, double *out_dev)
{
	if (!g || !b_dev || !out_dev) return fail(SGX_EINVAL, "sgx_grm_crossprod_dev: NULL argument");
	HIPCHK(hipSetDevice(g->device));
	return grm_matvec_dev(g, b_dev, (size_t)g->N, pcg_cols_iota(1), out_dev, (size_t)g->N);
}

extern "C" int sgx_grm_crossprod_multi_dev(sgx_grm *g, const double *B_dev, size_t ldb, int k, double *Out_dev)
{
	int rc = grm_multi_args("sgx_grm_crossprod_multi_dev", g, B_dev, ldb, k, Out_dev);
	if (rc) return rc;
	HIPCHK(hipSetDevice(g->device));
	return grm_matvec_dev(g, B_dev, ldb, pcg_cols_iota(k), Out_dev, ldb);
}

// ---- the marker side of the product as an output: Out[c][v] = dot_v of column c = sum_i G[v, i] B[i, c], device
// vectors (Out row c at Out + c * ldo).  The launches of pass 1 of grm_matvec_dev, group by group; the epilogue's place
// is taken by grm_dot_out_kernel.  Marker groups are ignored.
static int grm_marker_dots_run(sgx_grm *g, const double *B, size_t ldb, int k, double *Out, size_t ldo)
{
	const GrmCols cols = pcg_cols_iota(k);
	double sum_b[GRM_MAX_RHS];
	int rc = pcg_sum(&g->pw, B, nullptr, ldb, cols, sum_b);
	if (rc) return rc;
	for (int g0 = 0; g0 < k; g0 += GRM_GROUP) {
		GrmCols gc{};
		gc.n = std::min(GRM_GROUP, k - g0);
		GrmScal sb{};
		for (int y = 0; y < gc.n; y++) { gc.c[y] = cols.c[g0 + y]; sb.v[y] = sum_b[g0 + y]; }
		if ((rc = grm_pass1_sums(g, B, ldb, gc))) return rc;
		hipLaunchKernelGGL(grm_dot_out_kernel, dim3(GRM_RED_BLOCKS, gc.n), dim3(256), 0, g->stream, g->M, (gc.n + 1) / 2,
			g->accV, g->maxb, sb, g->inv, g->l0, Out, ldo, gc);
		HIPCHK(hipGetLastError());
	}
	return SGX_OK;
}

static int grm_marker_dots_args(const char *fn, sgx_grm *g, const void *B, size_t ldb, int k, const void *Out, size_t ldo)
{
	int rc = grm_multi_args(fn, g, B, ldb, k, Out);
	if (rc) return rc;
	if (ldo < g->M) return fail(SGX_EINVAL, "%s: ldo=%zu < M=%zu", fn, ldo, g->M);
	return SGX_OK;
}

extern "C" int sgx_grm_marker_dots_dev(sgx_grm *g, const double *B_dev, size_t ldb, int k, double *Out_dev, size_t ldo)
{
	int rc = grm_marker_dots_args("sgx_grm_marker_dots_dev", g, B_dev, ldb, k, Out_dev, ldo);
	if (rc) return rc;
	HIPCHK(hipSetDevice(g->device));
	return grm_marker_dots_run(g, B_dev, ldb, k, Out_dev, ldo);
}

extern "C" int sgx_grm_marker_dots(sgx_grm *g, const double *B, size_t ldb, int k, double *Out, size_t ldo)
{
	int rc = grm_marker_dots_args("sgx_grm_marker_dots", g, B, ldb, k, Out, ldo);
	if (rc) return rc;
	HIPCHK(hipSetDevice(g->device));
	HIPCHK(pcg_reserve(&g->pw, k));
	HIPCHK(g->md_out.reserve((size_t)k * g->M));
	const size_t N = (size_t)g->N, M = g->M;
	HIPCHK(pcg_copy_cols(&g->pw, g->pw.B, B, ldb, k, hipMemcpyHostToDevice));
	if ((rc = grm_marker_dots_run(g, g->pw.B, N, k, g->md_out, M))) return rc;
	HIPCHK(hipMemcpy2DAsync(Out, ldo * sizeof(double), g->md_out, M * sizeof(double), M * sizeof(double), (size_t)k,
		hipMemcpyDeviceToHost, g->stream));
	HIPCHK(hipStreamSynchronize(g->stream));
	return SGX_OK;
}

// PCG_diag_sigma (saige_fitnull.cpp:581-614) on the implicit GRM: the loop is pcg_run (host_pcg.h).
// excl (NULL: the whole GRM for all columns): column j leaves out group excl[j] and, with pc, has its own weights
// and diagonal (sgx_grm_pcg_loco).
static int grm_pcg_run(sgx_grm *g, const double *w, const double *tau, const double *B, size_t ldb, int k,
	int maxiter, double tol, double *X_out, int *iters, const int *excl = nullptr, const PcgPerCol *pc = nullptr)
{
	return pcg_run(&g->pw, g->diag, w, tau, B, ldb, k, maxiter, tol, X_out, iters,
		[&](const double *Bd, size_t ld, const GrmCols &cols, double *Od, size_t ldo) {
			return grm_matvec_dev(g, Bd, ld, cols, Od, ldo, excl);
		}, pc);
}

extern "C" int sgx_grm_pcg(sgx_grm *g, const double *w, const double *tau, const double *b,
	int maxiter, double tol, double *x_out, int *iters_out)
{
	if (!g || !w || !tau || !b || !x_out) return fail(SGX_EINVAL, "sgx_grm_pcg: NULL argument");
	int iters = 0;
	int rc = grm_pcg_run(g, w, tau, b, (size_t)g->N, 1, maxiter, tol, x_out, &iters);
	if (rc) return rc;
	if (iters_out) *iters_out = iters;
	return SGX_OK;
}

extern "C" int sgx_grm_pcg_multi(sgx_grm *g, const double *w, const double *tau, const double *B, size_t ldb, int k,
	int maxiter, double tol, double *X_out, int *iters)
{
	if (!w || !tau || !iters) return fail(SGX_EINVAL, "sgx_grm_pcg_multi: NULL argument");
	int rc = grm_multi_args("sgx_grm_pcg_multi", g, B, ldb, k, X_out);
	if (rc) return rc;
	return grm_pcg_run(g, w, tau, B, ldb, k, maxiter, tol, X_out, iters);
}

// ===========================================================================
// Marker groups and leave-one-group-out columns (LOCO: a variant of chromosome c is tested against a null
// model whose GRM leaves out the markers of c).  Column j of a *_loco call works on the GRM of the markers
// outside group excl[j]: pass 1 zeroes the excluded markers' dot products, pass 2 divides by M - M_excl, and
// the diagonal is the matching one.  The genotype sweeps are shared by all columns of a call.

extern "C" int sgx_grm_set_groups(sgx_grm *g, const int32_t *group, int n_groups)
{
	if (!g || !group) return fail(SGX_EINVAL, "sgx_grm_set_groups: NULL argument");
	if (n_groups < 1 || n_groups > SGX_GRM_MAX_GROUPS)
		return fail(SGX_EINVAL, "sgx_grm_set_groups: n_groups=%d outside 1..%d", n_groups, SGX_GRM_MAX_GROUPS);
	const size_t N = (size_t)g->N, M = g->M;
	size_t sizes[GRM_MAX_GROUPS] = {};
	for (size_t v = 0; v < M; v++) {
		if (group[v] < 0 || group[v] >= n_groups)
			return fail(SGX_EINVAL, "sgx_grm_set_groups: group[%zu]=%d outside 0..%d", v, (int)group[v], n_groups - 1);
		sizes[group[v]]++;
	}
	HIPCHK(hipSetDevice(g->device));
	hipStream_t st = g->stream;
	HIPCHK(hipStreamSynchronize(st));
	g->n_groups = 0;                       // (no groups until the new tables are complete)
	HIPCHK(g->grp.reserve(M));
	HIPCHK(g->diagx.alloc((size_t)(1 + n_groups) * N));
	DevBuf<double> S, msub;                // the call's scratch: the synchronisation below comes before their release
	double h_msub[GRM_MAX_GROUPS];
	for (int c = 0; c < n_groups; c++) h_msub[c] = (double)(M - sizes[c]);
	HIPCHK(S.alloc((size_t)n_groups * N));
	HIPCHK(msub.alloc(GRM_MAX_GROUPS));
	HIPCHK(hipMemcpyAsync(g->grp, group, M * sizeof(int), hipMemcpyHostToDevice, st));
	HIPCHK(hipMemcpyAsync(msub, h_msub, (size_t)n_groups * sizeof(double), hipMemcpyHostToDevice, st));
	hipLaunchKernelGGL(grm_diag_groups_kernel, dim3((unsigned)N), dim3(WAVE), (size_t)n_groups * WAVE * sizeof(double), st,
		g->Gt, g->bpvM, g->N, M, g->inv, g->l0, g->grp, n_groups, S);
	hipLaunchKernelGGL(grm_diag_excl_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, g->N, n_groups, S, msub,
		g->diag, g->diagx);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(st));
	for (int c = 0; c < GRM_MAX_GROUPS; c++) g->gsize[c] = sizes[c];
	g->n_groups = n_groups;
	return SGX_OK;
}

extern "C" int sgx_grm_group_sizes(sgx_grm *g, int64_t *sizes_out)
{
	if (!g || !sizes_out) return fail(SGX_EINVAL, "sgx_grm_group_sizes: NULL argument");
	if (g->n_groups == 0) return fail(SGX_EINVAL, "sgx_grm_group_sizes: no marker groups (sgx_grm_set_groups)");
	for (int c = 0; c < g->n_groups; c++) sizes_out[c] = (int64_t)g->gsize[c];
	return SGX_OK;
}

// excl[k] of a *_loco call -> out[k]: checked, and an empty group (excluding it is excluding nothing) as -1
static int grm_excl_args(const char *fn, sgx_grm *g, const int *excl, int k, int *out)
{
	if (!excl) return fail(SGX_EINVAL, "%s: NULL argument", fn);
	for (int j = 0; j < k; j++) {
		const int c = excl[j];
		if (c < -1) return fail(SGX_EINVAL, "%s: excl[%d]=%d (a group, or -1 for none)", fn, j, c);
		if (c >= 0 && g->n_groups == 0) return fail(SGX_EINVAL, "%s: excl[%d]=%d before sgx_grm_set_groups", fn, j, c);
		if (c >= g->n_groups && c >= 0) return fail(SGX_EINVAL, "%s: excl[%d]=%d outside -1..%d", fn, j, c, g->n_groups - 1);
		if (c >= 0 && g->gsize[c] == g->M)
			return fail(SGX_EINVAL, "%s: excl[%d]=%d leaves no marker (the group holds all %zu)", fn, j, c, g->M);
		out[j] = (c >= 0 && g->gsize[c] == 0) ? -1 : c;
	}
	return SGX_OK;
}

extern "C" int sgx_grm_diag_loco(sgx_grm *g, int excl, double *diag_out)
{
	if (!g || !diag_out) return fail(SGX_EINVAL, "sgx_grm_diag_loco: NULL argument");
	int ex = -1;
	int rc = grm_excl_args("sgx_grm_diag_loco", g, &excl, 1, &ex);
	if (rc) return rc;
	HIPCHK(hipSetDevice(g->device));
	const double *src = ex < 0 ? g->diag : g->diagx + (size_t)(1 + ex) * g->N;
	HIPCHK(hipMemcpy(diag_out, src, (size_t)g->N * sizeof(double), hipMemcpyDeviceToHost));
	return SGX_OK;
}

extern "C" int sgx_grm_crossprod_loco(sgx_grm *g, const double *B, size_t ldb, int k, const int *excl, double *Out)
{
	int rc = grm_multi_args("sgx_grm_crossprod_loco", g, B, ldb, k, Out);
	if (rc) return rc;
	int ex[GRM_MAX_RHS];
	if ((rc = grm_excl_args("sgx_grm_crossprod_loco", g, excl, k, ex))) return rc;
	return grm_crossprod_run(g, B, ldb, k, Out, ex);
}

extern "C" int sgx_grm_pcg_loco(sgx_grm *g, const double *W, size_t ldw, int n_w, const int *w_idx, const double *tau,
	const double *B, size_t ldb, int k, const int *excl, int maxiter, double tol, double *X_out, int *iters)
{
	if (!W || !w_idx || !tau || !iters) return fail(SGX_EINVAL, "sgx_grm_pcg_loco: NULL argument");
	int rc = grm_multi_args("sgx_grm_pcg_loco", g, B, ldb, k, X_out);
	if (rc) return rc;
	if (n_w < 1 || n_w > SGX_GRM_MAX_RHS) return fail(SGX_EINVAL, "sgx_grm_pcg_loco: n_w=%d outside 1..%d", n_w, SGX_GRM_MAX_RHS);
	if (ldw < (size_t)g->N) return fail(SGX_EINVAL, "sgx_grm_pcg_loco: ldw=%zu < N=%d", ldw, g->N);
	for (int j = 0; j < k; j++)
		if (w_idx[j] < 0 || w_idx[j] >= n_w)
			return fail(SGX_EINVAL, "sgx_grm_pcg_loco: w_idx[%d]=%d outside 0..%d", j, w_idx[j], n_w - 1);
	int ex[GRM_MAX_RHS];
	if ((rc = grm_excl_args("sgx_grm_pcg_loco", g, excl, k, ex))) return rc;
	const PcgPerCol pc{W, ldw, n_w, w_idx, ex, g->diagx ? g->diagx : g->diag};
	return grm_pcg_run(g, nullptr, tau, B, ldb, k, maxiter, tol, X_out, iters, ex, &pc);
}
