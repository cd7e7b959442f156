// host_skat.h -- the SKAT set test's score vector and covariance matrix per unit from 2-bit rows in host
// memory: the rows and tables go to the device once, kern_skat.h makes the Gram tiles and the dense sums, the host
// turns them into S and Phi by the scan's own algebra in double.  The checks of the units, the tile
// plan, the slab sum and that last step are functions of their own: sgx_ds_block_skat (host_skat_ds.h) runs the same
// ones on the dosage rows of a resident block.
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.

static const int SKAT_SLAB_DW = 256;                        // dwords (of 16 samples) per sample slab: cut by N alone
static const size_t SKAT_PART_BYTES = (size_t)256 << 20;    // per-slab partial tiles of one launch

// The units of a call: sizes first, so that nothing is read through a unit_ptr that is out of bounds, then the
// indices against the n_rows rows they point into.
static int skat_units_check(const char *who, size_t n_units, const int64_t *unit_ptr, const int32_t *var_idx, size_t n_rows)
{
	if (unit_ptr[0] != 0) return fail(SGX_EINVAL, "%s: bad unit_ptr", who);
	for (size_t u = 0; u < n_units; u++) {
		const int64_t m = unit_ptr[u + 1] - unit_ptr[u];
		if (m < 0) return fail(SGX_EINVAL, "%s: unit_ptr not ascending", who);
		if (m > SGX_SKAT_MAX_VARIANTS)
			return fail(SGX_EINVAL, "%s: unit %zu has %lld variants, at most %d are supported", who, u, (long long)m, SGX_SKAT_MAX_VARIANTS);
	}
	const int32_t *bad;
	int rc = csr_check(who, "unit_ptr", n_units, unit_ptr, var_idx, n_rows, &bad);
	if (rc) return rc;
	if (bad) return fail(SGX_EINVAL, "%s: variant index %d out of range", who, *bad);
	return SGX_OK;
}

// The tiles of a call: per unit the variant tiles with tile_col >= tile_row, then the row tile against the 2K+1
// columns of F; tchunk of them per launch, so that their per-slab partial tiles fit SKAT_PART_BYTES.
struct SkatPlan {
	std::vector<SkatTile> tiles;
	std::vector<uint32_t> tile_unit;
	int nslab = 0;
	size_t tchunk = 0;
};

static void skat_plan(SkatPlan &pl, size_t n_units, const int64_t *unit_ptr, int C, int nslab)
{
	const int n_dt = (C + 15) / 16;
	for (size_t u = 0; u < n_units; u++) {
		const int64_t e0 = unit_ptr[u], m = unit_ptr[u + 1] - e0;
		const int n_vt = (int)((m + 15) / 16);
		for (int tr = 0; tr < n_vt; tr++) {
			SkatTile t{};
			t.row_e0 = e0 + 16 * tr; t.nrow = (int)std::min<int64_t>(16, m - 16 * tr);
			for (int tc = tr; tc < n_vt; tc++) {
				t.col_e0 = e0 + 16 * tc; t.ncol = (int)std::min<int64_t>(16, m - 16 * tc); t.dense = 0;
				pl.tiles.push_back(t); pl.tile_unit.push_back((uint32_t)u);
			}
			for (int dt = 0; dt < n_dt; dt++) {
				t.col_e0 = 16 * dt; t.ncol = std::min(16, C - 16 * dt); t.dense = 1;
				pl.tiles.push_back(t); pl.tile_unit.push_back((uint32_t)u);
			}
		}
	}
	pl.nslab = nslab;
	const size_t T = pl.tiles.size();
	pl.tchunk = std::min(T, std::max<size_t>(1, SKAT_PART_BYTES / ((size_t)nslab * 256 * sizeof(double))));
}

// The plan's tiles, tchunk at a time: launch(t0, nt) queues the Gram kernel of tiles [t0, t0 + nt) into h->skat_part
// (grown here, with h->skat_fin); the slabs are added in slab order and the tiles scattered: W into cov (upper
// triangle, unit by unit), the dense sums into `dense` [entry][2K+1].
template <class Launch>
static int skat_run(sgx_handle *h, const SkatPlan &pl, size_t n_units, const int64_t *unit_ptr, int C, Launch launch,
	std::vector<double> &dense, double *cov)
{
	const size_t T = pl.tiles.size(), tchunk = pl.tchunk;
	const int nslab = pl.nslab;
	int rc = grow(h->skat_part, tchunk * (size_t)nslab * 256);
	if (rc) return rc;
	rc = grow(h->skat_fin, tchunk * 256);
	if (rc) return rc;
	std::vector<size_t> cov_off(n_units + 1, 0);
	for (size_t u = 0; u < n_units; u++) {
		const size_t m = (size_t)(unit_ptr[u + 1] - unit_ptr[u]);
		cov_off[u + 1] = cov_off[u] + m * m;
	}
	dense.assign((size_t)unit_ptr[n_units] * C, 0.0);
	std::vector<double> fin(tchunk * 256);
	for (size_t t0 = 0; t0 < T; t0 += tchunk) {
		const size_t nt = std::min(tchunk, T - t0);
		launch(t0, nt);
		HIPCHK(hipGetLastError());
		hipLaunchKernelGGL(skat_reduce_kernel, dim3((unsigned)nt), dim3(256), 0, h->stream,
			h->skat_part, nt * 256, nslab, h->skat_fin);
		HIPCHK(hipGetLastError());
		HIPCHK(hipMemcpyAsync(fin.data(), h->skat_fin, nt * 256 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
		HIPCHK(hipStreamSynchronize(h->stream));
		for (size_t k = 0; k < nt; k++) {
			const SkatTile &t = pl.tiles[t0 + k];
			const double *f = &fin[k * 256];
			const size_t u = pl.tile_unit[t0 + k];
			const int64_t e0 = unit_ptr[u];
			const size_t m = (size_t)(unit_ptr[u + 1] - e0), r0 = (size_t)(t.row_e0 - e0);
			if (t.dense) {
				for (int i = 0; i < t.nrow; i++)
					for (int j = 0; j < t.ncol; j++) dense[(size_t)(t.row_e0 + i) * C + t.col_e0 + j] = f[i * 16 + j];
			} else {
				const size_t c0 = (size_t)(t.col_e0 - e0);
				double *w = cov + cov_off[u];
				for (int i = 0; i < t.nrow; i++)
					for (int j = (c0 == r0 ? i : 0); j < t.ncol; j++) w[(r0 + i) * m + c0 + j] = f[i * 16 + j];
			}
		}
	}
	return SGX_OK;
}

// From the dense sums [entry][2K+1] (c', e, s of DESIGN.md 3.1) and W (the upper triangles in cov) to
//     S_j = s_j - S_a c'_j;  Phi_jl = r (c'_j XVX c'_l + W_jl - e_j c'_l - e_l c'_j), j <= l, mirrored
// -- the one place where this is done, for 2-bit rows and for dosage rows.
static void skat_finish(const DevModel &md, size_t n_units, const int64_t *unit_ptr, const std::vector<double> &dense,
	double *score, double *cov)
{
	const int K = md.K, C = 2 * K + 1;
	std::vector<double> q;
	size_t off = 0;
	for (size_t u = 0; u < n_units; u++) {
		const int64_t e0 = unit_ptr[u];
		const size_t m = (size_t)(unit_ptr[u + 1] - e0);
		if (m == 0) continue;
		double *phi = cov + off;
		off += m * m;
		q.assign(m * K, 0.0);
		for (size_t j = 0; j < m; j++) {
			const double *cj = &dense[(size_t)(e0 + j) * C];
			double sa = 0;
			for (int a = 0; a < K; a++) {
				double x = 0;
				for (int b = 0; b < K; b++) x += md.XVX[a * K + b] * cj[b];
				q[j * K + a] = x;
				sa += md.S_a[a] * cj[a];
			}
			const double S = cj[2 * K] - sa;
			score[e0 + j] = md.quant ? S / md.tau0 : S;
		}
		for (size_t j = 0; j < m; j++) {
			const double *cj = &dense[(size_t)(e0 + j) * C], *ej = cj + K;
			for (size_t l = j; l < m; l++) {
				const double *cl = &dense[(size_t)(e0 + l) * C], *el = cl + K, *ql = &q[l * K];
				double cq = 0, ec = 0;
				for (int a = 0; a < K; a++) { cq += cj[a] * ql[a]; ec += ej[a] * cl[a] + el[a] * cj[a]; }
				const double v = md.r * (cq + phi[j * m + l] - ec);
				phi[j * m + l] = v;
				phi[l * m + j] = v;
			}
		}
	}
}

// sgx_skat_2bit; `dense` keeps the entries' dense sums [entry][2K+1] for a caller that wants them (sgx_cond_set).
static int skat_2bit_host(sgx_handle *h, const uint8_t *packed, size_t bpv, size_t n_variants,
	size_t n_units, const int64_t *unit_ptr, const int32_t *var_idx, const double *lut,
	double *score, double *cov, std::vector<double> &dense)
{
	if (!h) return fail(SGX_EINVAL, "sgx_skat_2bit: NULL handle");
	if (n_units == 0) return SGX_OK;
	if (!packed || !unit_ptr || !var_idx || !lut || !score || !cov)
		return fail(SGX_EINVAL, "sgx_skat_2bit: NULL buffer");
	const int N = h->md.N, K = h->md.K, P = h->md.P, C = 2 * K + 1;
	int rc = bpv_check(bpv, N);
	if (!rc) rc = skat_units_check("sgx_skat_2bit", n_units, unit_ptr, var_idx, n_variants);
	if (rc) return rc;
	const int64_t nnz = unit_ptr[n_units];
	if (nnz == 0) return SGX_OK;
	rc = begin_call(h);
	if (rc) return rc;

	const int ndw = (N + 15) >> 4;
	SkatPlan pl;
	skat_plan(pl, n_units, unit_ptr, C, (ndw + SKAT_SLAB_DW - 1) / SKAT_SLAB_DW);

	// device copies: the rows (dword stride) in the host-row pipeline's chunks, then entries, tables, tiles
	const size_t dbpv = (size_t)ndw * 4;
	TabLayout tl;
	tl.add<uint8_t>(n_variants * dbpv);
	const auto s_idx = tl.add(nnz, var_idx);
	const auto s_lut = tl.add(nnz * 4, lut);
	const auto s_til = tl.add(pl.tiles.size(), pl.tiles.data());
	rc = grow(h->stage_pk, tl.bytes());
	if (rc) return rc;
	rc = rows_2bit_upload(h, h->stage_pk, dbpv, packed, bpv, n_variants, h->stream);
	if (rc) return rc;
	rc = tabs_upload(h->stage_pk, h->stream, s_idx, s_lut, s_til);
	if (rc) return rc;

	rc = skat_run(h, pl, n_units, unit_ptr, C, [&](size_t t0, size_t nt) {
		hipLaunchKernelGGL(skat_gram_kernel, dim3((unsigned)nt, (unsigned)pl.nslab), dim3(64), 0, h->stream,
			h->stage_pk, dbpv, N, tl.at(h->stage_pk, s_idx), tl.at(h->stage_pk, s_lut), h->md.F, P,
			tl.at(h->stage_pk, s_til) + t0, nt, SKAT_SLAB_DW, h->skat_part);
	}, dense, cov);
	if (rc) return rc;
	skat_finish(h->md, n_units, unit_ptr, dense, score, cov);
	return SGX_OK;
}

extern "C" int sgx_skat_2bit(sgx_handle *h, const uint8_t *packed, size_t bpv, size_t n_variants,
	size_t n_units, const int64_t *unit_ptr, const int32_t *var_idx, const double *lut,
	double *score, double *cov)
{
	std::vector<double> dense;
	return skat_2bit_host(h, packed, bpv, n_variants, n_units, unit_ptr, var_idx, lut, score, cov, dense);
}
