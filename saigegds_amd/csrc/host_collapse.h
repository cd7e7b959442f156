// host_collapse.h -- the pseudo-variants of groups of 2-bit rows (kern_collapse.h): sgx_collapse_2bit_dev
// queues the kernel for rows in device memory, sgx_collapse_2bit is its wrapper for rows in host memory.
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.  The checks of a
// call's groups are plain C++, tested on their own (tests/collapse_check.cpp): what follows COLLAPSE_CHECK_ONLY needs HIP.
#include <stddef.h>
#include <stdint.h>

// The groups of a call (CSR in host memory), in two steps so that nothing is read through a list that is not sound:
// grp_ptr as a whole first -- after it var_idx has grp_ptr[n_groups] entries --, then every index against the
// n_variants rows.  *at: the group or the entry that is wrong.
enum { COLLAPSE_OK = 0, COLLAPSE_PTR0, COLLAPSE_DESCEND, COLLAPSE_INDEX };

static int collapse_ptr_check(size_t n_groups, const int64_t *grp_ptr, size_t *at)
{
	*at = 0;
	if (grp_ptr[0] != 0) return COLLAPSE_PTR0;
	for (size_t g = 0; g < n_groups; g++)
		if (grp_ptr[g + 1] < grp_ptr[g]) { *at = g; return COLLAPSE_DESCEND; }
	return COLLAPSE_OK;
}

static int collapse_idx_check(size_t nnz, const int32_t *var_idx, size_t n_variants, size_t *at)
{
	for (size_t e = 0; e < nnz; e++)
		if (var_idx[e] < 0 || (size_t)var_idx[e] >= n_variants) { *at = e; return COLLAPSE_INDEX; }
	return COLLAPSE_OK;
}

#ifndef COLLAPSE_CHECK_ONLY
static int collapse_fail(const char *who, int code, size_t at, size_t n_variants)
{
	switch (code) {
	case COLLAPSE_OK: return SGX_OK;
	case COLLAPSE_PTR0: return fail(SGX_EINVAL, "%s: bad grp_ptr", who);
	case COLLAPSE_DESCEND: return fail(SGX_EINVAL, "%s: grp_ptr not ascending at group %zu", who, at);
	default: return fail(SGX_EINVAL, "%s: variant index of entry %zu outside the %zu rows", who, at, n_variants);
	}
}

// n_groups checked groups over rows in device memory -> out_rows (at the rows' stride) and counts, queued on the
// handle's stream: the counts are zeroed, then a workgroup per (group, slab of COLLAPSE_SLAB bytes); beyond 2^20
// workgroups they loop.  No scratch.
static int collapse_rows_dev(sgx_handle *h, const uint8_t *rows, size_t bpv, size_t n_groups, const int64_t *grp_ptr,
	const int32_t *var_idx, const uint8_t *flip, uint8_t *out_rows, int32_t *counts)
{
	HIPCHK(hipMemsetAsync(counts, 0, n_groups * 2 * sizeof(int32_t), h->stream));
	const size_t total = n_groups * ((bpv + COLLAPSE_SLAB - 1) / COLLAPSE_SLAB);
	hipLaunchKernelGGL(collapse_kernel, dim3((unsigned)std::min(total, (size_t)1 << 20)), dim3(COLLAPSE_BLOCK), 0, h->stream,
		rows, bpv, h->md.N, n_groups, grp_ptr, var_idx, flip, out_rows, counts);
	HIPCHK(hipGetLastError());
	return SGX_OK;
}

extern "C" int sgx_collapse_2bit_dev(sgx_handle *h, const uint8_t *packed_dev, size_t bpv, size_t n_variants, size_t n_groups,
	const int64_t *grp_ptr_dev, const int32_t *var_idx_dev, const uint8_t *flip_dev, uint8_t *out_rows_dev, int32_t *counts_dev)
{
	const char *who = "sgx_collapse_2bit_dev";
	if (!h) return fail(SGX_EINVAL, "%s: NULL handle", who);
	if (n_groups == 0) return SGX_OK;
	if (!packed_dev || !grp_ptr_dev || !var_idx_dev || !flip_dev || !out_rows_dev || !counts_dev)
		return fail(SGX_EINVAL, "%s: NULL buffer", who);
	int rc = dev_rows_check(who, packed_dev, bpv, h->md.N);
	if (rc) return rc;
	if (((uintptr_t)out_rows_dev & 15u) != 0 || ((uintptr_t)grp_ptr_dev & 7u) != 0 || (((uintptr_t)var_idx_dev | (uintptr_t)counts_dev) & 3u) != 0)
		return fail(SGX_EINVAL, "%s: out_rows_dev must be 16-byte aligned, grp_ptr_dev 8-byte, var_idx_dev and counts_dev 4-byte", who);
	rc = set_dev(h);
	if (rc) return rc;
	// the kernel reads rows through the groups: they come back to the host to be checked, behind what the stream holds
	size_t at;
	std::vector<int64_t> gp(n_groups + 1);
	HIPCHK(hipMemcpyAsync(gp.data(), grp_ptr_dev, gp.size() * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipStreamSynchronize(h->stream));
	rc = collapse_fail(who, collapse_ptr_check(n_groups, gp.data(), &at), at, n_variants);
	if (rc) return rc;
	std::vector<int32_t> vi((size_t)gp[n_groups]);
	if (!vi.empty()) {
		HIPCHK(hipMemcpyAsync(vi.data(), var_idx_dev, vi.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
		HIPCHK(hipStreamSynchronize(h->stream));
	}
	rc = collapse_fail(who, collapse_idx_check(vi.size(), vi.data(), n_variants, &at), at, n_variants);
	if (rc) return rc;
	return collapse_rows_dev(h, packed_dev, bpv, n_groups, grp_ptr_dev, var_idx_dev, flip_dev, out_rows_dev, counts_dev);
}

extern "C" int sgx_collapse_2bit(sgx_handle *h, const uint8_t *packed, size_t bpv, size_t n_variants, size_t n_groups,
	const int64_t *grp_ptr, const int32_t *var_idx, const uint8_t *flip, uint8_t *out_rows, int32_t *counts)
{
	const char *who = "sgx_collapse_2bit";
	if (!h) return fail(SGX_EINVAL, "%s: NULL handle", who);
	if (n_groups == 0) return SGX_OK;
	if (!packed || !grp_ptr || !var_idx || !flip || !out_rows || !counts) return fail(SGX_EINVAL, "%s: NULL buffer", who);
	size_t at;
	int rc = bpv_check(bpv, h->md.N);
	if (!rc) rc = collapse_fail(who, collapse_ptr_check(n_groups, grp_ptr, &at), at, n_variants);
	if (rc) return rc;
	const size_t nnz = (size_t)grp_ptr[n_groups];
	rc = collapse_fail(who, collapse_idx_check(nnz, var_idx, n_variants, &at), at, n_variants);
	if (!rc) rc = sync_lane(h);             // (not begin_call: this entry leaves last_issued as it is)
	if (rc) return rc;

	// device copies: the rows at the device stride in the host-row chunks, the groups, then room for the results
	const size_t dbpv = sgx_row_stride(h->md.N);
	TabLayout tl;
	tl.add<uint8_t>(n_variants * dbpv);
	const auto s_ptr = tl.add(n_groups + 1, grp_ptr);
	const auto s_idx = tl.add(nnz, var_idx);
	const auto s_flip = tl.add(nnz, flip);
	const auto s_rows = tl.add<uint8_t>(n_groups * dbpv);
	const auto s_cnt = tl.add<int32_t>(n_groups * 2);
	rc = grow(h->stage_pk, tl.bytes());
	if (!rc) rc = rows_2bit_upload(h, h->stage_pk, dbpv, packed, bpv, n_variants, h->stream);
	if (!rc) rc = tabs_upload(h->stage_pk, h->stream, s_ptr, s_idx, s_flip);
	if (!rc) rc = collapse_rows_dev(h, h->stage_pk, dbpv, n_groups, tl.at(h->stage_pk, s_ptr), tl.at(h->stage_pk, s_idx),
		tl.at(h->stage_pk, s_flip), tl.at(h->stage_pk, s_rows), tl.at(h->stage_pk, s_cnt));
	if (rc) return rc;
	if (bpv > dbpv) memset(out_rows, 0, n_groups * bpv);           // what a longer host row has more is zero
	HIPCHK(hipMemcpy2DAsync(out_rows, bpv, tl.at(h->stage_pk, s_rows), dbpv, std::min(bpv, dbpv), n_groups,
		hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipMemcpyAsync(counts, tl.at(h->stage_pk, s_cnt), n_groups * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
	HIPCHK(hipStreamSynchronize(h->stream));
	return SGX_OK;
}
#endif
