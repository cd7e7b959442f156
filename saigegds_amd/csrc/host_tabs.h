// host_tabs.h -- what the entries beyond the single-variant scan share on the host: the layout of a call's tables in one
// device byte buffer (h->stage_pk, a block's tabs) with their upload, the dosage-type dispatch, and the argument checks
// whose texts are the same everywhere.  Part of libsaigehip.so: included by saigehip.hip (one translation unit); the
// layout itself is plain C++, tested on its own (tests/tab_layout_check.cpp): what follows TAB_LAYOUT_ONLY needs HIP.
#include <stddef.h>
#include <stdint.h>

// n elements of T at byte `off` of the buffer; src: the n elements in host memory, or nullptr for a slot that the
// device writes or that tab_copy fills a chunk at a time
template <class T>
struct TabSlot { size_t off = 0, n = 0; const T *src = nullptr; };

// The one place where the offset and alignment of a device table are decided.  Every slot starts on a 16-byte
// boundary (no less than any table had when each entry rounded for itself; SkatTile holds a long long); a slot of no
// elements is legal and takes no room.  The layout does not allocate: the caller reserves bytes() with the function
// whose error it wants (host_mem.h) and hands the base to at() and the uploads.
struct TabLayout {
	size_t total = 0;
	template <class T>
	TabSlot<T> add(size_t n, const T *src = nullptr)
	{
		const TabSlot<T> s{total, n, src};
		total = (total + n * sizeof(T) + 15) & ~(size_t)15;
		return s;
	}
	size_t bytes() const { return total; }
	template <class T>
	static T *at(uint8_t *base, TabSlot<T> s) { return reinterpret_cast<T *>(base + s.off); }
};

#ifndef TAB_LAYOUT_ONLY
static_assert(sizeof(int) == sizeof(int32_t), "var_idx, m_of: the callers' int32_t lists go to the device as int");

// queues the copy of m <= s.n elements from src to the front of slot s
template <class T>
static int tab_copy(uint8_t *base, TabSlot<T> s, const T *src, size_t m, hipStream_t st)
{
	if (m > s.n) return fail(SGX_EINVAL, "tab_copy: %zu elements into a slot of %zu", m, s.n);
	if (m) HIPCHK(hipMemcpyAsync(base + s.off, src, m * sizeof(T), hipMemcpyHostToDevice, st));
	return SGX_OK;
}

// queues the copies of those of the slots that have a host source, which stays the caller's until the stream has run them
template <class... S>
static int tabs_upload(uint8_t *base, hipStream_t st, const S &...slots)
{
	int rc = SGX_OK;
	((rc = rc ? rc : tab_copy(base, slots, slots.src, slots.src ? slots.n : 0, st)), ...);
	return rc;
}

// f(rows, T()) with a dosage block's rows (the buffer's address, DevBuf::p) as what they are: const T *rows with T =
// uint8_t (SGX_DS_U8) or double (i32 rows are stored as doubles); T() names T for the kernel template (cf. with_k, host_spa.h)
template <typename F>
static void with_ds_rows(int dtype, const void *rows, F &&f)
{
	if (dtype == SGX_DS_U8) f(static_cast<const uint8_t *>(rows), uint8_t());
	else f(static_cast<const double *>(rows), double());
}

// 2-bit rows in host memory
static int bpv_check(size_t bpv, int N)
{
	if (bpv >= (size_t)(N + 3) / 4) return SGX_OK;
	return fail(SGX_EINVAL, "Invalid length of dosages: bytes_per_variant=%zu < ceil(N/4)=%zu", bpv, (size_t)(N + 3) / 4);
}

// 2-bit rows in device memory, as the kernels read them
static int dev_rows_check(const char *who, const uint8_t *packed_dev, size_t bpv, int N)
{
	if (bpv % 64 != 0 || bpv < sgx_row_stride(N))
		return fail(SGX_EINVAL, "Invalid length of dosages: bytes_per_variant=%zu, need a multiple of 64 >= %zu", bpv, sgx_row_stride(N));
	if (((uintptr_t)packed_dev & 15u) != 0) return fail(SGX_EINVAL, "%s: packed_dev must be 16-byte aligned", who);
	return SGX_OK;
}

// a list of n row indices into a block of M rows
static int block_idx_check(const char *who, const int32_t *var_idx, size_t n, size_t M)
{
	for (size_t e = 0; e < n; e++)
		if (var_idx[e] < 0 || (size_t)var_idx[e] >= M)
			return fail(SGX_EINVAL, "%s: variant index %d outside the block's %zu rows", who, var_idx[e], M);
	return SGX_OK;
}
#endif
