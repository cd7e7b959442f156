// host_mem.h -- the owners of everything the host state holds on the device: DevBuf, PinBuf, DevEvent, DevStream.
// Part of libsaigehip.so: included by saigehip.hip (one translation unit), not a header of its own.
//
// Every device or pinned allocation, event and stream of the library lives in one of these four types, as a member of
// the struct (or a local of the call) that uses it: the destructor is the only release, so no way out of a function
// skips it and no free list has to be kept.  The only allocation calls outside this file are sgx_host_alloc /
// sgx_host_free, which hand pinned memory to the caller (not counted below).
//
// Two rules the types do not enforce:
//  * a buffer that grows frees what it held, and none of these types waits for anything: the CALLER sees to it that
//    nothing queued still reads the old buffer (ensure_buf, ensure_recs, ... synchronise the lane first);
//  * the sgx_*_free functions wait for what is in flight, then `delete` -- members go in reverse order of declaration,
//    so a struct declares its streams first, then its events, then its buffers.
//
// Error codes.  reserve / alloc / create report the hipError_t.  grow() and HIPCHK turn it into SGX_EHIP, as for every
// other HIP call.  Where the CALLER sizes what is kept (sgx_block_create, sgx_dsblock_create; dev_room for the entries
// on an explicit GRM) running out of memory is SGX_ENOMEM: those collect the hipError_t (HIPPASS), give mem_code() of it
// and keep their own messages.

static std::atomic<size_t> g_live_bytes{0};

// bytes held by every DevBuf and PinBuf of the process (device and pinned together)
extern "C" size_t sgx_live_bytes(void) { return g_live_bytes.load(std::memory_order_relaxed); }

// in a function that returns hipError_t: pass a failure on
#define HIPPASS(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)

static int mem_code(hipError_t e) { return e == hipErrorOutOfMemory ? SGX_ENOMEM : SGX_EHIP; }

// cap elements of device (PINNED: pinned host) memory
template <class T, bool PINNED>
struct MemBuf {
	T *p = nullptr;
	size_t cap = 0;
	MemBuf() = default;
	MemBuf(const MemBuf &) = delete;
	MemBuf &operator=(const MemBuf &) = delete;
	MemBuf(MemBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
	MemBuf &operator=(MemBuf &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
	~MemBuf() { (void)release(); }
	operator T *() const { return p; }
	hipError_t release()
	{
		if (!p) return hipSuccess;
		g_live_bytes -= cap * sizeof(T);
		T *q = p;
		p = nullptr; cap = 0;
		if constexpr (PINNED) return hipHostFree(q); else return hipFree(q);
	}
	// exactly n elements, fresh (what it held is freed first)
	hipError_t alloc(size_t n)
	{
		hipError_t e = release();
		if (e != hipSuccess || n == 0) return e;
		if constexpr (PINNED) e = hipHostMalloc((void **)&p, n * sizeof(T), hipHostMallocDefault);
		else e = hipMalloc((void **)&p, n * sizeof(T));
		if (e != hipSuccess) { p = nullptr; return e; }
		cap = n;
		g_live_bytes += n * sizeof(T);
		return hipSuccess;
	}
	// room for n elements: grows, never shrinks; what it held is not kept
	hipError_t reserve(size_t n) { return n <= cap ? hipSuccess : alloc(n); }
};
template <class T> using DevBuf = MemBuf<T, false>;
template <class T> using PinBuf = MemBuf<T, true>;

// Room for n elements, three ways: a new entry takes dev_room for what its caller sizes (rows, units, sets: SGX_ENOMEM
// with a text that says what for), grow for the rest (reserve() as the library's return code), and ensure_buf
// (host_scan.h) instead of either for a lane's buffer that a call still in flight may read.
template <class B>
static int grow(B &b, size_t n)
{
	HIPCHK(b.reserve(n));
	return SGX_OK;
}

// reserve() with out of memory as SGX_ENOMEM: `what` the room is for, `who` asks
template <class T>
static int dev_room(DevBuf<T> &b, size_t n, const char *what, const char *who)
{
	const hipError_t e = b.reserve(n);
	if (e == hipSuccess) return SGX_OK;
	(void)hipGetLastError();
	return fail(mem_code(e), "%s: %zu bytes for %s: %s", who, n * sizeof(T), what, hipGetErrorString(e));
}

struct DevEvent {
	hipEvent_t e = nullptr;
	DevEvent() = default;
	DevEvent(const DevEvent &) = delete;
	DevEvent &operator=(const DevEvent &) = delete;
	~DevEvent() { if (e) (void)hipEventDestroy(e); }
	operator hipEvent_t() const { return e; }
	hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(&e, flags); }
};

struct DevStream {
	hipStream_t s = nullptr;
	DevStream() = default;
	DevStream(const DevStream &) = delete;
	DevStream &operator=(const DevStream &) = delete;
	~DevStream() { if (s) (void)hipStreamDestroy(s); }
	operator hipStream_t() const { return s; }
	hipError_t create(unsigned flags) { return hipStreamCreateWithFlags(&s, flags); }
	hipError_t create(unsigned flags, int priority) { return hipStreamCreateWithPriority(&s, flags, priority); }
};
