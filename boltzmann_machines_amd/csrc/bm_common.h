// bm_common.h — error plumbing + the owners of device buffers, streams and events shared by the API files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <utility>
#include <map>
#include <vector>

namespace bm {

void set_error(const char *fmt, ...);

// Developer switches live in ONE environment variable: BM355_DEBUG="name=value,name=value" (DESIGN.md 9 lists the names:
// forced tile geometries, the launch tuner's log, chained-launch modes and measurement aids).  dbg("name") returns the value
// text or null.  None of them changes results; the variables a USER may set (BM355_HOST_WAIT, BM355_FAST_BINARY,
// BM355_AIS_LITERAL, BM355_DATA_PARALLEL, BM355_STAGED_SAVE, BM355_RCCL_LIB, BM_XCHG_TIMEOUT_S) keep names of their own.
static inline const char *dbg(const char *name) {
    static const std::map<std::string, std::string> *tab = [] {
        auto *m = new std::map<std::string, std::string>();
        const char *e = getenv("BM355_DEBUG");
        std::string cur;
        for (const char *c = e ? e : ""; ; ++c) {
            if (*c == ',' || *c == ';' || *c == ' ' || *c == 0) {
                if (!cur.empty()) {
                    const size_t q = cur.find('=');
                    (*m)[q == std::string::npos ? cur : cur.substr(0, q)] = q == std::string::npos ? std::string("1") : cur.substr(q + 1);
                }
                cur.clear();
                if (*c == 0) break;
            } else cur += *c;
        }
        return m;
    }();
    const auto it = tab->find(name);
    return it == tab->end() ? nullptr : it->second.c_str();
}

#define BM_HIP(expr)                                                                          \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            bm::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,    \
                          __LINE__);                                                          \
            return 1;                                                                         \
        }                                                                                     \
    } while (0)

#define BM_CHECK(cond, ...)                 \
    do {                                    \
        if (!(cond)) {                      \
            bm::set_error(__VA_ARGS__);     \
            return 2;                       \
        }                                   \
    } while (0)

#define BM_TRY(expr)              \
    do {                          \
        int _r = (expr);          \
        if (_r) return _r;        \
    } while (0)

// ---- owners of the engines' HIP resources.  Each is move-only and frees what it holds when it is destroyed or
// overwritten, so a handle frees itself member by member and an early return frees whatever was built so far.  A failed
// allocation or creation records the message (set_error), clears HIP's last error - a later, unrelated
// hipGetLastError() must not report it - and leaves the owner empty.
static inline int hip_failed(hipError_t e, const char *what, size_t bytes = 0) {
    (void)hipGetLastError();
    if (bytes) set_error("%s of %zu bytes failed: %s", what, bytes, hipGetErrorString(e));
    else set_error("%s failed: %s", what, hipGetErrorString(e));
    return 1;
}

// What the runtime allows one workgroup of `kernel` in DYNAMIC LDS - a query, no launch: out3 = {the device's
// hipDeviceAttributeMaxSharedMemoryPerBlock, the kernel's static LDS bytes, the dynamic bytes a launch may ask for = min(the
// kernel's maxDynamicSharedSizeBytes, per block - static)}.  The row-staging kernels (softmax_multinomial_kernel) size their
// width limit by it at create, so a handle that exists can launch.
static inline int dyn_lds_query(const void *kernel, long long out3[3]) {
    int dev = 0, per_block = 0;
    BM_HIP(hipGetDevice(&dev));
    BM_HIP(hipDeviceGetAttribute(&per_block, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    hipFuncAttributes fa;
    BM_HIP(hipFuncGetAttributes(&fa, kernel));
    const long long room = (long long)per_block - (long long)fa.sharedSizeBytes;
    out3[0] = per_block; out3[1] = (long long)fa.sharedSizeBytes;
    out3[2] = std::max(0ll, std::min(room, (long long)fa.maxDynamicSharedSizeBytes));
    return 0;
}

// a typed device array of n elements, zero-filled
template <class T> struct DevArray {
    T *p = nullptr;
    size_t n = 0;
    DevArray() = default;
    DevArray(DevArray &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevArray &operator=(DevArray o) noexcept { std::swap(p, o.p); std::swap(n, o.n); return *this; }
    ~DevArray() { if (p) (void)hipFree(p); }
    // n = count; max(count, room, 1) elements are allocated and zeroed.  Any earlier allocation is freed first.
    int alloc(size_t count, size_t room = 1) {
        *this = DevArray();
        DevArray a;
        const size_t bytes = std::max(count, room) * sizeof(T);
        hipError_t e = hipMalloc((void **)&a.p, bytes);
        if (e != hipSuccess) { a.p = nullptr; return hip_failed(e, "hipMalloc", bytes); }
        if ((e = hipMemset(a.p, 0, bytes)) != hipSuccess) return hip_failed(e, "hipMemset", bytes);
        a.n = count;
        *this = std::move(a);
        return 0;
    }
};

// float vector: the allocation is rounded up to whole 16-byte groups (vector kernels of bm_xchg may touch the round-up)
struct DevBuf : DevArray<float> {
    int alloc(size_t count) { return DevArray::alloc(count, count ? (count + 3) & ~(size_t)3 : 4); }
};

// a stream, an event or pinned host memory (the raw value converts implicitly, so call sites use it as before)
static inline void hip_destroy(hipStream_t s) { (void)hipStreamDestroy(s); }
static inline void hip_destroy(hipEvent_t e) { (void)hipEventDestroy(e); }
static inline void hip_destroy(void *host) { (void)hipHostFree(host); }
template <class H> struct Owned {
    H h = nullptr;
    Owned() = default;
    Owned(Owned &&o) noexcept : h(o.h) { o.h = nullptr; }
    Owned &operator=(Owned o) noexcept { std::swap(h, o.h); return *this; }
    ~Owned() { if (h) hip_destroy(h); }
    operator H() const { return h; }
};
using Stream = Owned<hipStream_t>;
using Event = Owned<hipEvent_t>;
template <class T> using Pinned = Owned<T *>;

static inline int create(Stream &s, unsigned flags = hipStreamDefault) {
    Stream t;
    const hipError_t e = hipStreamCreateWithFlags(&t.h, flags);
    if (e != hipSuccess) { t.h = nullptr; return hip_failed(e, "hipStreamCreateWithFlags"); }
    s = std::move(t);
    return 0;
}
static inline int create(Event &ev, unsigned flags = hipEventDefault) {
    Event t;
    const hipError_t e = hipEventCreateWithFlags(&t.h, flags);
    if (e != hipSuccess) { t.h = nullptr; return hip_failed(e, "hipEventCreateWithFlags"); }
    ev = std::move(t);
    return 0;
}
template <class T> static inline int create(Pinned<T> &m, size_t count) {
    Pinned<T> t;
    const hipError_t e = hipHostMalloc((void **)&t.h, count * sizeof(T), hipHostMallocDefault);
    if (e != hipSuccess) { t.h = nullptr; return hip_failed(e, "hipHostMalloc", count * sizeof(T)); }
    m = std::move(t);
    return 0;
}

// Leading dimension for matrices owned by the library.  A row pitch that is a
// multiple of 256 B (e.g. H = 1024 floats = 4 KiB) makes every row of a K-chunk
// hit the SAME L2/HBM channel (measured: 6x slower tiles); such pitches get +128 B.
static inline int pad_ld(int n) {
    int ld = (n + 3) & ~3;
    if (ld % 64 == 0) ld += 32;
    return ld;
}

// row-major [rows][cols] matrix in HBM with padded pitch `ld`
struct Mat : DevArray<float> {
    int rows = 0, cols = 0, ld = 0;
    size_t count() const { return (size_t)rows * ld; }
    int alloc(int r, int c) {
        rows = cols = ld = 0;
        BM_TRY(DevArray::alloc((size_t)r * pad_ld(c)));
        rows = r; cols = c; ld = pad_ld(c);
        return 0;
    }
    int upload(const float *host) {   // dense host [rows][cols] -> device
        BM_HIP(hipMemcpy2D(p, (size_t)ld * sizeof(float), host, (size_t)cols * sizeof(float),
                           (size_t)cols * sizeof(float), rows, hipMemcpyHostToDevice));
        return 0;
    }
    int download(float *host) const {
        BM_HIP(hipMemcpy2D(host, (size_t)cols * sizeof(float), p, (size_t)ld * sizeof(float),
                           (size_t)cols * sizeof(float), rows, hipMemcpyDeviceToHost));
        return 0;
    }
};

// the 16-column slots of a row of n columns: the epilogues leave one partial of a row sum per slot (ActArgs::rowdot_out)
static inline int nslots(int n) { return (n + 15) / 16; }

// bf16 matrix [planes][rows][ld] (bm_bf3.h): weight planes or the shadow of a {0,1} state matrix; ld % 64 == 0,
// zero initialised (the padding must stay zero: the bf16 contraction has no K tail handling)
struct Mat16 : DevArray<uint16_t> {
    int planes = 0, rows = 0, cols = 0, ld = 0;
    long long plane_stride() const { return (long long)rows * ld; }
    int alloc(int np, int r, int c) {
        planes = rows = cols = ld = 0;
        const int l = (c + 63) & ~63;
        BM_TRY(DevArray::alloc((size_t)np * r * l));
        planes = np; rows = r; cols = c; ld = l;
        return 0;
    }
};

}  // namespace bm
