// ss_host.h — host staging shared by every entry that moves data around a launch: an owning, growable buffer, an event owner,
// the HIP check of the *_impl functions, image layout arithmetic, the carve-out and list-order read-back of a state's tables and the
// small thread pool of the batch copies.  Host code only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

// `who` is the entry's name with its ": " (a const char* or a std::string); needs `std::string& err` in scope
#define SS_HIPCHK(who, x)                                                                                           \
    do {                                                                                                            \
        hipError_t e_ = (x);                                                                                        \
        if (e_ != hipSuccess) { err = std::string(who) + #x ": " + hipGetErrorString(e_); return SS_ERR_HIP; }      \
    } while (0)

enum SsMem { SS_DEVICE, SS_PINNED, SS_PINNED_WC };      // SS_PINNED_WC: write-combined, for buffers the CPU only fills
enum SsSlack { SS_EXACT, SS_QUARTER };                  // what reserve() allocates: bytes, or bytes + bytes / 4

// Memory of one kind that is freed exactly once; the pointer and the capacity change together.
template <SsMem K>
class SsBuf {
    void* p_ = nullptr;
    size_t cap_ = 0;
    hipError_t drop()
    {
        const hipError_t e = K == SS_DEVICE ? hipFree(p_) : hipHostFree(p_);
        p_ = nullptr;
        cap_ = 0;
        return e;
    }
public:
    SsBuf() = default;
    SsBuf(const SsBuf&) = delete;
    SsBuf& operator=(const SsBuf&) = delete;
    ~SsBuf() { if (p_) (void)drop(); }                  // teardown: nothing useful can be done with an error here
    // no-op when the capacity suffices; otherwise the old memory goes first (the contents are not kept)
    hipError_t reserve(size_t bytes, SsSlack slack)
    {
        if (cap_ >= bytes) return hipSuccess;
        if (p_) { const hipError_t e = drop(); if (e != hipSuccess) return e; }
        const size_t want = slack == SS_QUARTER ? bytes + bytes / 4 : bytes;
        const hipError_t e = K == SS_DEVICE ? hipMalloc(&p_, want)
                                            : hipHostMalloc(&p_, want, K == SS_PINNED_WC ? hipHostMallocWriteCombined : hipHostMallocDefault);
        if (e != hipSuccess) { p_ = nullptr; return e; }
        cap_ = want;
        return hipSuccess;
    }
    template <class T = char> T* as() const { return (T*)p_; }
};

// An untimed event, created by the first ensure()
struct SsEvent {
    hipEvent_t ev = nullptr;
    SsEvent() = default;
    SsEvent(const SsEvent&) = delete;
    SsEvent& operator=(const SsEvent&) = delete;
    ~SsEvent() { if (ev) (void)hipEventDestroy(ev); }
    hipError_t ensure() { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, hipEventDisableTiming); }
    operator hipEvent_t() const { return ev; }
};

static inline size_t ss_align_up(size_t b, size_t a) { return (b + a - 1) & ~(a - 1); }      // a: a power of two

// Running offset of an image's fields: take() hands out the current offset and moves on to the next aligned one
struct SsLayout {
    size_t at = 0, align = 16;
    size_t take(size_t bytes) { const size_t o = at; at = ss_align_up(at + bytes, align); return o; }
};

// Where tables of bytes[0..n) start in one buffer that holds them in this order, each on a 256-byte boundary (what an allocation of
// its own gave it) -> off[0..n); returns the buffer's size
static inline size_t ss_carve_plan(const size_t* bytes, size_t n, size_t* off)
{
    SsLayout l{0, 256};
    for (size_t i = 0; i < n; ++i) off[i] = l.take(bytes[i]);
    return l.at;
}

// The tables of one lifetime group out of one owned device buffer: add() registers a table's pointer field and element count; carve()
// plans the offsets, reserves, zeroes the whole range on `st` and only then assigns the fields
struct SsCarve {
    std::vector<void*> field;                           // each the address of a T* of the state's argument struct
    std::vector<size_t> bytes;
    template <class T> void add(T** f, size_t n) { field.push_back((void*)f); bytes.push_back(n * sizeof(T)); }
    hipError_t carve(SsBuf<SS_DEVICE>& buf, hipStream_t st) const
    {
        std::vector<size_t> off(bytes.size());
        const size_t total = ss_carve_plan(bytes.data(), bytes.size(), off.data());
        hipError_t e = buf.reserve(total, SS_EXACT);
        if (e == hipSuccess) e = hipMemsetAsync(buf.as(), 0, total, st);
        for (size_t i = 0; e == hipSuccess && i < field.size(); ++i) { void* p = buf.as() + off[i]; memcpy(field[i], &p, sizeof p); }
        return e;
    }
};

// Rows of a [rows][width] table in list order: dst[i * width + k] = src[slots[i] * width + k] for i < n; a NULL dst asks for nothing.
// ss_gather_device is what the read-backs call: it fetches the table from the device first (the stream has been drained) and hands the
// host copy to ss_gather_rows, which is apart so that a host program can check it without a device (tests/tracker_state_host_main.cpp).
template <class T>
static inline void ss_gather_rows(const int* slots, int n, const T* src, int width, T* dst)
{
    for (int i = 0; dst && i < n; ++i)
        for (int k = 0; k < width; ++k) dst[(size_t)i * width + k] = src[(size_t)slots[i] * width + k];
}

template <class T>
static hipError_t ss_gather_device(const int* slots, int n, const T* d_src, size_t rows, int width, T* dst)
{
    if (!dst) return hipSuccess;
    std::vector<T> h(rows * width);
    const hipError_t e = hipMemcpy(h.data(), d_src, h.size() * sizeof(T), hipMemcpyDeviceToHost);
    if (e == hipSuccess) ss_gather_rows(slots, n, h.data(), width, dst);
    return e;
}

// work(t, T) for t = 0 .. T - 1, t = 0 on the calling thread.  Threads that cannot be started have their share done by the
// caller; false on any exception, since nothing thrown may cross the C boundary.
template <class Work>
static bool run_threads(int T, Work work)
{
    try {
        std::vector<std::thread> pool;
        pool.reserve(T > 1 ? T - 1 : 0);
        int started = 1;
        try {
            for (int t = 1; t < T; ++t) { pool.emplace_back(work, t, T); ++started; }
        } catch (...) {
            for (auto& th : pool) th.join();
            for (int t = started; t < T; ++t) work(t, T);
            pool.clear();
        }
        work(0, T);
        for (auto& th : pool) th.join();
    } catch (...) {
        return false;
    }
    return true;
}
