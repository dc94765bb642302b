// Shared helpers for libmustache_hip.so: host side (error reporting, launch checks), and the one device routine that several
// files need (segment_of).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <functional>
#include <memory>
#include <vector>
#include "../../include/mustache_hip.h"

namespace mst {

char *error_buffer();                       // thread-local, 512 bytes
int fail(int code, const char *fmt, ...);   // formats into error_buffer(), returns code

#define MST_HIP(call)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return ::mst::fail(MST_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),   \
                               __FILE__, __LINE__);                                                \
    } while (0)

#define MST_LAUNCH_CHECK() MST_HIP(hipGetLastError())

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// The segment that holds e: the largest p in [lo, hi) with off[p] <= e.  off is non-decreasing and off[lo] <= e is the caller's
// word; empty segments (equal offsets) are stepped over; the result stays in [lo, hi) whatever off holds, so a table indexed
// by it is never read out of bounds.
__device__ __forceinline__ int32_t segment_of(const int64_t *__restrict__ off, int32_t lo, int32_t hi, int64_t e) {
    while (hi - lo > 1) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE property of a kernel: raise it once per (call site, device),
// so a process that drives several GPUs gets it on each of them.  `done` = the call site's static bit mask of devices.
inline hipError_t allow_dynamic_lds(const void *kernel, int bytes, unsigned long long *done) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = 1ull << (dev & 63);
    if (__atomic_load_n(done, __ATOMIC_ACQUIRE) & bit) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) __atomic_fetch_or(done, bit, __ATOMIC_RELEASE);
    return e;
}

// Host -> device upload of a small table (level table, block starts, tile lists) whose source may be reused or freed as
// soon as the call returns (a stack object, a thread_local vector, a ctypes array the Python caller drops): the bytes are
// copied into a PINNED staging slot first and the asynchronous copy reads from there, so its correctness does not rest on
// the runtime staging pageable sources before hipMemcpyAsync returns.  A ring of slots per host thread; a slot is reused
// only after the event recorded behind its copy has completed (normally long ago).
hipError_t upload_small(void *dst, const void *src, size_t bytes, hipStream_t s);

// "Has everything that was enqueued to read or write this resource finished?"  record(s) puts an event behind the work just
// enqueued on s, wait() blocks the host until every recorded use is over, the destructor waits and destroys.  One event per
// STREAM that has used the resource (callers alternate two streams), created lazily without timing, recreated when the current
// device changes (events belong to a device).  Four slots -- a guess, not a measurement; a fifth stream takes a slot over
// after a HOST wait for that slot's own last use (normally long over, like the former wait for the copy before last).
class UseFence {
public:
    UseFence() = default;
    UseFence(const UseFence &) = delete;
    UseFence &operator=(const UseFence &) = delete;
    ~UseFence();
    hipError_t record(hipStream_t s);
    hipError_t wait();
private:
    struct Slot {
        hipStream_t stream = nullptr;
        hipEvent_t ev = nullptr;
        bool pending = false;
    };
    Slot slot_[4];
    int dev_ = -1;
    unsigned turn_ = 0;
};

// A host list that is uploaded again and again unchanged (the work list of a launch, kept in a per-thread cache of recent
// launches): ONE page-locked copy made when the list is built (assign), every launch copies straight out of it (upload: no host
// memcpy, no staging slot), and the memory is released with its owner -- after the last copy out of it has completed.
struct PinnedList {
    void *p = nullptr;
    size_t cap = 0, bytes = 0;
    UseFence copied;                                       // behind the copies out of it
    PinnedList() = default;
    PinnedList(const PinnedList &) = delete;
    PinnedList &operator=(const PinnedList &) = delete;
    ~PinnedList();
    hipError_t assign(const void *src, size_t n);          // waits for copies still reading the old contents
    hipError_t upload(void *dst, hipStream_t s);
};

// Graph replay (MST_FLAG_GRAPH), the "second sight" rule: a call whose signature is unknown takes the least recently used entry
// and runs the ordinary way (one-off calls never pay a capture); the second call with that signature is captured into a
// hipGraph, instantiated and launched; later ones are one hipGraphLaunch.  An entry's graph is destroyed only after its last
// launch has completed.  One cache per user and host thread (a thread_local object); never on the legacy default stream (it
// cannot be captured), never in PROFILE builds.  MUSTACHE_NO_GRAPHS switches users off by `word`.
class ReplayCache {
public:
    enum Sight { kFirst, kCapture, kReplay };
    ReplayCache(int entries, const char *word);            // word: "launch" or "finish"
    bool usable(int32_t flags, hipStream_t s) const { return enabled_ && (flags & MST_FLAG_GRAPH) && s != nullptr; }
    // finds the signature (every scalar / pointer argument, the device, tables as bytes) or claims an entry for it; the call
    // that follows -- nothing (kFirst), capture or replay -- acts on that entry
    Sight look(const std::vector<int64_t> &sig);
    static const char *name(Sight sight);                  // for mst::note: "first sight" / "CAPTURE" / "REPLAY"
    int replay(hipStream_t s);
    // body(image) enqueues the call on s between begin and end of the capture; image = image_bytes of page-locked memory the
    // entry owns (grow-only) for what the graph's copy nodes read, so nothing the graph references can change or go away
    // under it.  A stream that refuses capture gets body(nullptr), an ordinary launch; the entry stays at second sight, so
    // the next call tries again.  A failed body, capture or instantiation forgets the signature.
    int capture(const char *who, hipStream_t s, size_t image_bytes, const std::function<int(char *)> &body);
private:
    struct Entry {
        std::vector<int64_t> sig;
        hipGraphExec_t exec = nullptr;
        UseFence done;                                     // behind the launches of exec
        char *image = nullptr;
        size_t image_cap = 0;
        bool seen = false;
        unsigned long long stamp = 0;
        void drop_graph();
        ~Entry();
    };
    std::unique_ptr<Entry[]> entry_;
    Entry *cur_ = nullptr;
    int n_;
    unsigned long long stamp_ = 0;
    bool enabled_;
};

// PROFILE builds mark the stage every entry point belongs to (read / normalise / launch / finish / tail) as a roctx range, so
// that `rocprofv3 --marker-trace` shows the stages of a run next to its kernels (profiles/r06_marker_trace.md); the product
// library carries no marker and does not link the roctx library.
#ifdef MST_PROFILE
struct Range {
    explicit Range(const char *name);
    ~Range();
};
#define MST_RANGE(name_) mst::Range mst_range_scope_(name_)
#else
#define MST_RANGE(name_)
#endif

// diagnostics (MUSTACHE_GRAPH_DEBUG set): a short in-memory ring of notes about recent launches, printed when a call fails
void note(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void dump_notes();

}  // namespace mst
