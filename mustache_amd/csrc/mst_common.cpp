#include "mst_common.h"
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <string>

namespace mst {

char *error_buffer() {
    static thread_local char buf[512] = {0};
    return buf;
}

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(error_buffer(), 512, fmt, ap);
    va_end(ap);
    return code;
}

UseFence::~UseFence() {
    (void)wait();
    for (Slot &q : slot_)
        if (q.ev) (void)hipEventDestroy(q.ev);
}

hipError_t UseFence::wait() {
    hipError_t e = hipSuccess;
    for (Slot &q : slot_) {
        if (q.pending) {
            const hipError_t r = hipEventSynchronize(q.ev);
            if (r != hipSuccess) e = r;
        }
        q.pending = false;
    }
    return e;
}

hipError_t UseFence::record(hipStream_t s) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev_ != dev) {                                     // events belong to a device
        (void)wait();
        for (Slot &q : slot_) {
            if (q.ev) (void)hipEventDestroy(q.ev);
            q = Slot();
        }
        dev_ = dev;
    }
    Slot *q = nullptr;
    for (Slot &c : slot_)
        if (!q && c.ev && c.stream == s) q = &c;
    for (Slot &c : slot_)
        if (!q && !c.ev) q = &c;
    if (!q) {                                              // more streams than slots: take one over once its own use is over
        q = &slot_[turn_++ % 4];
        if (q->pending && (e = hipEventSynchronize(q->ev)) != hipSuccess) return e;
        q->pending = false;
    }
    if (!q->ev && (e = hipEventCreateWithFlags(&q->ev, hipEventDisableTiming)) != hipSuccess) return e;
    q->stream = s;
    if ((e = hipEventRecord(q->ev, s)) != hipSuccess) return e;
    q->pending = true;
    return hipSuccess;
}

namespace {
struct StageSlot {
    void *p = nullptr;
    size_t cap = 0;
    UseFence copied;                                       // behind the copy out of the slot
    ~StageSlot() {
        (void)copied.wait();
        if (p) (void)hipHostFree(p);
    }
};
// Two rings per host thread: 16 slots for the small tables (level table, block origins: at most kSmallBytes each, so the ring
// never holds more than 1 MB of page-locked memory) and 4 slots for the occasional larger list (a difference-kernel tile list
// of a whole-genome launch: grow-only to the largest seen).  The slots are released when the thread ends -- the main thread's
// thread_local objects are destroyed at the start of exit(), before the HIP runtime's own teardown.
constexpr int kSmallSlots = 16, kLargeSlots = 4;
constexpr size_t kSmallBytes = 64 * 1024;
template <int N>
struct StageRing {
    StageSlot slot[N];
    int next = 0;
};

// page-locked memory for at least `bytes`, in multiples of `granule`; the old contents are not kept
hipError_t grow_pinned(void **p, size_t *cap, size_t bytes, size_t granule) {
    if (*cap >= bytes) return hipSuccess;
    if (*p) (void)hipHostFree(*p);
    *p = nullptr;
    *cap = 0;
    const size_t want = (bytes + granule - 1) / granule * granule;
    const hipError_t e = hipHostMalloc(p, want, hipHostMallocDefault);
    if (e == hipSuccess) *cap = want;
    return e;
}

hipError_t stage(StageSlot &q, size_t granule, void *dst, const void *src, size_t bytes, hipStream_t s) {
    hipError_t e = q.copied.wait();
    if (e == hipSuccess) e = grow_pinned(&q.p, &q.cap, bytes, granule);
    if (e != hipSuccess) return e;
    memcpy(q.p, src, bytes);
    e = hipMemcpyAsync(dst, q.p, bytes, hipMemcpyHostToDevice, s);
    return e != hipSuccess ? e : q.copied.record(s);
}
}  // namespace

hipError_t upload_small(void *dst, const void *src, size_t bytes, hipStream_t s) {
    if (bytes == 0) return hipSuccess;
    if (bytes <= kSmallBytes) {
        static thread_local StageRing<kSmallSlots> ring;
        StageSlot &q = ring.slot[ring.next];
        ring.next = (ring.next + 1) % kSmallSlots;
        return stage(q, kSmallBytes, dst, src, bytes, s);
    }
    static thread_local StageRing<kLargeSlots> big;
    StageSlot &q = big.slot[big.next];
    big.next = (big.next + 1) % kLargeSlots;
    return stage(q, 1 << 20, dst, src, bytes, s);
}

PinnedList::~PinnedList() {
    (void)copied.wait();
    if (p) (void)hipHostFree(p);
}

hipError_t PinnedList::assign(const void *src, size_t n) {
    hipError_t e = copied.wait();                          // copies out of the old contents may still be in flight
    if (e == hipSuccess) e = grow_pinned(&p, &cap, n, 65536);
    if (e != hipSuccess) return e;
    if (n) memcpy(p, src, n);
    bytes = n;
    return hipSuccess;
}

hipError_t PinnedList::upload(void *dst, hipStream_t s) {
    if (bytes == 0) return hipSuccess;
    const hipError_t e = hipMemcpyAsync(dst, p, bytes, hipMemcpyHostToDevice, s);
    return e != hipSuccess ? e : copied.record(s);
}

ReplayCache::ReplayCache(int entries, const char *word) : entry_(new Entry[entries]), n_(entries) {
#ifdef MST_PROFILE
    enabled_ = false;
#else
    // diagnostic switch, read once per process: unset / empty / 0 = all on, "launch" / "finish" = none for that user, 1 (or
    // any other word) = no graphs at all
    static const std::string off = [] {
        const char *e = getenv("MUSTACHE_NO_GRAPHS");
        return std::string(e ? e : "");
    }();
    enabled_ = off.empty() || off == "0" || ((off == "launch" || off == "finish") && off != word);
#endif
}

void ReplayCache::Entry::drop_graph() {
    if (!exec) return;
    (void)done.wait();
    (void)hipGraphExecDestroy(exec);
    exec = nullptr;
}

ReplayCache::Entry::~Entry() {
    drop_graph();
    if (image) (void)hipHostFree(image);
}

const char *ReplayCache::name(Sight sight) { return sight == kReplay ? "REPLAY" : sight == kCapture ? "CAPTURE" : "first sight"; }

ReplayCache::Sight ReplayCache::look(const std::vector<int64_t> &sig) {
    cur_ = nullptr;
    for (int i = 0; i < n_; ++i)
        if (entry_[i].seen && entry_[i].sig == sig) cur_ = &entry_[i];
    const bool known = cur_ != nullptr;
    if (!known) {
        cur_ = &entry_[0];
        for (int i = 1; i < n_; ++i)
            if (entry_[i].stamp < cur_->stamp) cur_ = &entry_[i];
        cur_->drop_graph();
        cur_->sig = sig;
        cur_->seen = true;
    }
    cur_->stamp = ++stamp_;
    return !known ? kFirst : cur_->exec ? kReplay : kCapture;
}

int ReplayCache::replay(hipStream_t s) {
    MST_HIP(hipGraphLaunch(cur_->exec, s));
    MST_HIP(cur_->done.record(s));
    return MST_OK;
}

int ReplayCache::capture(const char *who, hipStream_t s, size_t image_bytes, const std::function<int(char *)> &body) {
    Entry &g = *cur_;
    MST_HIP(grow_pinned((void **)&g.image, &g.image_cap, image_bytes, 256));
    if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        return body(nullptr);
    }
    const int rc = body(g.image);
    hipGraph_t graph = nullptr;
    const hipError_t ee = hipStreamEndCapture(s, &graph);            // always: the stream must leave capture mode
    const bool captured = rc == MST_OK && ee == hipSuccess && graph;
    const hipError_t ie = captured ? hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0) : hipSuccess;
    if (graph) (void)hipGraphDestroy(graph);
    if (captured && ie == hipSuccess) return replay(s);
    g.exec = nullptr;
    g.seen = false;
    if (rc != MST_OK) return rc;
    if (captured) return fail(MST_E_HIP, "%s: graph instantiation failed: %s", who, hipGetErrorString(ie));
    return fail(MST_E_HIP, "%s: graph capture failed: %s", who, hipGetErrorString(ee));
}

namespace {
char g_notes[64][240];
unsigned g_note_at = 0;
}  // namespace

void note(const char *fmt, ...) {
    static const char *mode = getenv("MUSTACHE_GRAPH_DEBUG");
    if (!mode) return;
    char *line = g_notes[g_note_at++ % 64];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(line, sizeof(g_notes[0]), fmt, ap);
    va_end(ap);
    if (mode[0] == 'p') fprintf(stderr, "[note] %s\n", line);          // "print": every note at once (changes the timing)
}

void dump_notes() {
    const unsigned n = g_note_at < 64 ? g_note_at : 64;
    for (unsigned i = g_note_at - n; i != g_note_at; ++i) fprintf(stderr, "[note %u] %s\n", i, g_notes[i % 64]);
}

}  // namespace mst

extern "C" int mst_abi_version(void) { return MST_ABI_VERSION; }
extern "C" int mst_abi_revision(void) { return MST_ABI_REVISION; }
extern "C" const char *mst_last_error(void) { return mst::error_buffer(); }

#ifdef MST_PROFILE
#include <rocprofiler-sdk-roctx/roctx.h>
namespace mst {
Range::Range(const char *name) { (void)roctxRangePushA(name); }
Range::~Range() { (void)roctxRangePop(); }
}  // namespace mst
#endif
