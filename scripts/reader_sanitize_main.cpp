// Sanitizer check of the native readers' threads and buffers: a stand-alone program (never loaded into Python, host only).
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=thread -o /tmp/reader_tsan scripts/reader_sanitize_main.cpp \
//       mustache_amd/csrc/hic_reader.cpp mustache_amd/csrc/text_reader.cpp -lz
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -o /tmp/reader_asan \
//       scripts/reader_sanitize_main.cpp mustache_amd/csrc/hic_reader.cpp mustache_amd/csrc/text_reader.cpp -lz
//
// The two files come from a separate Python step (the fixture of tests/test_hic_reader.py: chr1's intra matrix, the pair
// chr1 / chr2, and a copy with one undecodable block in each matrix):
//
//   python -c "import sys; sys.path.insert(0, 'tests'); import test_hic_reader as t; t.write_queue_files('/tmp')"
//   /tmp/reader_tsan /tmp/good.hic /tmp/bad.hic && /tmp/reader_asan /tmp/good.hic /tmp/bad.hic
//
// It performs both one-shot reads, drains each of the three streams with slabs released late and out of order, closes each
// stream early with a slab still in the consumer's hands, and reads the corrupted file through every path (MST_IO_E_ZLIB
// expected).  Exit status 0 and no sanitizer report = clean.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/mustache_io.h"
#include "../include/mustache_io_trans.h"

// 8 slabs: 4 with the workers, at most 3 held back by the consumer, one spare -- so next() can always wait without a time limit.
// (A timed wait goes through pthread_cond_clockwait, which older ThreadSanitizer runtimes do not model: they then report a
// "double lock" and races between accesses that hold the same mutex.  The timed answers of next() are held by pytest.)
static const int32_t kRes = 1000, kDist = 12, kSlabs = 8, kThreads = 4, kHeld = 3;
static const int64_t kCap = 64, kRawBytes = 4096;
static int failures = 0;

static void expect(bool ok, const char *what) {
    if (!ok) {
        fprintf(stderr, "FAILED: %s (%s)\n", what, mst_io_last_error());
        ++failures;
    }
}

struct Memory {
    std::vector<uint8_t> bytes;
    void *ptr;
    explicit Memory(size_t n) : bytes(n + 16), ptr(bytes.data() + (16 - reinterpret_cast<uintptr_t>(bytes.data()) % 16) % 16) {}
};

// kind 0: packed stream, 1: raw stream, 2: trans raw stream.  Returns the open code; *st / *rs is set on success.
static int open_stream(int kind, mst_hic *h, Memory &m, int32_t n_slabs, mst_hic_stream **st, mst_hic_rawstream **rs) {
    int32_t transposed = 0;
    if (kind == 0) return mst_hic_stream_open(h, "chr1", kRes, "KR", kDist, 0, kThreads, 0, 1, m.ptr, n_slabs, kCap, 2, st);
    if (kind == 1) return mst_hic_rawstream_open(h, "chr1", kRes, "KR", kDist, kThreads, 0, 1, m.ptr, n_slabs, kRawBytes, rs);
    return mst_hic_rawstream_open_trans(h, "chr1", "chr2", kRes, "KR", kThreads, m.ptr, n_slabs, kRawBytes, &transposed, rs);
}

static int next(int kind, mst_hic_stream *st, mst_hic_rawstream *rs, int32_t timeout, int32_t *slab) {
    int64_t n = 0;
    int32_t rows = 0;
    return kind == 0 ? mst_hic_stream_next(st, timeout, slab, &n) : mst_hic_rawstream_next(rs, timeout, slab, &n, &rows);
}

static int release(int kind, mst_hic_stream *st, mst_hic_rawstream *rs, int32_t slab) {
    return kind == 0 ? mst_hic_stream_release(st, slab) : mst_hic_rawstream_release(rs, slab);
}

static int close(int kind, mst_hic_stream *st, mst_hic_rawstream *rs, int64_t *total) {
    int64_t a = 0;
    int32_t bt = 0, bm = 0;
    return kind == 0 ? mst_hic_stream_close(st, &a, total, &bt, &bm) : mst_hic_rawstream_close(rs, total, &a, &bt, &bm);
}

// drain with up to kHeld slabs held back and given back in a scrambled order; returns the code that ended the drain
static int drain(int kind, mst_hic_stream *st, mst_hic_rawstream *rs, int *delivered) {
    std::vector<int32_t> held;
    uint32_t lcg = 12345;
    for (;;) {
        int32_t slab = -1;
        const int rc = next(kind, st, rs, -1, &slab);
        if (rc <= 0) return rc;
        held.push_back(slab);
        ++*delivered;
        while (held.size() > (size_t)kHeld) {
            lcg = lcg * 1664525u + 1013904223u;
            const size_t k = (lcg >> 16) % held.size();
            expect(release(kind, st, rs, held[k]) == MST_IO_OK, "release");
            held.erase(held.begin() + (long)k);
        }
    }
}

static void one_shot(mst_hic *h, bool corrupted) {
    int64_t *x = nullptr, *y = nullptr, n_bins = 0;
    double *v = nullptr;
    const int64_t n = mst_hic_read_intra(h, "chr1", kRes, "KR", kDist, kThreads, &x, &y, &v);
    expect(corrupted ? n == MST_IO_E_ZLIB : n > 1000, "mst_hic_read_intra");
    mst_io_free(x);
    mst_io_free(y);
    mst_io_free(v);
    int32_t *px = nullptr, *pd = nullptr;
    float *pv = nullptr;
    const int64_t np = mst_hic_read_intra_packed(h, "chr1", kRes, "KR", kDist, 0, kThreads, &px, &pd, &pv, &n_bins);
    expect(corrupted ? np == MST_IO_E_ZLIB : np == n, "mst_hic_read_intra_packed");
    mst_io_free(px);
    mst_io_free(pd);
    mst_io_free(pv);
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s good.hic corrupted.hic\n", argv[0]);
        return 2;
    }
    for (int file = 0; file < 2; ++file) {
        const bool corrupted = file == 1;
        mst_hic *h = nullptr;
        if (mst_hic_open(argv[1 + file], &h) != MST_IO_OK) {
            fprintf(stderr, "%s\n", mst_io_last_error());
            return 2;
        }
        one_shot(h, corrupted);
        for (int kind = 0; kind < 3; ++kind) {
            Memory m((size_t)kSlabs * (size_t)(kind == 0 ? kCap * 10 : kRawBytes));
            mst_hic_stream *st = nullptr;
            mst_hic_rawstream *rs = nullptr;
            int64_t total = 0;
            int delivered = 0;
            expect(open_stream(kind, h, m, kSlabs, &st, &rs) == MST_IO_OK, "open");
            const int end = drain(kind, st, rs, &delivered);
            const int rc = close(kind, st, rs, &total);
            if (corrupted) expect(end == MST_IO_E_ZLIB && rc == MST_IO_E_ZLIB, "a corrupted block is reported by next and close");
            else expect(end == 0 && rc == MST_IO_OK && delivered > 4 && total > 0, "full drain");
            if (corrupted) continue;
            // early close: two slabs, one taken and never given back
            int32_t slab = -1;
            st = nullptr;
            rs = nullptr;
            expect(open_stream(kind, h, m, 2, &st, &rs) == MST_IO_OK, "open with two slabs");
            expect(next(kind, st, rs, -1, &slab) == 1, "first slab");
            expect(close(kind, st, rs, &total) == MST_IO_OK, "early close");
        }
        mst_hic_close(h);
    }
    if (failures) return 1;
    printf("reader_sanitize_main: all paths ran as expected\n");
    return 0;
}
