// Sanitizer check of the `.pairs` reader's threads and buffers: a stand-alone program (never loaded into Python, host only).
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -o /tmp/pairs_asan \
//       scripts/pairs_sanitize_main.cpp mustache_amd/csrc/pairs_reader.cpp mustache_amd/csrc/hic_reader.cpp -lz
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=thread -o /tmp/pairs_tsan \
//       scripts/pairs_sanitize_main.cpp mustache_amd/csrc/pairs_reader.cpp mustache_amd/csrc/hic_reader.cpp -lz
//
// The files come from a separate Python step (the layouts of tests/test_pairs_reference.py: plain, .gz and two-member .gz
// copies; `good_*` must open, `bad_*` must fail with MST_IO_E_FORMAT and a message that names a line):
//
//   python -c "import sys; sys.path.insert(0, 'tests'); import test_pairs_reference as t; print('\n'.join(t.write_sanitizer_files('/tmp/pairs_files')))"
//   /tmp/pairs_asan /tmp/pairs_files/*.pairs /tmp/pairs_files/*.pairs.gz
//
// Every file is opened under both position conventions with 1, 3 and 8 threads and chunks of the default size, 4096, 97 and 7
// bytes (cuts inside lines, lines longer than a chunk, a header longer than a chunk); every accessor is called and every
// borrowed array is read to its end; all openings of one file must agree on every number.  Every `good_*` file is opened with
// keep_trans as well (mst_pairs_open_ex): a file with a `#chromsize` table must open, its trans arrays are walked to their end
// (seg_off, both position arrays, the per-pair out-of-range counts), the trans counters must add up with counters[2], and
// everything the plain opening yields must come out unchanged; a file without a table must be refused with MST_IO_E_FORMAT and a
// message that names `#chromsize`.  A handle opened the plain way must refuse the trans accessors.  Exit status 0 and no
// sanitizer report = clean.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/mustache_io_pairs.h"

static int failures = 0;

static void expect(bool ok, const char *what, const char *path) {
    if (!ok) {
        fprintf(stderr, "FAILED: %s: %s (%s)\n", path, what, mst_io_last_error());
        ++failures;
    }
}

// everything one opening yields, folded into a few numbers
struct Digest {
    std::vector<std::string> names;
    std::vector<int64_t> numbers;
    bool operator==(const Digest &o) const { return names == o.names && numbers == o.numbers; }
};

// the trans rows of a handle opened with keep_trans, read to their end; `trans` = counters[2] of the handle
static void walk_trans(const mst_pairs *h, int32_t nc, int64_t trans, const char *path, Digest *out) {
    int64_t P = -1, tc[3] = {0, 0, 0};
    const int64_t *seg = nullptr, *oor = nullptr;
    const int32_t *a = nullptr, *b = nullptr;
    expect(mst_pairs_trans_rows(h, &P, &seg, &a, &b, &oor) == MST_IO_OK && seg, "trans rows", path);
    expect(mst_pairs_trans_counters(h, tc) == MST_IO_OK, "trans counters", path);
    expect(P == (int64_t)nc * (nc - 1) / 2, "P = C (C - 1) / 2", path);
    if (P < 0 || !seg) return;
    expect(seg[0] == 0 && seg[P] == tc[0] && (tc[0] == 0 || (a && b)), "seg_off spans the stored rows", path);
    int64_t oor_sum = 0;
    for (int64_t p = 0; p < P; ++p) {
        expect(seg[p] <= seg[p + 1] && oor[p] >= 0 && oor[p] <= seg[p + 1] - seg[p], "a pair's segment", path);
        oor_sum += oor[p];
        uint64_t sum = 1469598103934665603ull;                    // order-sensitive: file order within the pair
        for (int64_t k = seg[p]; k < seg[p + 1]; ++k) sum = (sum ^ (uint32_t)a[k]) * 1099511628211ull, sum = (sum ^ (uint32_t)b[k]) * 1099511628211ull;
        out->numbers.push_back(seg[p + 1]);
        out->numbers.push_back(oor[p]);
        out->numbers.push_back((int64_t)sum);
    }
    expect(oor_sum == tc[1] && tc[0] + tc[2] == trans, "the trans counters add up", path);
    out->numbers.insert(out->numbers.end(), tc, tc + 3);
}

static bool digest(const char *path, int zero_based, int threads, int64_t chunk, int keep_trans, Digest *out, int *code, Digest *trans_out) {
    mst_pairs *h = nullptr;
    if (keep_trans) *code = mst_pairs_open_ex(path, zero_based, threads, chunk < 0 ? 0 : chunk, 1, &h);
    else *code = chunk < 0 ? mst_pairs_open(path, zero_based, threads, &h) : mst_pairs_open_chunked(path, zero_based, threads, chunk, &h);
    if (*code != MST_IO_OK) return false;
    int64_t counters[5];
    expect(mst_pairs_counters(h, counters) == MST_IO_OK, "counters", path);
    out->numbers.assign(counters, counters + 5);
    const int32_t nc = mst_pairs_n_chromosomes(h);
    int64_t stored = 0, oor_sum = 0;
    for (int32_t i = 0; i < nc; ++i) {
        const char *name = nullptr;
        int64_t length = 0, oor = 0;
        const int32_t *p1 = nullptr, *p2 = nullptr;
        expect(mst_pairs_chromosome(h, i, &name, &length) == MST_IO_OK && name, "chromosome", path);
        const int64_t n = mst_pairs_rows(h, i, &p1, &p2, &oor);
        expect(n >= 0 && (n == 0 || (p1 && p2)), "rows", path);
        uint64_t sum = 1469598103934665603ull;                    // order-sensitive: rows must keep file order
        for (int64_t k = 0; k < n; ++k) sum = (sum ^ (uint32_t)p1[k]) * 1099511628211ull, sum = (sum ^ (uint32_t)p2[k]) * 1099511628211ull;
        out->names.push_back(name ? name : "");
        out->numbers.push_back(length);
        out->numbers.push_back(n);
        out->numbers.push_back(oor);
        out->numbers.push_back((int64_t)sum);
        stored += n;
        oor_sum += oor;
    }
    expect(counters[0] == counters[1] + counters[2] + counters[3] + counters[4], "the counters add up", path);
    expect(counters[1] + counters[3] == stored && counters[3] == oor_sum, "the counters match the arrays", path);
    expect(mst_pairs_chromosome(h, nc, nullptr, nullptr) == MST_IO_E_ARG && mst_pairs_rows(h, -1, nullptr, nullptr, nullptr) == MST_IO_E_ARG,
           "an index outside the table is refused", path);
    if (keep_trans) {
        walk_trans(h, nc, counters[2], path, trans_out);
    } else {
        int64_t P = 0, tc[3];
        expect(mst_pairs_trans_rows(h, &P, nullptr, nullptr, nullptr, nullptr) == MST_IO_E_ARG && mst_pairs_trans_counters(h, tc) == MST_IO_E_ARG,
               "a plain handle refuses the trans accessors", path);
    }
    mst_pairs_close(h);
    return true;
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s FILE.pairs[.gz] ...   (good_* must open, bad_* must fail)\n", argv[0]);
        return 2;
    }
    const int threads[] = {1, 3, 8};
    const int64_t chunks[] = {-1, 4096, 97, 7};
    int opened = 0, refused = 0, with_trans = 0, no_table = 0;
    for (int a = 1; a < argc; ++a) {
        const char *path = argv[a];
        const char *base = strrchr(path, '/');
        const bool bad = strncmp(base ? base + 1 : path, "bad_", 4) == 0;
        for (int zero_based = 0; zero_based < 2; ++zero_based) {
            Digest first, first_trans;
            bool have_trans = false;
            std::string first_error;
            bool have = false;
            for (int t : threads)
                for (int64_t c : chunks) {
                    Digest d;
                    int code = 0;
                    const bool ok = digest(path, zero_based, t, c, 0, &d, &code, nullptr);
                    if (bad) {
                        const std::string msg = mst_io_last_error();
                        expect(!ok && code == MST_IO_E_FORMAT && msg.find("line ") != std::string::npos, "a malformed file names its line", path);
                        if (have) expect(msg == first_error, "the same line whatever the threads and chunks", path);
                        first_error = msg;
                        have = true;
                        ++refused;
                        continue;
                    }
                    expect(ok, "open", path);
                    if (!ok) continue;
                    ++opened;
                    if (have) expect(d == first, "every opening agrees", path);
                    else first = d, have = true;
                    // the same file with keep_trans: the plain digest unchanged, the trans arrays the same for every opening
                    Digest again, tr;
                    const bool table = !d.numbers.empty() && d.names.size() > 0 && d.numbers[6 - 1] >= 0;     // the first length
                    const bool ok2 = digest(path, zero_based, t, c, 1, &again, &code, &tr);
                    if (ok2) {
                        ++with_trans;
                        expect(table, "keep_trans opens only a file with a table", path);
                        expect(again == d, "keep_trans changes nothing the plain opening yields", path);
                        if (have_trans) expect(tr == first_trans, "every opening with keep_trans agrees", path);
                        else first_trans = tr, have_trans = true;
                    } else {
                        ++no_table;
                        const std::string msg = mst_io_last_error();
                        expect(!table && code == MST_IO_E_FORMAT && msg.find("#chromsize") != std::string::npos,
                               "only a file without a table is refused, by naming #chromsize", path);
                    }
                }
        }
    }
    mst_pairs *h = nullptr;
    expect(mst_pairs_open("/nonexistent/x.pairs", 0, 1, &h) == MST_IO_E_FILE && !h, "a missing file", "-");
    expect(mst_pairs_open("/nonexistent/x.pairs.gz", 0, 1, &h) == MST_IO_E_FILE && !h, "a missing .gz file", "-");
    expect(mst_pairs_open(nullptr, 0, 1, &h) == MST_IO_E_ARG, "a null path", "-");
    mst_pairs_close(nullptr);
    printf("%d openings agreed, %d with trans rows, %d without a table refused, %d refused as expected, %d failures\n", opened,
           with_trans, no_table, refused, failures);
    return failures ? 1 : 0;
}
