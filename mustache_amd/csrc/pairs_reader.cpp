// libmustache_io.so -- 4DN `.pairs` / `.pairs.gz` files, see include/mustache_io_pairs.h (the rule: mustache_amd/pairs.py).
//
// One pass over the file.  A plain file is memory-mapped and cut into byte ranges at line ends; a `.gz` file is inflated by one
// producer thread (gzread: concatenated members, so bgzf too) that cuts its buffer at line ends.  Either way the chunks are
// parsed by a pool of threads into per-chunk, per-chromosome position vectors, which are then laid end to end in chunk order:
// rows keep file order within a chromosome whatever the thread count and the chunk size are.  With keep_trans the trans rows
// whose two chromosomes are in the table are kept as well: per chunk as (pair, position on a, position on b) triples, laid in
// pair-major order, chunk after chunk, by the same merge.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <atomic>
#include <climits>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/mustache_io_pairs.h"

namespace mst_io {
int fail(int code, const char *fmt, ...);      // hic_reader.cpp (shared thread-local error buffer)
}

namespace {

struct Table {
    std::vector<std::string> names;
    std::vector<int64_t> length;                // -1: no `#chromsize` line
    std::unordered_map<std::string, int> index;
    bool fixed = false;                         // true: the header named the chromosomes

    int add(const std::string &name, int64_t len) {
        auto it = index.find(name);
        if (it != index.end()) return it->second;
        const int id = (int)names.size();
        index.emplace(name, id);
        names.push_back(name);
        length.push_back(len);
        return id;
    }
};

struct Columns {
    int chr1 = 1, pos1 = 2, chr2 = 3, pos2 = 4;
    int last() const { return std::max(std::max(chr1, pos1), std::max(chr2, pos2)); }
};

inline bool is_blank(char c) { return c == ' ' || c == '\t'; }

// the fields of the line [p, q): up to `want` of them; returns how many were found
int split_fields(const char *p, const char *q, int want, const char **f0, const char **f1) {
    int nf = 0;
    while (nf < want) {
        while (p < q && is_blank(*p)) ++p;
        if (p == q) break;
        f0[nf] = p;
        while (p < q && !is_blank(*p)) ++p;
        f1[nf++] = p;
    }
    return nf;
}

// [+-]?[0-9]+ -> true and the value; a value outside int32 becomes INT32_MIN (out of range under either convention)
bool parse_position(const char *p, const char *e, int32_t *out) {
    bool neg = false;
    if (p < e && (*p == '-' || *p == '+')) neg = *p++ == '-';
    if (p == e) return false;
    int64_t v = 0;
    for (; p < e; ++p) {
        if (*p < '0' || *p > '9') return false;
        if (v < ((int64_t)1 << 40)) v = v * 10 + (*p - '0');
    }
    if (neg) v = -v;
    *out = (v < INT32_MIN || v > INT32_MAX) ? INT32_MIN : (int32_t)v;
    return true;
}

struct ChunkOut {
    Table local;                                 // the names of this chunk in order of first appearance (header-less files)
    std::vector<std::vector<int32_t>> p1, p2;    // per chromosome id (global when the table is fixed, local otherwise)
    std::vector<int64_t> out_of_range;
    std::vector<int64_t> tp;                     // keep_trans: the pair index of each stored trans row, file order
    std::vector<int32_t> ta, tb;                 // its position on the pair's first / second chromosome (table order)
    int64_t rows = 0, trans = 0, unknown = 0, trans_unknown = 0;
    bool bad = false;
    int64_t bad_line = 0;                        // 0-based, counted from the chunk's first line
    std::string what;
};

struct Job {
    const char *p = nullptr, *end = nullptr;
    std::string own;                             // the bytes, when they are not part of a mapping
    int64_t first_line = 0;                      // 1-based number of the chunk's first line
};

// the index of the pair (a, b), a < b, of a table of C chromosomes in pair-major order: (0,1), (0,2), ..., (1,2), ...
inline int64_t pair_index(int64_t a, int64_t b, int64_t C) { return a * (2 * C - a - 1) / 2 + (b - a - 1); }

inline bool out_of_range(int32_t pos, int64_t len, bool zero_based) {
    if (pos < (zero_based ? 0 : 1)) return true;
    return len >= 0 && (zero_based ? pos >= len : pos > len);
}

void parse_chunk(const char *p, const char *end, const Columns &col, const Table &table, bool zero_based, bool keep_trans,
                 ChunkOut &out) {
    const int64_t C = (int64_t)table.names.size();
    const int want = col.last() + 1;
    std::vector<const char *> f0(want), f1(want);
    if (table.fixed) {
        out.p1.resize(table.names.size());
        out.p2.resize(table.names.size());
        out.out_of_range.assign(table.names.size(), 0);
    }
    const int32_t lo = zero_based ? 0 : 1;
    const char *last_name = nullptr;             // the previous row's chromosome: sorted files repeat it for millions of rows
    size_t last_len = 0;
    int last_id = -1;
    auto lookup = [&](const char *a, const char *b) {
        const size_t n = (size_t)(b - a);
        if (last_name && n == last_len && memcmp(a, last_name, n) == 0) return last_id;
        int id;
        if (table.fixed) {
            auto it = table.index.find(std::string(a, b));
            id = it == table.index.end() ? -1 : it->second;
        } else {
            id = out.local.add(std::string(a, b), -1);
            if ((size_t)id >= out.p1.size()) {
                out.p1.resize(id + 1);
                out.p2.resize(id + 1);
                out.out_of_range.resize(id + 1, 0);
            }
        }
        last_name = a;
        last_len = n;
        last_id = id;
        return id;
    };
    int64_t line = 0;
    for (; p < end; ++line) {
        const char *eol = (const char *)memchr(p, '\n', (size_t)(end - p));
        const char *q = eol ? eol : end;
        const char *next = eol ? eol + 1 : end;
        if (q > p && q[-1] == '\r') --q;
        const char *s = p;
        p = next;
        if (s < q && *s == '#') continue;
        const int nf = split_fields(s, q, want, f0.data(), f1.data());
        if (nf == 0) continue;                   // a blank line
        if (nf < want) {
            out.bad = true;
            out.bad_line = line;
            out.what = "too few fields (" + std::to_string(nf) + ", " + std::to_string(want) + " needed)";
            return;
        }
        int32_t a, b;
        if (!parse_position(f0[col.pos1], f1[col.pos1], &a) || !parse_position(f0[col.pos2], f1[col.pos2], &b)) {
            out.bad = true;
            out.bad_line = line;
            out.what = "a position that is not a decimal integer";
            return;
        }
        ++out.rows;
        const size_t n1 = (size_t)(f1[col.chr1] - f0[col.chr1]), n2 = (size_t)(f1[col.chr2] - f0[col.chr2]);
        const bool cis = n1 == n2 && memcmp(f0[col.chr1], f0[col.chr2], n1) == 0;
        if (!cis) {
            ++out.trans;
            if (!table.fixed) {                  // both names still take their place in the order of first appearance
                lookup(f0[col.chr1], f1[col.chr1]);
                lookup(f0[col.chr2], f1[col.chr2]);
            } else if (keep_trans) {             // oriented by the table: the lower index is the pair's first chromosome
                const int i1 = lookup(f0[col.chr1], f1[col.chr1]), i2 = lookup(f0[col.chr2], f1[col.chr2]);
                if (i1 < 0 || i2 < 0 || i1 == i2) {          // (two spellings of one table entry cannot happen: exact compare)
                    ++out.trans_unknown;
                } else {
                    out.tp.push_back(i1 < i2 ? pair_index(i1, i2, C) : pair_index(i2, i1, C));
                    out.ta.push_back(i1 < i2 ? a : b);
                    out.tb.push_back(i1 < i2 ? b : a);
                }
            }
            continue;
        }
        const int id = lookup(f0[col.chr1], f1[col.chr1]);
        if (id < 0) {
            ++out.unknown;
            continue;
        }
        out.p1[id].push_back(a);
        out.p2[id].push_back(b);
        const int64_t len = table.fixed ? table.length[id] : -1;
        bool oor = a < lo || b < lo;
        if (!oor && len >= 0) oor = zero_based ? (a >= len || b >= len) : (a > len || b > len);
        out.out_of_range[id] += oor;
    }
}

// one header line [s, q) (it starts with '#'); false and *why when it is malformed
bool header_line(const char *s, const char *q, Table &table, Columns &col, std::string *why) {
    const char *f0[64], *f1[64];
    const int nf = split_fields(s, q, 64, f0, f1);
    auto is = [&](int k, const char *w) { return (size_t)(f1[k] - f0[k]) == strlen(w) && memcmp(f0[k], w, strlen(w)) == 0; };
    if (nf >= 1 && is(0, "#chromsize:")) {
        int32_t len;
        if (nf < 3 || !parse_position(f0[2], f1[2], &len) || len < 0) {
            *why = "a #chromsize: line without a name and a length";
            return false;
        }
        table.fixed = true;
        table.add(std::string(f0[1], f1[1]), len);
    } else if (nf >= 1 && is(0, "#columns:")) {
        int *slot[4] = {&col.chr1, &col.pos1, &col.chr2, &col.pos2};
        const char *name[4] = {"chr1", "pos1", "chr2", "pos2"};
        for (int c = 0; c < 4; ++c) {
            *slot[c] = -1;
            for (int k = 1; k < nf && *slot[c] < 0; ++k)
                if (is(k, name[c])) *slot[c] = k - 1;
            if (*slot[c] < 0) {
                *why = std::string("a #columns: line without ") + name[c];
                return false;
            }
        }
    }
    return true;
}

// The leading header block of [p, end): '#' lines and blank lines.  Returns the first byte behind it, or nullptr when the
// block may go on behind `end` (no complete non-header line was seen; `at_eof`: then it ends at `end`).  *lines: lines consumed.
const char *read_header(const char *p, const char *end, bool at_eof, Table &table, Columns &col, int64_t *lines, std::string *why,
                        bool *bad) {
    while (p < end) {
        const char *eol = (const char *)memchr(p, '\n', (size_t)(end - p));
        if (!eol && !at_eof) return nullptr;
        const char *q = eol ? eol : end;
        if (q > p && q[-1] == '\r') --q;
        const char *s = p;
        while (s < q && is_blank(*s)) ++s;
        if (s < q && *p != '#') return p;
        if (s < q && !header_line(p, q, table, col, why)) {
            *bad = true;
            return p;
        }
        ++*lines;
        p = eol ? eol + 1 : end;
    }
    return at_eof ? end : nullptr;
}

}  // namespace

struct mst_pairs {
    Table table;
    std::vector<int32_t *> p1, p2;
    std::vector<int64_t> rows, out_of_range;
    int64_t counters[5] = {0, 0, 0, 0, 0};
    bool keep_trans = false;
    bool zero_based = false;
    std::vector<int64_t> seg_off, trans_oor;     // keep_trans: [P + 1] and [P], P = C (C - 1) / 2
    int32_t *ta = nullptr, *tb = nullptr;        // the stored trans rows, pair-major
    int64_t trans_counters[3] = {0, 0, 0};       // stored; of those out of range; naming a chromosome the table lacks
    ~mst_pairs() {
        for (int32_t *p : p1) free(p);
        for (int32_t *p : p2) free(p);
        free(ta);
        free(tb);
    }
};

namespace {

// keep_trans: a counting sort of the chunks' trans rows by pair, chunk after chunk -- file order within a pair
bool merge_trans(std::deque<ChunkOut> &parts, mst_pairs &h) {
    const int64_t C = (int64_t)h.table.names.size(), P = C * (C - 1) / 2;
    h.seg_off.assign((size_t)P + 1, 0);
    h.trans_oor.assign((size_t)P, 0);
    for (const ChunkOut &part : parts) {
        h.trans_counters[2] += part.trans_unknown;
        for (int64_t p : part.tp) ++h.seg_off[(size_t)p + 1];
    }
    for (int64_t p = 0; p < P; ++p) h.seg_off[(size_t)p + 1] += h.seg_off[(size_t)p];
    const int64_t total = h.seg_off[(size_t)P];
    h.trans_counters[0] = total;
    if (total) {
        h.ta = (int32_t *)malloc((size_t)total * sizeof(int32_t));
        h.tb = (int32_t *)malloc((size_t)total * sizeof(int32_t));
        if (!h.ta || !h.tb) return false;
    }
    std::vector<int32_t> first((size_t)P), second((size_t)P);     // pair -> its two chromosomes
    for (int64_t a = 0, p = 0; a < C; ++a)
        for (int64_t b = a + 1; b < C; ++b, ++p) {
            first[(size_t)p] = (int32_t)a;
            second[(size_t)p] = (int32_t)b;
        }
    std::vector<int64_t> fill(h.seg_off.begin(), h.seg_off.end() - 1);
    for (ChunkOut &part : parts) {
        for (size_t k = 0; k < part.tp.size(); ++k) {
            const size_t p = (size_t)part.tp[k];
            const int32_t a = part.ta[k], b = part.tb[k];
            h.ta[fill[p]] = a;
            h.tb[fill[p]++] = b;
            h.trans_oor[p] += out_of_range(a, h.table.length[(size_t)first[p]], h.zero_based) ||
                              out_of_range(b, h.table.length[(size_t)second[p]], h.zero_based);
        }
        std::vector<int64_t>().swap(part.tp);
        std::vector<int32_t>().swap(part.ta);
        std::vector<int32_t>().swap(part.tb);
    }
    for (int64_t v : h.trans_oor) h.trans_counters[1] += v;
    return true;
}

// lay the chunks' vectors end to end, in chunk order
bool merge(std::deque<ChunkOut> &parts, mst_pairs &h) {
    Table &table = h.table;
    std::vector<std::vector<int>> map(parts.size());           // chunk's id -> global id
    for (size_t c = 0; c < parts.size(); ++c) {
        const size_t ids = parts[c].p1.size();
        map[c].resize(ids);
        for (size_t k = 0; k < ids; ++k) map[c][k] = table.fixed ? (int)k : table.add(parts[c].local.names[k], -1);
    }
    const size_t nc = table.names.size();
    h.rows.assign(nc, 0);
    h.out_of_range.assign(nc, 0);
    h.p1.assign(nc, nullptr);
    h.p2.assign(nc, nullptr);
    for (size_t c = 0; c < parts.size(); ++c) {
        h.counters[0] += parts[c].rows;
        h.counters[2] += parts[c].trans;
        h.counters[4] += parts[c].unknown;
        for (size_t k = 0; k < parts[c].p1.size(); ++k) {
            h.rows[map[c][k]] += (int64_t)parts[c].p1[k].size();
            h.out_of_range[map[c][k]] += parts[c].out_of_range[k];
        }
    }
    std::vector<int64_t> fill(nc, 0);
    for (size_t g = 0; g < nc; ++g) {
        h.counters[3] += h.out_of_range[g];
        h.counters[1] += h.rows[g] - h.out_of_range[g];
        if (!h.rows[g]) continue;
        h.p1[g] = (int32_t *)malloc((size_t)h.rows[g] * sizeof(int32_t));
        h.p2[g] = (int32_t *)malloc((size_t)h.rows[g] * sizeof(int32_t));
        if (!h.p1[g] || !h.p2[g]) return false;
    }
    for (size_t c = 0; c < parts.size(); ++c) {
        for (size_t k = 0; k < parts[c].p1.size(); ++k) {
            const size_t n = parts[c].p1[k].size();
            if (!n) continue;
            const int g = map[c][k];
            memcpy(h.p1[g] + fill[g], parts[c].p1[k].data(), n * sizeof(int32_t));
            memcpy(h.p2[g] + fill[g], parts[c].p2[k].data(), n * sizeof(int32_t));
            fill[g] += (int64_t)n;
        }
        std::vector<std::vector<int32_t>>().swap(parts[c].p1);
        std::vector<std::vector<int32_t>>().swap(parts[c].p2);
    }
    return !h.keep_trans || merge_trans(parts, h);
}

int64_t count_lines(const char *p, const char *end) {
    int64_t n = 0;
    while (p < end) {
        const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p));
        if (!nl) break;
        ++n;
        p = nl + 1;
    }
    return n;
}

int report_bad(const char *path, std::deque<ChunkOut> &parts, const std::vector<int64_t> &first_line) {
    for (size_t c = 0; c < parts.size(); ++c)
        if (parts[c].bad)
            return mst_io::fail(MST_IO_E_FORMAT, "%s: line %lld: %s", path, (long long)(first_line[c] + parts[c].bad_line),
                                parts[c].what.c_str());
    return MST_IO_OK;
}

int no_table(const char *path) {
    return mst_io::fail(MST_IO_E_FORMAT, "%s has no #chromsize lines: trans rows are kept by the table's chromosome pairs, and the "
                                         "genome layout needs the lengths", path);
}

int open_plain(const char *path, bool zero_based, int nt, size_t chunk_bytes, mst_pairs &h) {
    const int fd = open(path, O_RDONLY);
    struct stat st;
    if (fd < 0 || fstat(fd, &st) != 0) {
        if (fd >= 0) close(fd);
        return mst_io::fail(MST_IO_E_FILE, "cannot open %s", path);
    }
    const size_t size = (size_t)st.st_size;
    if (!size) {
        close(fd);
        return MST_IO_OK;
    }
    void *m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) return mst_io::fail(MST_IO_E_FILE, "cannot map %s", path);
    const char *base = (const char *)m, *end = base + size;
    int rc = MST_IO_OK;
    {
        Columns col;
        int64_t header_lines = 0;
        std::string why;
        bool bad = false;
        const char *data = read_header(base, end, true, h.table, col, &header_lines, &why, &bad);
        if (bad) {
            rc = mst_io::fail(MST_IO_E_FORMAT, "%s: line %lld: %s", path, (long long)(header_lines + 1), why.c_str());
        } else if (h.keep_trans && !h.table.fixed) {
            rc = no_table(path);
        } else {
            const size_t left = (size_t)(end - data);
            size_t nchunks = left / chunk_bytes + 1;
            if (nchunks > 65536) nchunks = 65536;
            std::vector<const char *> cut(nchunks + 1);
            cut[0] = data;
            cut[nchunks] = end;
            for (size_t i = 1; i < nchunks; ++i) {              // advance each cut to the next line start
                const char *c = data + left / nchunks * i;
                if (c < cut[i - 1]) c = cut[i - 1];
                const char *nl = c < end ? (const char *)memchr(c, '\n', (size_t)(end - c)) : nullptr;
                cut[i] = nl ? nl + 1 : end;
            }
            std::deque<ChunkOut> parts(nchunks);
            std::atomic<size_t> next(0);
            std::atomic<int> stop(0);
            auto work = [&]() {
                for (;;) {
                    const size_t i = next.fetch_add(1);
                    if (i >= nchunks || stop.load()) return;
                    try {
                        parse_chunk(cut[i], cut[i + 1], col, h.table, zero_based, h.keep_trans, parts[i]);
                        if (parts[i].bad) stop.store(1);
                    } catch (...) {
                        stop.store(2);
                    }
                }
            };
            if ((size_t)nt > nchunks) nt = (int)nchunks;
            std::vector<std::thread> pool;
            for (int t = 1; t < nt; ++t) pool.emplace_back(work);
            work();
            for (auto &t : pool) t.join();
            if (stop.load() == 2) {
                rc = mst_io::fail(MST_IO_E_FILE, "out of memory while parsing %s", path);
            } else if (stop.load() == 1) {
                std::vector<int64_t> first_line(nchunks, 0);
                for (size_t c = 0; c < nchunks; ++c)
                    if (parts[c].bad) {
                        first_line[c] = 1 + count_lines(base, cut[c]);
                        break;
                    }
                rc = report_bad(path, parts, first_line);
            } else if (!merge(parts, h)) {
                rc = mst_io::fail(MST_IO_E_FILE, "out of memory for the rows of %s", path);
            }
        }
    }
    munmap(m, size);
    return rc;
}

int open_gz(const char *path, bool zero_based, int nt, size_t chunk_bytes, mst_pairs &h) {
    gzFile gz = gzopen(path, "rb");
    if (!gz) return mst_io::fail(MST_IO_E_FILE, "cannot open %s", path);
    gzbuffer(gz, 1 << 20);
    Columns col;
    std::deque<ChunkOut> parts;                  // grown by the producer; a deque keeps its elements in place
    std::vector<int64_t> first_line;
    std::deque<std::pair<size_t, std::shared_ptr<Job>>> queue;
    std::mutex mu;
    std::condition_variable can_take, can_put;
    bool done = false;
    std::atomic<int> stop(0);
    const size_t max_queued = 2 * (size_t)nt + 2;

    auto work = [&]() {
        for (;;) {
            std::pair<size_t, std::shared_ptr<Job>> item;
            ChunkOut *out;
            {
                std::unique_lock<std::mutex> lk(mu);
                can_take.wait(lk, [&] { return done || !queue.empty(); });
                if (queue.empty()) return;
                item = std::move(queue.front());
                queue.pop_front();
                out = &parts[item.first];
                can_put.notify_one();
            }
            if (stop.load()) continue;           // drain: the producer may be waiting for room
            try {
                parse_chunk(item.second->p, item.second->end, col, h.table, zero_based, h.keep_trans, *out);
                if (out->bad) stop.store(1);
            } catch (...) {
                stop.store(2);
            }
        }
    };
    auto put = [&](std::string &&bytes, int64_t line) {
        auto job = std::make_shared<Job>();
        job->own = std::move(bytes);
        job->p = job->own.data();
        job->end = job->p + job->own.size();
        job->first_line = line;
        std::unique_lock<std::mutex> lk(mu);
        can_put.wait(lk, [&] { return queue.size() < max_queued; });
        parts.emplace_back();
        first_line.push_back(line);
        queue.emplace_back(parts.size() - 1, std::move(job));
        can_take.notify_one();
    };

    std::vector<std::thread> pool;
    int rc = MST_IO_OK;
    bool in_header = true, at_eof = false;
    int64_t line = 1;                            // number of the first line of `buf`
    std::string buf;
    try {
        while (!at_eof && !stop.load()) {
            const size_t old = buf.size();
            buf.resize(old + chunk_bytes);
            size_t got = 0;
            while (got < chunk_bytes) {          // gzread may return short at a member boundary
                const int r = gzread(gz, &buf[old + got], (unsigned)std::min<size_t>(chunk_bytes - got, (size_t)1 << 30));
                if (r < 0) {
                    int err = 0;
                    const char *msg = gzerror(gz, &err);
                    rc = mst_io::fail(MST_IO_E_ZLIB, "%s: %s", path, msg ? msg : "inflate failed");
                    break;
                }
                if (r == 0) {
                    at_eof = true;
                    break;
                }
                got += (size_t)r;
            }
            if (rc != MST_IO_OK) break;
            buf.resize(old + got);
            size_t start = 0;
            if (in_header) {
                int64_t lines = 0;
                std::string why;
                bool bad = false;
                const char *data = read_header(buf.data(), buf.data() + buf.size(), at_eof, h.table, col, &lines, &why, &bad);
                if (bad) {
                    rc = mst_io::fail(MST_IO_E_FORMAT, "%s: line %lld: %s", path, (long long)(line + lines), why.c_str());
                    break;
                }
                if (!data) {                     // the block may go on behind the buffer: read more and parse it again
                    h.table = Table();
                    col = Columns();
                    continue;
                }
                if (h.keep_trans && !h.table.fixed) {
                    rc = no_table(path);
                    break;
                }
                line += lines;
                start = (size_t)(data - buf.data());
                in_header = false;
                for (int t = 0; t < nt; ++t) pool.emplace_back(work);   // the table and the columns are final from here on
            }
            size_t cut = buf.size();
            if (!at_eof) {
                while (cut > start && buf[cut - 1] != '\n') --cut;
                if (cut == start) {              // no line end yet: one line longer than a chunk
                    if (start) buf.erase(0, start);
                    continue;
                }
            }
            if (cut > start) {
                std::string bytes(buf, start, cut - start);
                const int64_t n_lines = count_lines(bytes.data(), bytes.data() + bytes.size());
                put(std::move(bytes), line);
                line += n_lines;
            }
            buf.erase(0, cut);
        }
    } catch (...) {
        rc = mst_io::fail(MST_IO_E_FILE, "out of memory while reading %s", path);
    }
    {
        std::unique_lock<std::mutex> lk(mu);
        done = true;
        can_take.notify_all();
    }
    for (auto &t : pool) t.join();
    gzclose(gz);
    if (rc != MST_IO_OK) return rc;
    if (stop.load() == 2) return mst_io::fail(MST_IO_E_FILE, "out of memory while parsing %s", path);
    if (stop.load() == 1) return report_bad(path, parts, first_line);
    if (!merge(parts, h)) return mst_io::fail(MST_IO_E_FILE, "out of memory for the rows of %s", path);
    return MST_IO_OK;
}

bool ends_with(const char *s, const char *tail) {
    const size_t n = strlen(s), m = strlen(tail);
    return n >= m && memcmp(s + n - m, tail, m) == 0;
}

}  // namespace

extern "C" int mst_pairs_open_ex(const char *path, int32_t zero_based, int32_t n_threads, int64_t chunk_bytes, int32_t keep_trans,
                                 mst_pairs **out) {
    if (!path || !out) return mst_io::fail(MST_IO_E_ARG, "mst_pairs_open: bad argument");
    *out = nullptr;
    int nt = n_threads > 0 ? n_threads : (int)std::thread::hardware_concurrency();
    if (nt < 1) nt = 1;
    if (nt > 256) nt = 256;
    const size_t chunk = chunk_bytes > 0 ? (size_t)chunk_bytes : (size_t)4 << 20;
    try {
        std::unique_ptr<mst_pairs> h(new mst_pairs());
        h->keep_trans = keep_trans != 0;
        h->zero_based = zero_based != 0;
        const int rc = ends_with(path, ".gz") ? open_gz(path, zero_based != 0, nt, chunk, *h) : open_plain(path, zero_based != 0, nt, chunk, *h);
        if (rc != MST_IO_OK) return rc;
        if (h->rows.size() < h->table.names.size()) {           // an empty file body: no chunk was merged
            const size_t nc = h->table.names.size();
            h->rows.resize(nc, 0);
            h->out_of_range.resize(nc, 0);
            h->p1.resize(nc, nullptr);
            h->p2.resize(nc, nullptr);
        }
        if (h->keep_trans) {
            if (!h->table.fixed) return no_table(path);         // an empty file
            const size_t C = h->table.names.size(), P = C * (C - 1) / 2;
            if (h->seg_off.size() != P + 1) {                   // an empty file body
                h->seg_off.assign(P + 1, 0);
                h->trans_oor.assign(P, 0);
            }
        }
        *out = h.release();
        return MST_IO_OK;
    } catch (...) {
        return mst_io::fail(MST_IO_E_FILE, "out of memory while reading %s", path);
    }
}

extern "C" int mst_pairs_open_chunked(const char *path, int32_t zero_based, int32_t n_threads, int64_t chunk_bytes, mst_pairs **out) {
    return mst_pairs_open_ex(path, zero_based, n_threads, chunk_bytes, 0, out);
}

extern "C" int mst_pairs_open(const char *path, int32_t zero_based, int32_t n_threads, mst_pairs **out) {
    return mst_pairs_open_chunked(path, zero_based, n_threads, 0, out);
}

extern "C" void mst_pairs_close(mst_pairs *h) { delete h; }

extern "C" int32_t mst_pairs_n_chromosomes(const mst_pairs *h) { return h ? (int32_t)h->table.names.size() : 0; }

extern "C" int mst_pairs_chromosome(const mst_pairs *h, int32_t index, const char **name, int64_t *length_bp) {
    if (!h || index < 0 || (size_t)index >= h->table.names.size())
        return mst_io::fail(MST_IO_E_ARG, "mst_pairs_chromosome: bad argument");
    if (name) *name = h->table.names[index].c_str();
    if (length_bp) *length_bp = h->table.length[index];
    return MST_IO_OK;
}

extern "C" int64_t mst_pairs_rows(const mst_pairs *h, int32_t index, const int32_t **pos1, const int32_t **pos2,
                                  int64_t *out_of_range) {
    if (!h || index < 0 || (size_t)index >= h->table.names.size()) return mst_io::fail(MST_IO_E_ARG, "mst_pairs_rows: bad argument");
    if (pos1) *pos1 = h->p1[index];
    if (pos2) *pos2 = h->p2[index];
    if (out_of_range) *out_of_range = h->out_of_range[index];
    return h->rows[index];
}

extern "C" int mst_pairs_counters(const mst_pairs *h, int64_t counters[5]) {
    if (!h || !counters) return mst_io::fail(MST_IO_E_ARG, "mst_pairs_counters: bad argument");
    memcpy(counters, h->counters, sizeof(h->counters));
    return MST_IO_OK;
}

extern "C" int mst_pairs_trans_rows(const mst_pairs *h, int64_t *n_pairs, const int64_t **seg_off, const int32_t **posA,
                                    const int32_t **posB, const int64_t **out_of_range) {
    if (!h || !h->keep_trans) return mst_io::fail(MST_IO_E_ARG, "mst_pairs_trans_rows: the handle was opened without keep_trans");
    if (n_pairs) *n_pairs = (int64_t)h->trans_oor.size();
    if (seg_off) *seg_off = h->seg_off.data();
    if (posA) *posA = h->ta;
    if (posB) *posB = h->tb;
    if (out_of_range) *out_of_range = h->trans_oor.data();
    return MST_IO_OK;
}

extern "C" int mst_pairs_trans_counters(const mst_pairs *h, int64_t counters[3]) {
    if (!h || !counters || !h->keep_trans)
        return mst_io::fail(MST_IO_E_ARG, "mst_pairs_trans_counters: the handle was opened without keep_trans");
    memcpy(counters, h->trans_counters, sizeof(h->trans_counters));
    return MST_IO_OK;
}
