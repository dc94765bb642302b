// libmustache_io.so -- native reader for Juicer `.hic` files (host only: g++ + zlib), see include/mustache_io.h.
//
// Replaces the hic-straw calls of reference mustache/mustache.py:300-396.  The file layout is restated from the
// published format as implemented by straw (github.com/aidenlab/straw, straw.cpp); all integers little-endian:
//   header  : "HIC\0", int32 version, int64 masterIndexPosition, genomeId\0, [v9: int64 nviPosition, int64 nviLength],
//             int32 nAttributes {key\0 value\0}, int32 nChrs {name\0, v9 int64 / v8 int32 length},
//             int32 nBpResolutions {int32}, int32 nFragResolutions {int32}
//   footer  : (at masterIndexPosition) v9 int64 / v8 int32 nBytes, int32 nEntries {key\0 "c1_c2", int64 position,
//             int32 size}; expected-value vectors; normalised expected-value vectors; then the normalisation-vector
//             index: int32 nEntries {type\0, int32 chrIdx, unit\0, int32 binSize, int64 position, v9 int64 / v8 int32 size}
//             (v9 files also give its position directly as nviPosition)
//   matrix  : int32 c1, int32 c2, int32 nResolutions, per resolution: unit\0, int32 zoomIndex, 4 x float32 statistics,
//             int32 binSize, int32 blockBinCount, int32 blockColumnCount, int32 nBlocks {int32 number, int64 position,
//             int32 size}
//   block   : zlib stream; int32 nRecords, int32 binXOffset, int32 binYOffset, byte useShort(0 = yes),
//             [v9: byte useShortBinX(0 = yes), byte useShortBinY(0 = yes)], byte type;
//             type 1 = list of rows {y, count {x, value}}, type 2 = dense w-wide grid with sentinels
//             (v6: plain {int32 x, int32 y, float32 value} records)
//   norm    : v9 int64 / v8 int32 nValues, then v9 float32 / v8 float64 values
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mustache_io.h"
#include "../../include/mustache_io_trans.h"
#include "mst_inflate.h"

namespace {

thread_local char g_err[512] = "";

int vfail(int code, const char *fmt, va_list ap) {
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    return code;
}

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfail(code, fmt, ap);
    va_end(ap);
    return code;
}

struct FormatError {
    const char *what;
};
}  // namespace

namespace mst_io {
int fail(int code, const char *fmt, ...) {          // the error buffer is shared with text_reader.cpp
    va_list ap;
    va_start(ap, fmt);
    vfail(code, fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace mst_io

namespace {

// bounds-checked little-endian cursor over a byte range
struct Cursor {
    const uint8_t *p, *end;
    Cursor(const uint8_t *b, size_t n) : p(b), end(b + n) {}
    void need(size_t n) const {
        if ((size_t)(end - p) < n) throw FormatError{"truncated structure"};
    }
    template <class T>
    T get() {
        need(sizeof(T));
        T v;
        memcpy(&v, p, sizeof(T));
        p += sizeof(T);
        return v;
    }
    std::string str() {
        const void *z = memchr(p, 0, (size_t)(end - p));
        if (!z) throw FormatError{"unterminated string"};
        std::string s((const char *)p, (const char *)z);
        p = (const uint8_t *)z + 1;
        return s;
    }
    void skip(uint64_t n) {
        if ((uint64_t)(end - p) < n) throw FormatError{"truncated structure"};
        p += n;
    }
};

struct Chrom {
    std::string name;
    int64_t length;
};
struct BlockRef {
    int32_t number;
    int64_t pos;
    int32_t size;
};
struct NormRef {
    int64_t pos, size;
};

}  // namespace

struct mst_hic {
    int fd = -1;
    const uint8_t *map = nullptr;
    size_t size = 0;
    int32_t version = 0;
    int64_t master = 0, nvi_pos = 0, nvi_len = 0;
    std::string genome;
    std::vector<Chrom> chroms;
    std::vector<int32_t> bp_res;
    std::map<std::string, std::pair<int64_t, int32_t>> matrices;     // "c1_c2" -> (position, size)
    size_t after_master = 0;                                          // file offset right behind the master index entries
    bool norm_index_read = false;
    std::map<std::string, NormRef> norm_index;                        // "TYPE|chrIdx|UNIT|binSize"
    // records of the last mst_hic_decode_intra_packed call: one grow-only arena per worker thread (capacity survives
    // from call to call, so a whole-genome run stops paying for fresh pages after its largest chromosome), and per
    // block which arena holds its records and where
    struct PackedArena {
        std::vector<int32_t> x, d;
        std::vector<float> v;
    };
    struct PackedSpan {
        int arena;
        size_t begin, count;
    };
    std::vector<PackedArena> arenas;
    std::vector<std::vector<uint8_t>> inflate_bufs;                   // per worker thread, grow-only like the arenas
    std::vector<PackedSpan> spans;
    int64_t packed_total = -1;

    Cursor at(int64_t pos) const {
        if (pos < 0 || (uint64_t)pos > size) throw FormatError{"file position outside the file"};
        return Cursor(map + pos, size - (size_t)pos);
    }
};

namespace {

void parse_header(mst_hic *h) {
    Cursor c = h->at(0);
    if (c.str() != "HIC") throw FormatError{"missing HIC magic"};
    h->version = c.get<int32_t>();
    if (h->version < 6 || h->version > 9) throw FormatError{"unsupported .hic version (6-9 are handled)"};
    h->master = c.get<int64_t>();
    h->genome = c.str();
    if (h->version > 8) {
        h->nvi_pos = c.get<int64_t>();
        h->nvi_len = c.get<int64_t>();
    }
    const int32_t n_attr = c.get<int32_t>();
    if (n_attr < 0) throw FormatError{"negative attribute count"};
    for (int32_t i = 0; i < n_attr; ++i) {
        c.str();
        c.str();
    }
    const int32_t n_chr = c.get<int32_t>();
    if (n_chr < 0 || n_chr > 1000000) throw FormatError{"implausible chromosome count"};
    for (int32_t i = 0; i < n_chr; ++i) {
        Chrom ch;
        ch.name = c.str();
        ch.length = h->version > 8 ? c.get<int64_t>() : (int64_t)c.get<int32_t>();
        h->chroms.push_back(ch);
    }
    const int32_t n_res = c.get<int32_t>();
    if (n_res < 0 || n_res > 10000) throw FormatError{"implausible resolution count"};
    for (int32_t i = 0; i < n_res; ++i) h->bp_res.push_back(c.get<int32_t>());
    // fragment resolutions and restriction sites follow; nothing on this path needs them
}

void parse_master_index(mst_hic *h) {
    Cursor c = h->at(h->master);
    if (h->version > 8) c.get<int64_t>(); else c.get<int32_t>();          // nBytes
    const int32_t n = c.get<int32_t>();
    if (n < 0) throw FormatError{"negative master index size"};
    for (int32_t i = 0; i < n; ++i) {
        std::string key = c.str();
        const int64_t pos = c.get<int64_t>();
        const int32_t size = c.get<int32_t>();
        h->matrices[key] = std::make_pair(pos, size);
    }
    h->after_master = (size_t)(c.p - h->map);
}

void skip_expected(mst_hic *h, Cursor &c, bool normalised) {
    const int32_t n = c.get<int32_t>();
    if (n < 0) throw FormatError{"negative expected-value count"};
    for (int32_t i = 0; i < n; ++i) {
        if (normalised) c.str();                                           // normalisation type
        c.str();                                                           // unit
        c.get<int32_t>();                                                  // bin size
        const int64_t nv = h->version > 8 ? c.get<int64_t>() : (int64_t)c.get<int32_t>();
        if (nv < 0) throw FormatError{"negative expected-value length"};
        c.skip((uint64_t)nv * (h->version > 8 ? 4u : 8u));
        const int32_t nf = c.get<int32_t>();
        if (nf < 0) throw FormatError{"negative normalisation-factor count"};
        c.skip((uint64_t)nf * (4u + (h->version > 8 ? 4u : 8u)));
    }
}

std::string norm_key(const std::string &type, int32_t chr_idx, const std::string &unit, int32_t bin) {
    return type + "|" + std::to_string(chr_idx) + "|" + unit + "|" + std::to_string(bin);
}

void read_norm_index(mst_hic *h) {
    if (h->norm_index_read) return;
    Cursor c = h->at(0);
    if (h->version > 8 && h->nvi_pos > 0) {
        c = h->at(h->nvi_pos);
    } else {
        c = h->at((int64_t)h->after_master);
        skip_expected(h, c, false);
        skip_expected(h, c, true);
    }
    const int32_t n = c.get<int32_t>();
    if (n < 0) throw FormatError{"negative normalisation-vector count"};
    for (int32_t i = 0; i < n; ++i) {
        std::string type = c.str();
        const int32_t chr_idx = c.get<int32_t>();
        std::string unit = c.str();
        const int32_t bin = c.get<int32_t>();
        NormRef r;
        r.pos = c.get<int64_t>();
        r.size = h->version > 8 ? c.get<int64_t>() : (int64_t)c.get<int32_t>();
        h->norm_index[norm_key(type, chr_idx, unit, bin)] = r;
    }
    h->norm_index_read = true;
}

std::vector<double> read_norm_vector(mst_hic *h, const NormRef &r) {
    Cursor c = h->at(r.pos);
    const int64_t n = h->version > 8 ? c.get<int64_t>() : (int64_t)c.get<int32_t>();
    if (n < 0 || n > (int64_t)1 << 40) throw FormatError{"implausible normalisation-vector length"};
    std::vector<double> v((size_t)n);
    if (h->version > 8) {
        for (int64_t i = 0; i < n; ++i) v[(size_t)i] = (double)c.get<float>();
    } else {
        for (int64_t i = 0; i < n; ++i) v[(size_t)i] = c.get<double>();
    }
    return v;
}

struct ZoomData {
    int32_t bin_size = 0, block_bin_count = 0, block_column_count = 0;
    std::vector<BlockRef> blocks;
    bool found = false;
};

ZoomData read_zoom(mst_hic *h, int64_t matrix_pos, int32_t resolution) {
    Cursor c = h->at(matrix_pos);
    c.get<int32_t>();                                                     // c1
    c.get<int32_t>();                                                     // c2
    const int32_t n_res = c.get<int32_t>();
    if (n_res < 0 || n_res > 10000) throw FormatError{"implausible zoom count"};
    ZoomData z;
    for (int32_t i = 0; i < n_res; ++i) {
        const std::string unit = c.str();
        c.get<int32_t>();                                                 // zoom index
        c.skip(16);                                                       // sumCounts, occupiedCellCount, stdDev, percent95
        const int32_t bin = c.get<int32_t>();
        const int32_t bbc = c.get<int32_t>();
        const int32_t bcc = c.get<int32_t>();
        const int32_t nb = c.get<int32_t>();
        if (nb < 0) throw FormatError{"negative block count"};
        if (unit == "BP" && bin == resolution) {
            z.bin_size = bin;
            z.block_bin_count = bbc;
            z.block_column_count = bcc;
            z.blocks.resize((size_t)nb);
            for (int32_t b = 0; b < nb; ++b) {
                z.blocks[(size_t)b].number = c.get<int32_t>();
                z.blocks[(size_t)b].pos = c.get<int64_t>();
                z.blocks[(size_t)b].size = c.get<int32_t>();
            }
            z.found = true;
            return z;
        }
        c.skip((uint64_t)nb * 16u);
    }
    return z;
}

// Can block `number` hold a record with |binX - binY| <= max_dist?  Errs on the side of reading the block.
bool block_near_diagonal(int32_t version, int32_t number, int32_t bbc, int32_t bcc, int64_t max_dist) {
    if (max_dist < 0 || bbc <= 0 || bcc <= 0) return true;
    if (version > 8) {
        // v9 intra-chromosomal blocks are indexed (depth, position along the diagonal):
        //   depth = int(log2(1 + |binX - binY| / sqrt(2) / blockBinCount)),  number = depth * blockColumnCount + pad
        const int64_t depth = number / bcc;
        const int64_t far = (int64_t)std::log2(1.0 + (double)max_dist / std::sqrt(2.0) / (double)bbc) + 1;
        return depth <= far;
    }
    const int64_t r = number / bcc, col = number % bcc;                    // number = row * blockColumnCount + column
    const int64_t d = r > col ? r - col : col - r;
    // bins of block row r / column col differ by at least (d - 1) * blockBinCount + 1 when d >= 1 -- exact, so the blocks just
    // beyond the distance limit (a few per cent of a 1 kb chromosome's compressed bytes) are not inflated for nothing
    return d == 0 || (d - 1) * (int64_t)bbc + 1 <= max_dist;
}

// The record filter of every decoder (mustache.py:370-388), whatever the sink: a sink has push(binX, binY, value) and reserve(n).
template <class Sink>
inline void emit(Sink &out, int64_t bx, int64_t by, float counts, const std::vector<double> *norm, int64_t max_dist) {
    if (bx > by) {                                                         // intra blocks store binX <= binY; be lenient
        const int64_t t = bx;
        bx = by;
        by = t;
    }
    if (max_dist >= 0 && by - bx > max_dist) return;
    float c = counts;
    if (norm) {
        if (bx < 0 || (size_t)by >= norm->size()) return;                  // straw would index out of range; drop
        c = (float)((double)counts / ((*norm)[(size_t)bx] * (*norm)[(size_t)by]));
    }
    if (std::isnan(c) || !(c > 0.0f)) return;                              // mustache.py:370-373, :385-388
    out.push(bx, by, c);
}

struct Records {
    std::vector<int64_t> x, y;
    std::vector<double> v;
    void push(int64_t bx, int64_t by, float c) {
        x.push_back(bx);
        y.push_back(by);
        v.push_back((double)c);
    }
    void reserve(size_t room) {
        x.reserve(room);
        y.reserve(room);
        v.reserve(room);
    }
};

// packed sink: binX, binY - binX, float32 value appended to a worker's arena; y_limit = first bin past the caller's size
struct PackedSink {
    mst_hic::PackedArena *a;
    int64_t y_limit, ymax;
    void push(int64_t bx, int64_t by, float c) {
        if (by >= y_limit) return;
        a->x.push_back((int32_t)bx);
        a->d.push_back((int32_t)(by - bx));
        a->v.push_back(c);
        ymax = by > ymax ? by : ymax;
    }
    void reserve(size_t) {}
};

// MUSTACHE_HIC_ZLIB=1: inflate through zlib instead of mst_inflate.h (the cross-check the tests use)
bool use_zlib() {
    static const bool z = [] {
        const char *e = getenv("MUSTACHE_HIC_ZLIB");
        return e && *e && *e != '0';
    }();
    return z;
}

// one zlib stream -> buf (grown until it fits: the uncompressed size is not stored); returns the byte count.
// `readable_past`: bytes known to be readable behind comp + comp_size (the decoder prefetches up to mst_inflate::kSlack).
size_t inflate_block(const uint8_t *comp, size_t comp_size, size_t readable_past, std::vector<uint8_t> &buf,
                     std::vector<uint8_t> &pad) {
    if (buf.size() < comp_size * 4 + 4096) buf.resize(comp_size * 4 + 4096);
    if (!use_zlib()) {
        const uint8_t *src = comp;
        if (readable_past < mst_inflate::kSlack) {          // the last block(s) of the file: decode from a padded copy
            pad.assign(comp_size + mst_inflate::kSlack, 0);
            memcpy(pad.data(), comp, comp_size);
            src = pad.data();
        }
        for (;;) {
            size_t n_out = 0;
            const int rc = mst_inflate::inflate_zlib(src, comp_size, buf.data(), buf.size() - mst_inflate::kSlack, &n_out);
            if (rc == mst_inflate::kOk) return n_out;
            if (rc == mst_inflate::kOutputFull && buf.size() < ((size_t)1 << 31)) {
                buf.resize(buf.size() * 2);
                continue;
            }
            throw FormatError{"zlib inflate failed"};
        }
    }
    size_t n_out = 0;
    for (;;) {
        z_stream zs;
        memset(&zs, 0, sizeof(zs));
        if (inflateInit(&zs) != Z_OK) throw FormatError{"zlib init failed"};
        zs.next_in = const_cast<Bytef *>(comp);
        zs.avail_in = (uInt)comp_size;
        zs.next_out = buf.data();
        zs.avail_out = (uInt)buf.size();
        const int rc = inflate(&zs, Z_FINISH);
        n_out = zs.total_out;
        inflateEnd(&zs);
        if (rc == Z_STREAM_END) break;
        if ((rc == Z_BUF_ERROR || rc == Z_OK) && buf.size() < ((size_t)1 << 31)) {
            buf.resize(buf.size() * 2);
            continue;
        }
        throw FormatError{"zlib inflate failed"};
    }
    return n_out;
}

template <class Sink>
void decode_records(int32_t version, const uint8_t *data, size_t n_out, Sink &out, const std::vector<double> *norm,
                    int64_t max_dist);

// block `b` of the mapped file inflated into buf
size_t inflate_block(const mst_hic *h, const BlockRef *b, std::vector<uint8_t> &buf, std::vector<uint8_t> &pad) {
    return inflate_block(h->map + b->pos, (size_t)b->size, h->size - (size_t)b->pos - (size_t)b->size, buf, pad);
}

template <class Sink>
void decode_block(const mst_hic *h, const BlockRef *b, std::vector<uint8_t> &buf, Sink &out, const std::vector<double> *norm,
                  int64_t max_dist) {
    static thread_local std::vector<uint8_t> pad;
    const size_t n_out = inflate_block(h, b, buf, pad);
    decode_records(h->version, buf.data(), n_out, out, norm, max_dist);
}

template <class Sink>
void decode_records(int32_t version, const uint8_t *data, size_t n_out, Sink &out, const std::vector<double> *norm,
                    int64_t max_dist) {
    Cursor c(data, n_out);
    const int32_t n_rec = c.get<int32_t>();
    if (n_rec < 0) throw FormatError{"negative record count in a block"};
    const size_t room = (size_t)n_rec < n_out ? (size_t)n_rec : n_out;      // a record takes at least one byte
    out.reserve(room);
    if (version < 7) {
        for (int32_t i = 0; i < n_rec; ++i) {
            const int32_t bx = c.get<int32_t>();
            const int32_t by = c.get<int32_t>();
            const float v = c.get<float>();
            emit(out, bx, by, v, norm, max_dist);
        }
        return;
    }
    const int32_t x_off = c.get<int32_t>();
    const int32_t y_off = c.get<int32_t>();
    const bool short_counts = c.get<uint8_t>() == 0;                      // 0 means "yes" in this format
    bool short_x = true, short_y = true;
    if (version > 8) {
        short_x = c.get<uint8_t>() == 0;
        short_y = c.get<uint8_t>() == 0;
    }
    const uint8_t type = c.get<uint8_t>();
    if (type == 1) {
        const int32_t rows = short_y ? (int32_t)c.get<int16_t>() : c.get<int32_t>();
        for (int32_t r = 0; r < rows; ++r) {
            const int32_t y = short_y ? (int32_t)c.get<int16_t>() : c.get<int32_t>();
            const int32_t cols = short_x ? (int32_t)c.get<int16_t>() : c.get<int32_t>();
            for (int32_t j = 0; j < cols; ++j) {
                const int32_t x = short_x ? (int32_t)c.get<int16_t>() : c.get<int32_t>();
                const float v = short_counts ? (float)c.get<int16_t>() : c.get<float>();
                emit(out, (int64_t)x_off + x, (int64_t)y_off + y, v, norm, max_dist);
            }
        }
    } else if (type == 2) {
        const int32_t n_pts = c.get<int32_t>();
        const int32_t w = (int32_t)c.get<int16_t>();
        if (w <= 0) throw FormatError{"dense block of width 0"};
        for (int32_t i = 0; i < n_pts; ++i) {
            const int32_t row = i / w, col = i - row * w;
            if (short_counts) {
                const int16_t s = c.get<int16_t>();
                if (s != -32768) emit(out, (int64_t)x_off + col, (int64_t)y_off + row, (float)s, norm, max_dist);
            } else {
                const float v = c.get<float>();
                if (!std::isnan(v)) emit(out, (int64_t)x_off + col, (int64_t)y_off + row, v, norm, max_dist);
            }
        }
    } else {
        throw FormatError{"unknown block type"};
    }
}

// ---- streaming read: records land in caller-owned slabs {x int32 [cap], v float32 [cap], dist uint16 | int32 [cap]} ----------
struct SlabSink {
    int32_t *x;
    float *v;
    void *d;
    int dist_bytes;
    int64_t count, cap, y_limit, ymax;
    void (*on_full)(SlabSink &, void *) = nullptr;        // streamed read: hand the full slab over and continue in a fresh one
    void *ctx = nullptr;
    void push(int64_t bx, int64_t by, float c) {
        if (by >= y_limit) return;
        if (count >= cap) {
            if (!on_full) throw FormatError{"a block holds more records than its header says"};
            on_full(*this, ctx);
        }
        x[count] = (int32_t)bx;
        v[count] = c;
        if (dist_bytes == 2) ((uint16_t *)d)[count] = (uint16_t)(by - bx);
        else ((int32_t *)d)[count] = (int32_t)(by - bx);
        ++count;
        ymax = by > ymax ? by : ymax;
    }
    void reserve(size_t) {}
};

// The layout almost every block of a real file has -- version 7-9, list of rows -- decoded with raw pointers: the row's byte
// extent is checked once, the records go through the same emit() as the general decoder (same filters, same arithmetic).
// Returns false when the block is of another kind (the caller then runs decode_records).
template <bool SHORT_X, bool SHORT_C>
void decode_rows(const uint8_t *p, const uint8_t *end, int32_t rows, bool short_y, int32_t x_off, int32_t y_off, SlabSink &out,
                 const std::vector<double> *norm, int64_t max_dist) {
    constexpr size_t rec = (SHORT_X ? 2 : 4) + (SHORT_C ? 2 : 4);
    for (int32_t r = 0; r < rows; ++r) {
        const size_t head = (short_y ? 2 : 4) + (SHORT_X ? 2 : 4);
        if ((size_t)(end - p) < head) throw FormatError{"truncated structure"};
        int32_t y, cols;
        if (short_y) {
            int16_t t;
            memcpy(&t, p, 2);
            y = t;
            p += 2;
        } else {
            memcpy(&y, p, 4);
            p += 4;
        }
        if (SHORT_X) {
            int16_t t;
            memcpy(&t, p, 2);
            cols = t;
            p += 2;
        } else {
            memcpy(&cols, p, 4);
            p += 4;
        }
        if (cols < 0) cols = 0;                                   // the general decoder's loop runs zero times as well
        if ((size_t)(end - p) < (size_t)cols * rec) throw FormatError{"truncated structure"};
        const int64_t by = (int64_t)y_off + y;
        for (int32_t j = 0; j < cols; ++j) {
            int32_t x;
            float val;
            if (SHORT_X) {
                int16_t t;
                memcpy(&t, p, 2);
                x = t;
                p += 2;
            } else {
                memcpy(&x, p, 4);
                p += 4;
            }
            if (SHORT_C) {
                int16_t t;
                memcpy(&t, p, 2);
                val = (float)t;
                p += 2;
            } else {
                memcpy(&val, p, 4);
                p += 4;
            }
            emit(out, (int64_t)x_off + x, by, val, norm, max_dist);
        }
    }
}

bool decode_rows_fast(int32_t version, const uint8_t *data, size_t n, SlabSink &out, const std::vector<double> *norm,
                      int64_t max_dist) {
    if (version < 7) return false;
    const size_t hdr = 4 + 4 + 4 + 1 + (version > 8 ? 2 : 0) + 1;
    if (n < hdr) return false;
    const uint8_t *p = data + 4;
    int32_t x_off, y_off;
    memcpy(&x_off, p, 4);
    memcpy(&y_off, p + 4, 4);
    p += 8;
    const bool short_c = *p++ == 0;
    bool short_x = true, short_y = true;
    if (version > 8) {
        short_x = *p++ == 0;
        short_y = *p++ == 0;
    }
    if (*p++ != 1) return false;
    const uint8_t *end = data + n;
    int32_t rows;
    if (short_y) {
        if (end - p < 2) return false;
        int16_t t;
        memcpy(&t, p, 2);
        rows = t;
        p += 2;
    } else {
        if (end - p < 4) return false;
        memcpy(&rows, p, 4);
        p += 4;
    }
    if (short_x && short_c) decode_rows<true, true>(p, end, rows, short_y, x_off, y_off, out, norm, max_dist);
    else if (short_x) decode_rows<true, false>(p, end, rows, short_y, x_off, y_off, out, norm, max_dist);
    else if (short_c) decode_rows<false, true>(p, end, rows, short_y, x_off, y_off, out, norm, max_dist);
    else decode_rows<false, false>(p, end, rows, short_y, x_off, y_off, out, norm, max_dist);
    return true;
}

int find_chromosome(const mst_hic *h, const char *name) {
    const std::string want(name);
    const std::string bare = want.rfind("chr", 0) == 0 ? want.substr(3) : want;
    for (int pass = 0; pass < 2; ++pass)
        for (size_t i = 0; i < h->chroms.size(); ++i) {
            const std::string &n = h->chroms[i].name;
            if (pass == 0 ? n == want : (n == bare || n == "chr" + bare)) return (int)i;
        }
    return -1;
}

}  // namespace

extern "C" int mst_io_abi_version(void) { return MST_IO_ABI_VERSION; }
extern "C" const char *mst_io_last_error(void) { return g_err; }
extern "C" void mst_io_free(void *p) { free(p); }

extern "C" int64_t mst_io_inflate(const uint8_t *src, int64_t n, uint8_t *dst, int64_t capacity) {
    if (!src || !dst || n < 0 || capacity < 0) return fail(MST_IO_E_ARG, "mst_io_inflate: bad argument");
    std::vector<uint8_t> in((size_t)n + mst_inflate::kSlack, 0), out((size_t)capacity + mst_inflate::kSlack);
    memcpy(in.data(), src, (size_t)n);
    size_t produced = 0;
    const int rc = mst_inflate::inflate_zlib(in.data(), (size_t)n, out.data(), (size_t)capacity, &produced);
    if (rc == mst_inflate::kOutputFull) return fail(MST_IO_E_ARG, "mst_io_inflate: output does not fit %lld bytes", (long long)capacity);
    if (rc != mst_inflate::kOk) return fail(MST_IO_E_ZLIB, "mst_io_inflate: not a valid zlib stream");
    memcpy(dst, out.data(), produced);
    return (int64_t)produced;
}

extern "C" int mst_hic_open(const char *path, mst_hic **out) {
    if (!path || !out) return fail(MST_IO_E_ARG, "mst_hic_open: null argument");
    *out = nullptr;
    mst_hic *h = new (std::nothrow) mst_hic();
    if (!h) return fail(MST_IO_E_FILE, "out of memory");
    h->fd = open(path, O_RDONLY);
    struct stat st;
    if (h->fd < 0 || fstat(h->fd, &st) != 0 || st.st_size <= 0) {
        mst_hic_close(h);
        return fail(MST_IO_E_FILE, "cannot open %s", path);
    }
    h->size = (size_t)st.st_size;
    void *m = mmap(nullptr, h->size, PROT_READ, MAP_PRIVATE, h->fd, 0);
    if (m == MAP_FAILED) {
        mst_hic_close(h);
        return fail(MST_IO_E_FILE, "cannot map %s", path);
    }
    h->map = (const uint8_t *)m;
    try {
        parse_header(h);
        parse_master_index(h);
    } catch (const FormatError &e) {
        mst_hic_close(h);
        return fail(MST_IO_E_FORMAT, "%s: %s", path, e.what);
    } catch (...) {
        mst_hic_close(h);
        return fail(MST_IO_E_FORMAT, "%s: unreadable", path);
    }
    *out = h;
    return MST_IO_OK;
}

extern "C" void mst_hic_close(mst_hic *h) {
    if (!h) return;
    if (h->map) munmap((void *)h->map, h->size);
    if (h->fd >= 0) close(h->fd);
    delete h;
}

extern "C" int32_t mst_hic_version(const mst_hic *h) { return h ? h->version : 0; }
extern "C" int64_t mst_hic_master_offset(const mst_hic *h) { return h ? h->master : 0; }
extern "C" const char *mst_hic_genome(const mst_hic *h) { return h ? h->genome.c_str() : ""; }
extern "C" int32_t mst_hic_n_chromosomes(const mst_hic *h) { return h ? (int32_t)h->chroms.size() : 0; }
extern "C" int mst_hic_chromosome(const mst_hic *h, int32_t i, const char **name, int64_t *length) {
    if (!h || i < 0 || (size_t)i >= h->chroms.size()) return fail(MST_IO_E_ARG, "mst_hic_chromosome: bad index");
    if (name) *name = h->chroms[(size_t)i].name.c_str();
    if (length) *length = h->chroms[(size_t)i].length;
    return MST_IO_OK;
}
extern "C" int32_t mst_hic_n_resolutions(const mst_hic *h) { return h ? (int32_t)h->bp_res.size() : 0; }
extern "C" int32_t mst_hic_resolution(const mst_hic *h, int32_t i) {
    return (h && i >= 0 && (size_t)i < h->bp_res.size()) ? h->bp_res[(size_t)i] : 0;
}

// Worker threads when the caller passes n_threads <= 0: the hardware concurrency, capped at twice the container's CPU
// quota when there is one (cgroup v2 cpu.max / v1 cpu.cfs_quota_us): inflate is compute bound, and 256 threads on a 16-CPU
// quota run slower than 32 (measured on the GPU box: 0.20 s against 0.12 s for 125 M records).
static int default_threads() {
    int hw = (int)std::thread::hardware_concurrency();
    if (hw < 1) hw = 1;
    double quota = 0.0;
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char a[64] = {0};
        long long period = 0;
        if (fscanf(f, "%63s %lld", a, &period) == 2 && strcmp(a, "max") != 0 && period > 0) quota = atof(a) / (double)period;
        fclose(f);
    } else if (FILE *g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
        long long q = -1, period = 0;
        if (fscanf(g, "%lld", &q) != 1) q = -1;
        fclose(g);
        if (FILE *p = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
            if (fscanf(p, "%lld", &period) != 1) period = 0;
            fclose(p);
        }
        if (q > 0 && period > 0) quota = (double)q / (double)period;
    }
    if (quota > 0.0) {
        const int cap = (int)(2.0 * quota + 0.5);
        if (cap >= 1 && cap < hw) hw = cap;
    }
    return hw;
}

// The ONE thread-count rule: the caller's request or the default, at least 1, at most one per job, and for a stream at most
// `slab_bound` = n_slabs - 1 (every worker holds a slab; one more keeps the consumer fed).
static int worker_count(int32_t requested, size_t jobs, int32_t slab_bound = 0) {
    int nt = requested > 0 ? requested : default_threads();
    if (nt < 1) nt = 1;
    if ((size_t)nt > jobs) nt = jobs ? (int)jobs : 1;
    if (slab_bound > 0 && nt > slab_bound) nt = slab_bound;
    return nt;
}

static int decode_failed(const char *what) { return fail(MST_IO_E_ZLIB, "block decode failed: %s", what); }

// The exception tail of every entry point that parses the file on the calling thread.
template <class F>
static auto guarded(F body) -> decltype(body()) {
    try {
        return body();
    } catch (const FormatError &e) {
        return fail(MST_IO_E_FORMAT, "%s", e.what);
    } catch (...) {
        return fail(MST_IO_E_FORMAT, "unreadable file (out of memory?)");
    }
}

// The one-shot forms' block runner: body(i, t) for i in [0, n) on nt threads, t = the worker's index (dynamic dealing).  The
// first exception wins and stops the dealing; returns its text (FormatError texts are literals), or null when all went well.
template <class F>
static const char *run_blocks(size_t n, int nt, F body) {
    std::atomic<size_t> next(0);
    std::atomic<const char *> bad(nullptr);
    auto work = [&](int t) {
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= n || bad.load()) return;
            const char *what = nullptr;
            try {
                body(i, t);
            } catch (const FormatError &e) {
                what = e.what;
            } catch (...) {
                what = "out of memory";
            }
            if (what) {
                const char *none = nullptr;
                bad.compare_exchange_strong(none, what);
                return;
            }
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; ++t) pool.emplace_back(work, t);
    work(0);
    for (auto &t : pool) t.join();
    return bad.load();
}

// The ONE prologue of every read: what a read needs of one matrix at one resolution.  `todo` points into `zoom.blocks`, so a
// Matrix is filled where it stays (a stream holds one as a member) and is never copied.
struct Matrix {
    ZoomData zoom;
    std::vector<const BlockRef *> todo;
    std::vector<double> norm_vec, norm_vec2;                          // pair: the vectors of A and of B
    bool use_norm = false;
    int64_t chrom_length = 0, chrom_length2 = 0;
    int32_t transposed = 0;                                           // pair: the file stores it as (B, A)
};

// chrom_b == null: the intra matrix of chrom_a, its blocks that can hold a record within max_dist_bins of the diagonal;
// otherwise the matrix of the pair (chrom_a, chrom_b), every block; `fn` = the entry point, named when the pair is no pair.
// Returns 0 or an MST_IO_E_* code (message set).
static int open_matrix(mst_hic *h, const char *chrom_a, const char *chrom_b, int32_t resolution, const char *norm,
                       int64_t max_dist_bins, Matrix &m, const char *fn = "") {
    const int ca = find_chromosome(h, chrom_a), cb = chrom_b ? find_chromosome(h, chrom_b) : ca;
    if (ca < 0) return fail(MST_IO_E_NOTFOUND, "chromosome %s is not in the file", chrom_a);
    if (cb < 0) return fail(MST_IO_E_NOTFOUND, "chromosome %s is not in the file", chrom_b);
    if (chrom_b && ca == cb) return fail(MST_IO_E_ARG, "%s: %s and %s are one chromosome", fn, chrom_a, chrom_b);
    const int lo = ca < cb ? ca : cb, hi = ca < cb ? cb : ca;
    auto it = h->matrices.find(std::to_string(lo) + "_" + std::to_string(hi));
    if (it == h->matrices.end())
        return chrom_b ? fail(MST_IO_E_NOTFOUND, "no matrix for the pair %s, %s", chrom_a, chrom_b)
                       : fail(MST_IO_E_NOTFOUND, "no intra-chromosomal matrix for %s", chrom_a);
    m.zoom = read_zoom(h, it->second.first, resolution);
    if (!m.zoom.found) return fail(MST_IO_E_NOTFOUND, "resolution %d is not in the file", resolution);
    m.use_norm = norm && *norm && strcmp(norm, "NONE") != 0;
    if (m.use_norm) {
        read_norm_index(h);
        for (int side = 0; side < (chrom_b ? 2 : 1); ++side) {
            const int ci = side ? cb : ca;
            auto nit = h->norm_index.find(norm_key(norm, ci, "BP", resolution));
            if (nit == h->norm_index.end())
                return fail(MST_IO_E_NOTFOUND, "no %s normalisation vector for %s at %d bp", norm,
                            chrom_b ? h->chroms[(size_t)ci].name.c_str() : chrom_a, resolution);
            (side ? m.norm_vec2 : m.norm_vec) = read_norm_vector(h, nit->second);
        }
    }
    for (const BlockRef &b : m.zoom.blocks) {
        if (b.size <= 0) continue;
        if (b.pos < 0 || (uint64_t)b.pos + (uint64_t)b.size > h->size) throw FormatError{"block outside the file"};
        if (chrom_b || block_near_diagonal(h->version, b.number, m.zoom.block_bin_count, m.zoom.block_column_count, max_dist_bins))
            m.todo.push_back(&b);
    }
    m.chrom_length = h->chroms[(size_t)ca].length;
    m.chrom_length2 = h->chroms[(size_t)cb].length;
    m.transposed = ca > cb ? 1 : 0;
    return MST_IO_OK;
}

// Part `part` of `n_parts` of a chromosome's block list (one process per GPU, each rank inflates its share): a contiguous run
// of the near-diagonal blocks in file index order, cut so that the parts hold equal shares of the COMPRESSED bytes (block i
// belongs to the part its byte midpoint falls into) -- every block belongs to exactly one part, whatever n_parts is.  The ONE
// definition every reader uses: ranks that disagreed on it would drop or double-decode blocks without any error.
static void split_todo(std::vector<const BlockRef *> &todo, int32_t part, int32_t n_parts) {
    if (n_parts <= 1) return;
    double total = 0.0, run = 0.0;
    for (const BlockRef *b : todo) total += (double)b->size;
    std::vector<const BlockRef *> own;
    for (const BlockRef *b : todo) {
        const double mid = run + 0.5 * (double)b->size;
        run += (double)b->size;
        int p = total > 0.0 ? (int)(mid / total * (double)n_parts) : 0;
        p = p < 0 ? 0 : (p >= n_parts ? n_parts - 1 : p);
        if (p == part) own.push_back(b);
    }
    todo.swap(own);
}

extern "C" int64_t mst_hic_read_intra(mst_hic *h, const char *chrom, int32_t resolution, const char *norm,
                                      int64_t max_dist_bins, int32_t n_threads, int64_t **x, int64_t **y, double **v) {
    if (!h || !chrom || !x || !y || !v || resolution <= 0) return fail(MST_IO_E_ARG, "mst_hic_read_intra: bad argument");
    *x = *y = nullptr;
    *v = nullptr;
    return guarded([&]() -> int64_t {
        Matrix m;
        const int rc = open_matrix(h, chrom, nullptr, resolution, norm, max_dist_bins, m);
        if (rc != MST_IO_OK) return rc;
        // one Records per block, in file block order
        const int nt = worker_count(n_threads, m.todo.size());
        std::vector<Records> part(m.todo.size());
        std::vector<std::vector<uint8_t>> bufs((size_t)nt);
        const char *bad = run_blocks(part.size(), nt, [&](size_t i, int t) {
            decode_block(h, m.todo[i], bufs[(size_t)t], part[i], m.use_norm ? &m.norm_vec : nullptr, max_dist_bins);
        });
        if (bad) return decode_failed(bad);
        std::vector<size_t> offs(part.size() + 1, 0);
        for (size_t i = 0; i < part.size(); ++i) offs[i + 1] = offs[i] + part[i].v.size();
        const size_t total = offs[part.size()];
        int64_t *ox = (int64_t *)malloc((total ? total : 1) * sizeof(int64_t));
        int64_t *oy = (int64_t *)malloc((total ? total : 1) * sizeof(int64_t));
        double *ov = (double *)malloc((total ? total : 1) * sizeof(double));
        if (!ox || !oy || !ov) {
            free(ox);
            free(oy);
            free(ov);
            return fail(MST_IO_E_FILE, "out of memory for %zu records", total);
        }
        // concatenate in file block order (deterministic), the copies spread over the same worker threads (memcpy and the
        // release of a vector cannot throw: nothing to report)
        (void)run_blocks(part.size(), nt, [&](size_t i, int) {
            Records &r = part[i];
            if (r.v.empty()) return;
            memcpy(ox + offs[i], r.x.data(), r.v.size() * sizeof(int64_t));
            memcpy(oy + offs[i], r.y.data(), r.v.size() * sizeof(int64_t));
            memcpy(ov + offs[i], r.v.data(), r.v.size() * sizeof(double));
            std::vector<int64_t>().swap(r.x);                      // release the block's buffers as we go
            std::vector<int64_t>().swap(r.y);
            std::vector<double>().swap(r.v);
        });
        *x = ox;
        *y = oy;
        *v = ov;
        return (int64_t)total;
    });
}

extern "C" int64_t mst_hic_decode_intra_packed(mst_hic *h, const char *chrom, int32_t resolution, const char *norm,
                                               int64_t max_dist_bins, int64_t chrom_size_bp, int32_t n_threads,
                                               int64_t *n_bins) {
    return mst_hic_decode_intra_packed_part(h, chrom, resolution, norm, max_dist_bins, chrom_size_bp, n_threads, 0, 1, n_bins,
                                            nullptr, nullptr);
}

extern "C" int64_t mst_hic_decode_intra_packed_part(mst_hic *h, const char *chrom, int32_t resolution, const char *norm,
                                                    int64_t max_dist_bins, int64_t chrom_size_bp, int32_t n_threads,
                                                    int32_t part, int32_t n_parts, int64_t *n_bins, int32_t *blocks_total,
                                                    int32_t *blocks_mine) {
    if (!h || !chrom || !n_bins || resolution <= 0 || n_parts < 1 || part < 0 || part >= n_parts)
        return fail(MST_IO_E_ARG, "mst_hic_decode_intra_packed: bad argument");
    *n_bins = 0;
    h->packed_total = -1;
    return guarded([&]() -> int64_t {
        Matrix m;
        const int rc = open_matrix(h, chrom, nullptr, resolution, norm, max_dist_bins, m);
        if (rc != MST_IO_OK) return rc;
        if (blocks_total) *blocks_total = (int32_t)m.todo.size();
        split_todo(m.todo, part, n_parts);
        if (blocks_mine) *blocks_mine = (int32_t)m.todo.size();
        const int nt = worker_count(n_threads, m.todo.size());
        if (h->arenas.size() < (size_t)nt) h->arenas.resize((size_t)nt);
        if (h->inflate_bufs.size() < (size_t)nt) h->inflate_bufs.resize((size_t)nt);
        for (auto &a : h->arenas) {
            a.x.clear();
            a.d.clear();
            a.v.clear();
        }
        h->spans.assign(m.todo.size(), mst_hic::PackedSpan{0, 0, 0});
        // straw's window end (mustache.py:320-333): no position at or past the chromosome size the caller gave
        const int64_t y_limit = chrom_size_bp > 0 ? (chrom_size_bp + resolution - 1) / resolution : INT64_MAX;
        struct alignas(64) Own {                                   // one per worker, a cache line each: ymax moves with every record
            PackedSink sink;
        };
        std::vector<Own> sinks;
        for (int t = 0; t < nt; ++t) sinks.push_back(Own{PackedSink{&h->arenas[(size_t)t], y_limit, -1}});
        const char *bad = run_blocks(m.todo.size(), nt, [&](size_t i, int t) {
            PackedSink &sink = sinks[(size_t)t].sink;
            const size_t before = sink.a->v.size();
            decode_block(h, m.todo[i], h->inflate_bufs[(size_t)t], sink, m.use_norm ? &m.norm_vec : nullptr, max_dist_bins);
            h->spans[i] = mst_hic::PackedSpan{t, before, sink.a->v.size() - before};
        });
        if (bad) return decode_failed(bad);
        int64_t total = 0, top = -1;
        for (const auto &sp : h->spans) total += (int64_t)sp.count;
        for (const Own &o : sinks) top = o.sink.ymax > top ? o.sink.ymax : top;
        if (top >= INT32_MAX) return fail(MST_IO_E_FORMAT, "bin index %lld does not fit 32 bits", (long long)top);
        h->packed_total = total;
        *n_bins = top + 1;
        return total;
    });
}

extern "C" int mst_hic_fetch_packed(mst_hic *h, int32_t *x, int32_t *dist, float *v, int64_t capacity, int32_t n_threads) {
    if (!h || h->packed_total < 0) return fail(MST_IO_E_ARG, "mst_hic_fetch_packed: no decoded records (call mst_hic_decode_intra_packed)");
    if (capacity < h->packed_total || (h->packed_total > 0 && (!x || !dist || !v)))
        return fail(MST_IO_E_ARG, "mst_hic_fetch_packed: room for %lld records, %lld decoded", (long long)capacity,
                    (long long)h->packed_total);
    std::vector<size_t> offs(h->spans.size() + 1, 0);
    for (size_t i = 0; i < h->spans.size(); ++i) offs[i + 1] = offs[i] + h->spans[i].count;
    // file block order (deterministic whatever thread decoded a block), the copies spread over the worker threads (plain
    // memcpy: the body cannot throw, nothing to report)
    (void)run_blocks(h->spans.size(), worker_count(n_threads, h->spans.size()), [&](size_t i, int) {
        const mst_hic::PackedSpan &sp = h->spans[i];
        if (!sp.count) return;
        const mst_hic::PackedArena &a = h->arenas[(size_t)sp.arena];
        memcpy(x + offs[i], a.x.data() + sp.begin, sp.count * sizeof(int32_t));
        memcpy(dist + offs[i], a.d.data() + sp.begin, sp.count * sizeof(int32_t));
        memcpy(v + offs[i], a.v.data() + sp.begin, sp.count * sizeof(float));
    });
    return MST_IO_OK;
}

extern "C" int64_t mst_hic_read_intra_packed(mst_hic *h, const char *chrom, int32_t resolution, const char *norm,
                                             int64_t max_dist_bins, int64_t chrom_size_bp, int32_t n_threads,
                                             int32_t **x, int32_t **dist, float **v, int64_t *n_bins) {
    if (!x || !dist || !v) return fail(MST_IO_E_ARG, "mst_hic_read_intra_packed: bad argument");
    *x = *dist = nullptr;
    *v = nullptr;
    const int64_t total = mst_hic_decode_intra_packed(h, chrom, resolution, norm, max_dist_bins, chrom_size_bp, n_threads,
                                                      n_bins);
    if (total < 0) return total;
    int32_t *ox = (int32_t *)malloc((size_t)(total ? total : 1) * sizeof(int32_t));
    int32_t *od = (int32_t *)malloc((size_t)(total ? total : 1) * sizeof(int32_t));
    float *ov = (float *)malloc((size_t)(total ? total : 1) * sizeof(float));
    if (!ox || !od || !ov) {
        free(ox);
        free(od);
        free(ov);
        return fail(MST_IO_E_FILE, "out of memory for %lld records", (long long)total);
    }
    const int rc = mst_hic_fetch_packed(h, ox, od, ov, total, n_threads);
    if (rc != MST_IO_OK) {
        free(ox);
        free(od);
        free(ov);
        return rc;
    }
    *x = ox;
    *dist = od;
    *v = ov;
    return total;
}

// ---- the slab queue of the streamed reads ------------------------------------------------------------------------------------
// Slabs of caller-owned memory travel in a circle: free -> a worker fills one -> ready -> the consumer -> released -> free.
// Worker threads deal the blocks of the stream's `matrix.todo` among themselves; what they do with a block is the stream's
// Worker (block(b), publish(), and leave() under the lock when the thread ends).  A stream's per-slab metadata and totals are
// written and read under this queue's lock: publish() and wait_ready() run the caller's `meta` while they hold it.
struct SlabQueue {
    struct Cancelled {};
    std::mutex mu;
    std::condition_variable cv_free, cv_ready;
    std::deque<int32_t> free_q, ready_q;
    std::vector<std::thread> workers;
    std::atomic<size_t> next{0};
    int active = 0;
    bool failed = false, cancelled = false;
    std::string error;

    void fail_with(const char *what) {
        std::lock_guard<std::mutex> lk(mu);
        if (!failed) error = what;
        failed = true;
        cv_free.notify_all();
        cv_ready.notify_all();
    }

    // a free slab for a worker; waits for one, gives up (Cancelled) when the stream has failed or is being closed
    int32_t acquire() {
        std::unique_lock<std::mutex> lk(mu);
        cv_free.wait(lk, [&] { return !free_q.empty() || failed || cancelled; });
        if (failed || cancelled) throw Cancelled{};
        const int32_t slab = free_q.front();
        free_q.pop_front();
        return slab;
    }

    // a worker is done with `slab`: to the consumer when it holds something, straight back to the free slabs when not
    template <class Meta>
    void publish(int32_t slab, bool has_content, Meta meta) {
        std::lock_guard<std::mutex> lk(mu);
        meta();
        if (has_content) {
            ready_q.push_back(slab);
            cv_ready.notify_one();
        } else {
            free_q.push_back(slab);
            cv_free.notify_one();
        }
    }

    // the consumer's side: 1 = meta(slab) was called for a filled slab, 2 = nothing yet, 0 = all delivered, < 0 = a worker failed
    template <class Meta>
    int wait_ready(int32_t timeout_ms, Meta meta) {
        std::unique_lock<std::mutex> lk(mu);
        auto ready = [&] { return !ready_q.empty() || failed || active == 0; };
        if (timeout_ms < 0) cv_ready.wait(lk, ready);
        else if (!cv_ready.wait_for(lk, std::chrono::milliseconds(timeout_ms), ready)) return 2;
        if (failed) return decode_failed(error.c_str());
        if (ready_q.empty()) return 0;
        meta(ready_q.front());
        ready_q.pop_front();
        return 1;
    }

    void release(int32_t slab) {
        std::lock_guard<std::mutex> lk(mu);
        free_q.push_back(slab);
        cv_free.notify_one();
    }

    void cancel_and_join() {
        {
            std::lock_guard<std::mutex> lk(mu);
            cancelled = true;
            cv_free.notify_all();
        }
        for (auto &t : workers) t.join();
    }

    template <class Stream>
    void work(Stream *s) {
        typename Stream::Worker w(s);
        try {
            for (;;) {
                const size_t i = next.fetch_add(1);
                if (i >= s->matrix.todo.size()) break;
                {
                    std::lock_guard<std::mutex> lk(mu);
                    if (failed || cancelled) break;
                }
                w.block(s->matrix.todo[i]);
            }
            w.publish();
        } catch (const Cancelled &) {
        } catch (const FormatError &e) {
            fail_with(e.what);
        } catch (...) {
            fail_with("out of memory");
        }
        std::lock_guard<std::mutex> lk(mu);
        w.leave();
        if (--active == 0) cv_ready.notify_all();
    }

    // every slab free, then the workers: the stream's thread count under the n_slabs - 1 cap
    template <class Stream>
    void start(Stream *s, int32_t n_threads, int32_t n_slabs) {
        for (int32_t i = 0; i < n_slabs; ++i) free_q.push_back(i);
        const int nt = active = worker_count(n_threads, s->matrix.todo.size(), n_slabs - 1);
        for (int t = 0; t < nt; ++t) workers.emplace_back([this, s] { work(s); });       // (a worker that ends lowers `active`)
    }
};

// ---- streaming packed read -------------------------------------------------------------------------------------------------
// Worker threads inflate and decode the chromosome's near-diagonal blocks (this part's share of them) straight into
// caller-owned slabs; a slab is handed to the consumer as soon as the next block would not fit, so the consumer's H2D copies
// run while later blocks are still being inflated.  No arena, no second copy, no total count needed in advance.
struct mst_hic_stream {
    mst_hic *h = nullptr;
    Matrix matrix;
    int64_t max_dist = -1, y_limit = INT64_MAX;
    uint8_t *base = nullptr;
    int32_t n_slabs = 0, dist_bytes = 2;
    int64_t cap = 0;
    std::vector<int64_t> counts;
    int64_t ymax = -1, total = 0;
    int32_t blocks_total = 0;
    SlabQueue q;

    // One worker: blocks are decoded straight into the slab it holds; a slab is handed over exactly when it is FULL (in the
    // middle of a block if need be: a block may hold more records than a slab) and at the end of the work list, so the
    // consumer sees a steady flow of full slabs however many workers there are.
    struct Worker {
        mst_hic_stream *s;
        int32_t cur = -1;
        SlabSink sink;
        std::vector<uint8_t> buf, pad;
        explicit Worker(mst_hic_stream *st) : s(st), sink{nullptr, nullptr, nullptr, st->dist_bytes, 0, 0, st->y_limit, -1} {
            sink.on_full = &Worker::full;
            sink.ctx = this;
        }
        void publish() {
            if (cur < 0) return;
            s->q.publish(cur, sink.count > 0, [&] {
                s->counts[(size_t)cur] = sink.count;
                s->total += sink.count;
            });
            cur = -1;
        }
        void next_slab() {
            publish();
            cur = s->q.acquire();
            uint8_t *m = s->base + (size_t)cur * (size_t)s->cap * (size_t)(8 + s->dist_bytes);
            sink.x = reinterpret_cast<int32_t *>(m);
            sink.v = reinterpret_cast<float *>(m + (size_t)s->cap * 4);
            sink.d = m + (size_t)s->cap * 8;
            sink.count = 0;
            sink.cap = s->cap;
        }
        static void full(SlabSink &, void *self) { static_cast<Worker *>(self)->next_slab(); }
        void block(const BlockRef *b) {
            const size_t n_out = inflate_block(s->h, b, buf, pad);
            if (n_out < 4) throw FormatError{"truncated structure"};
            int32_t n_rec;
            memcpy(&n_rec, buf.data(), 4);
            if (n_rec < 0) throw FormatError{"negative record count in a block"};
            if (cur < 0) next_slab();
            const std::vector<double> *norm = s->matrix.use_norm ? &s->matrix.norm_vec : nullptr;
            if (!decode_rows_fast(s->h->version, buf.data(), n_out, sink, norm, s->max_dist))
                decode_records(s->h->version, buf.data(), n_out, sink, norm, s->max_dist);
        }
        void leave() { s->ymax = sink.ymax > s->ymax ? sink.ymax : s->ymax; }
    };
};

extern "C" int mst_hic_stream_open(mst_hic *h, const char *chrom, int32_t resolution, const char *norm, int64_t max_dist_bins,
                                   int64_t chrom_size_bp, int32_t n_threads, int32_t part, int32_t n_parts, void *slab_memory,
                                   int32_t n_slabs, int64_t slab_records, int32_t dist_bytes, mst_hic_stream **out) {
    if (!h || !chrom || !out || resolution <= 0 || n_parts < 1 || part < 0 || part >= n_parts || !slab_memory || n_slabs < 2 ||
        slab_records < 2 || (slab_records & 1) || (dist_bytes != 2 && dist_bytes != 4) ||
        (reinterpret_cast<uintptr_t>(slab_memory) & 3))
        return fail(MST_IO_E_ARG, "mst_hic_stream_open: bad argument (slab_records must be even, slab_memory 4-byte aligned)");
    if (dist_bytes == 2 && (max_dist_bins < 0 || max_dist_bins > 65535))
        return fail(MST_IO_E_ARG, "mst_hic_stream_open: 16-bit distances need 0 <= max_dist_bins <= 65535");
    *out = nullptr;
    return guarded([&]() -> int {
        std::unique_ptr<mst_hic_stream> s(new mst_hic_stream());
        s->h = h;
        const int rc = open_matrix(h, chrom, nullptr, resolution, norm, max_dist_bins, s->matrix);
        if (rc != MST_IO_OK) return rc;
        s->blocks_total = (int32_t)s->matrix.todo.size();
        split_todo(s->matrix.todo, part, n_parts);
        s->max_dist = max_dist_bins;
        s->y_limit = chrom_size_bp > 0 ? (chrom_size_bp + resolution - 1) / resolution : INT64_MAX;
        s->base = static_cast<uint8_t *>(slab_memory);
        s->n_slabs = n_slabs;
        s->cap = slab_records;
        s->dist_bytes = dist_bytes;
        s->counts.assign((size_t)n_slabs, 0);
        s->q.start(s.get(), n_threads, n_slabs);
        *out = s.release();
        return MST_IO_OK;
    });
}

extern "C" int mst_hic_stream_next(mst_hic_stream *s, int32_t timeout_ms, int32_t *slab, int64_t *count) {
    if (!s || !slab || !count) return fail(MST_IO_E_ARG, "mst_hic_stream_next: bad argument");
    return s->q.wait_ready(timeout_ms, [&](int32_t i) {
        *slab = i;
        *count = s->counts[(size_t)i];
    });
}

extern "C" int mst_hic_stream_release(mst_hic_stream *s, int32_t slab) {
    if (!s || slab < 0 || slab >= s->n_slabs) return fail(MST_IO_E_ARG, "mst_hic_stream_release: bad argument");
    s->q.release(slab);
    return MST_IO_OK;
}

extern "C" int mst_hic_stream_close(mst_hic_stream *s, int64_t *n_bins, int64_t *total, int32_t *blocks_total,
                                    int32_t *blocks_mine) {
    if (!s) return MST_IO_OK;
    s->q.cancel_and_join();
    int rc = MST_IO_OK;
    if (s->q.failed) rc = decode_failed(s->q.error.c_str());
    else if (s->ymax >= INT32_MAX) rc = fail(MST_IO_E_FORMAT, "bin index %lld does not fit 32 bits", (long long)s->ymax);
    if (n_bins) *n_bins = s->ymax + 1;
    if (total) *total = s->total;
    if (blocks_total) *blocks_total = s->blocks_total;
    if (blocks_mine) *blocks_mine = (int32_t)s->matrix.todo.size();
    delete s;
    return rc;
}

// ---- streaming RAW read: the host only inflates ----------------------------------------------------------------------------
// Worker threads inflate the chromosome's near-diagonal blocks (this part's share of them) and copy the RECORD BYTES of every
// row, exactly as the file stores them (2 or 4 bytes of column + 2 or 4 bytes of count: 6 bytes per record in the usual
// float-count file, against the 10 of a decoded packed record), into caller-owned slabs, with one 16-byte directory entry per
// row {byte offset, binY, binXOffset, record count | layout flags}.  The rows are decoded -- columns, counts, normalisation
// vector, distance / NaN / sign filters, scatter into the band -- by a kernel (mst_band_scatter_hic_rows in
// libmustache_hip.so), so no host thread touches a record.  Slab layout: payload from byte 0 upwards, directory entries from
// the slab's end downwards (entry k at slab_bytes - 16 (k + 1)); a slab is handed over when the next row would not fit.
// A block may be split between slabs at any row.  v6 blocks (plain records, no rows) are not served: MST_IO_E_FORMAT at open.
// A trans stream delivers EVERY block of a pair's matrix in the same way.
struct mst_hic_rawstream {
    mst_hic *h = nullptr;
    Matrix matrix;
    uint8_t *base = nullptr;
    int32_t n_slabs = 0;
    int64_t slab_bytes = 0;
    std::vector<int64_t> pay_bytes;
    std::vector<int32_t> row_count;
    int64_t rows_total = 0, bytes_total = 0;
    int32_t blocks_total = 0;
    SlabQueue q;

    struct Worker {
        mst_hic_rawstream *s;
        int32_t cur = -1;
        uint8_t *m = nullptr;
        int64_t pay = 0;
        int32_t rows = 0;
        std::vector<uint8_t> buf, pad;
        double ratio = 2.0;                       // the largest expansion of a block this worker has seen, with a margin
        explicit Worker(mst_hic_rawstream *st) : s(st) {}
        void publish() {
            if (cur < 0) return;
            s->q.publish(cur, rows > 0, [&] {
                s->pay_bytes[(size_t)cur] = pay;
                s->row_count[(size_t)cur] = rows;
                s->rows_total += rows;
                s->bytes_total += pay;
            });
            cur = -1;
        }
        void next_slab() {
            publish();
            cur = s->q.acquire();
            m = s->base + (size_t)cur * (size_t)s->slab_bytes;
            pay = 0;
            rows = 0;
        }
        void leave() {}
        // directory entry of a row whose records already lie in this slab at byte `off`
        void list_row(int64_t off, int64_t count, int64_t y, int32_t x_off, uint32_t flags) {
            if (y < INT32_MIN || y > INT32_MAX) throw FormatError{"bin index does not fit 32 bits"};
            if (count >= ((int64_t)1 << 28)) throw FormatError{"a row holds more records than a slab"};
            mst_hic_row e{(uint32_t)off, (int32_t)y, x_off, (uint32_t)count | flags};
            memcpy(m + s->slab_bytes - 16 * ((int64_t)rows + 1), &e, 16);
            ++rows;
        }
        // one row: `count` records of `rec` bytes at p (columns + counts, or counts alone for a dense grid's row), copied in
        void put_row(const uint8_t *p, int64_t count, int64_t rec, int64_t y, int32_t x_off, uint32_t flags) {
            if (count <= 0) return;
            if (y < INT32_MIN || y > INT32_MAX) throw FormatError{"bin index does not fit 32 bits"};
            if (count >= ((int64_t)1 << 28)) throw FormatError{"a row holds more records than a slab"};
            const int64_t need = count * rec;
            if (cur < 0 || pay + need + 16 * ((int64_t)rows + 1) > s->slab_bytes) {
                if (need + 16 > s->slab_bytes) throw FormatError{"a row holds more records than a slab"};
                next_slab();
            }
            memcpy(m + pay, p, (size_t)need);
            mst_hic_row e{(uint32_t)pay, (int32_t)y, x_off, (uint32_t)count | flags};
            memcpy(m + s->slab_bytes - 16 * ((int64_t)rows + 1), &e, 16);
            pay += need + (need & 1);                 // (rec is even for every layout; kept even for the 16-bit loads)
            ++rows;
        }

        // header + rows of one inflated block (the walk of decode_records, without touching a record): row(p, count, rec, y, x_off, flags)
        template <class Row>
        void walk_block(const uint8_t *data, size_t n, Row row) {
            Cursor c(data, n);
            if (c.get<int32_t>() < 0) throw FormatError{"negative record count in a block"};
            const int32_t x_off = c.get<int32_t>();
            const int32_t y_off = c.get<int32_t>();
            const bool short_counts = c.get<uint8_t>() == 0;
            bool short_x = true, short_y = true;
            if (s->h->version > 8) {
                short_x = c.get<uint8_t>() == 0;
                short_y = c.get<uint8_t>() == 0;
            }
            const uint8_t type = c.get<uint8_t>();
            const uint32_t fc = short_counts ? MST_HIC_ROW_SHORT_COUNTS : 0u;
            if (type == 1) {
                const int64_t rec = (short_x ? 2 : 4) + (short_counts ? 2 : 4);
                const int32_t n_rows = short_y ? (int32_t)c.get<int16_t>() : c.get<int32_t>();
                for (int32_t r = 0; r < n_rows; ++r) {
                    const int32_t y = short_y ? (int32_t)c.get<int16_t>() : c.get<int32_t>();
                    int32_t cols = short_x ? (int32_t)c.get<int16_t>() : c.get<int32_t>();
                    if (cols < 0) cols = 0;                           // the decoder's loop runs zero times as well
                    const uint8_t *p = c.p;
                    c.skip((uint64_t)cols * (uint64_t)rec);
                    if (cols > 0) row(p, (int64_t)cols, rec, (int64_t)y_off + y, x_off, fc | (short_x ? 0u : MST_HIC_ROW_INT_COLUMNS));
                }
            } else if (type == 2) {
                const int32_t n_pts = c.get<int32_t>();
                const int32_t wd = (int32_t)c.get<int16_t>();
                if (wd <= 0) throw FormatError{"dense block of width 0"};
                const int64_t rec = short_counts ? 2 : 4;
                for (int64_t i = 0; i < n_pts; i += wd) {
                    const int64_t cnt = n_pts - i < wd ? n_pts - i : wd;
                    const uint8_t *p = c.p;
                    c.skip((uint64_t)cnt * (uint64_t)rec);
                    row(p, cnt, rec, (int64_t)y_off + i / wd, x_off, fc | MST_HIC_ROW_DENSE);
                }
            } else {
                throw FormatError{"unknown block type"};
            }
        }

        // One block.  The usual case: the zlib stream is inflated STRAIGHT INTO the worker's slab (no staging buffer, no copy) when
        // the room left is at least `ratio` times the compressed size and its rows are then listed where they lie (the block's
        // 14-18 header bytes and 4-8 bytes per row travel along unused).  A block that does not fit what is left opens the next
        // slab; one that does not fit an empty slab goes through the staging buffer and is cut at row boundaries.
        void block(const BlockRef *b) {
            const mst_hic *h = s->h;
            const int64_t slab_bytes = s->slab_bytes;
            const uint8_t *comp = h->map + b->pos;
            const size_t comp_size = (size_t)b->size, past = h->size - (size_t)b->pos - comp_size;
            if (!use_zlib() && past >= mst_inflate::kSlack) {
                for (int attempt = 0; attempt < 2; ++attempt) {
                    if (cur < 0) next_slab();
                    const int64_t at = (pay + 15) / 16 * 16;
                    // the directory grows down from the slab's end: room for this block's rows is kept free (checked after the walk)
                    const int64_t room = slab_bytes - at - 16 * ((int64_t)rows + 1) - (int64_t)mst_inflate::kSlack;
                    if (room >= (int64_t)((double)comp_size * ratio) + 64) {
                        size_t n_out = 0;
                        const int rc = mst_inflate::inflate_zlib(comp, comp_size, m + at, (size_t)room, &n_out);
                        if (rc == mst_inflate::kOk) {
                            const double seen = (double)n_out / (double)(comp_size ? comp_size : 1) * 1.05;
                            if (seen > ratio) ratio = seen;
                            int64_t nrows = 0;
                            walk_block(m + at, n_out, [&](const uint8_t *, int64_t, int64_t, int64_t, int32_t, uint32_t) { ++nrows; });
                            if (at + (int64_t)n_out + 16 * ((int64_t)rows + nrows) <= slab_bytes) {
                                walk_block(m + at, n_out, [&](const uint8_t *p, int64_t count, int64_t, int64_t y, int32_t x_off, uint32_t flags) {
                                    list_row((int64_t)(p - m), count, y, x_off, flags);
                                });
                                pay = at + (int64_t)n_out;
                                pay += pay & 1;
                                return;
                            }
                        } else if (rc != mst_inflate::kOutputFull) {
                            throw FormatError{"zlib inflate failed"};
                        } else if (ratio < 64.0) {
                            ratio *= 2.0;                           // the estimate was too small: remember, and take a fresh slab
                        }
                    }
                    if (rows == 0 && pay == 0) break;               // does not fit an EMPTY slab: staged below
                    next_slab();
                }
            }
            const size_t n_out = inflate_block(h, b, buf, pad);
            walk_block(buf.data(), n_out, [&](const uint8_t *p, int64_t count, int64_t rec, int64_t y, int32_t x_off, uint32_t flags) {
                put_row(p, count, rec, y, x_off, flags);
            });
        }
    };
};

// What the two raw opens differ in; everything else of an open is rawstream_start.
struct RawOpen {
    const char *fn, *v6_hint;                 // the entry point's name and its advice for a version 6 file, for the messages
    bool pair;                                // false: the intra matrix of chrom_a (chrom_b and transposed are null)
    const char *chrom_a, *chrom_b;
    int64_t max_dist_bins;
    int32_t part, n_parts;
    int32_t *transposed;                      // pair only
};

static int rawstream_start(const RawOpen &o, mst_hic *h, int32_t resolution, const char *norm, int32_t n_threads, void *slab_memory,
                           int32_t n_slabs, int64_t slab_bytes, mst_hic_rawstream **out) {
    if (!h || !o.chrom_a || (o.pair && (!o.chrom_b || !o.transposed)) || !out || resolution <= 0 || o.n_parts < 1 || o.part < 0 ||
        o.part >= o.n_parts || !slab_memory || n_slabs < 2 || slab_bytes < 4096 || (slab_bytes & 15) ||
        slab_bytes > ((int64_t)1 << 32) || (reinterpret_cast<uintptr_t>(slab_memory) & 15))
        return fail(MST_IO_E_ARG, "%s: bad argument (slab_bytes: a multiple of 16 in [4096, 2^32]; slab_memory 16-byte aligned)", o.fn);
    *out = nullptr;
    if (h->version < 7) return fail(MST_IO_E_FORMAT, "%s: version %d blocks are plain records, not rows%s", o.fn, h->version, o.v6_hint);
    return guarded([&]() -> int {
        std::unique_ptr<mst_hic_rawstream> s(new mst_hic_rawstream());
        s->h = h;
        const int rc = open_matrix(h, o.chrom_a, o.chrom_b, resolution, norm, o.max_dist_bins, s->matrix, o.fn);
        if (rc != MST_IO_OK) return rc;
        s->blocks_total = (int32_t)s->matrix.todo.size();
        split_todo(s->matrix.todo, o.part, o.n_parts);
        if (o.transposed) *o.transposed = s->matrix.transposed;
        s->base = static_cast<uint8_t *>(slab_memory);
        s->n_slabs = n_slabs;
        s->slab_bytes = slab_bytes;
        s->pay_bytes.assign((size_t)n_slabs, 0);
        s->row_count.assign((size_t)n_slabs, 0);
        s->q.start(s.get(), n_threads, n_slabs);
        *out = s.release();
        return MST_IO_OK;
    });
}

extern "C" int mst_hic_rawstream_open(mst_hic *h, const char *chrom, int32_t resolution, const char *norm, int64_t max_dist_bins,
                                      int32_t n_threads, int32_t part, int32_t n_parts, void *slab_memory, int32_t n_slabs,
                                      int64_t slab_bytes, mst_hic_rawstream **out) {
    const RawOpen o{"mst_hic_rawstream_open", ": use mst_hic_stream_open", false, chrom, nullptr, max_dist_bins, part, n_parts, nullptr};
    return rawstream_start(o, h, resolution, norm, n_threads, slab_memory, n_slabs, slab_bytes, out);
}

// every block of the pair's matrix (no distance limit, one part), rows delivered as for the intra stream
extern "C" int mst_hic_rawstream_open_trans(mst_hic *h, const char *chrom_a, const char *chrom_b, int32_t resolution,
                                            const char *norm, int32_t n_threads, void *slab_memory, int32_t n_slabs,
                                            int64_t slab_bytes, int32_t *transposed, mst_hic_rawstream **out) {
    const RawOpen o{"mst_hic_rawstream_open_trans", " (versions 7-9 are read)", true, chrom_a, chrom_b, -1, 0, 1, transposed};
    return rawstream_start(o, h, resolution, norm, n_threads, slab_memory, n_slabs, slab_bytes, out);
}

extern "C" int mst_hic_rawstream_info_trans(mst_hic_rawstream *s, const double **norm_a, int64_t *count_a, const double **norm_b,
                                            int64_t *count_b, int64_t *length_a_bp, int64_t *length_b_bp) {
    if (!s || !norm_a || !count_a || !norm_b || !count_b || !length_a_bp || !length_b_bp)
        return fail(MST_IO_E_ARG, "mst_hic_rawstream_info_trans: bad argument");
    const Matrix &m = s->matrix;
    *norm_a = m.use_norm ? m.norm_vec.data() : nullptr;
    *count_a = m.use_norm ? (int64_t)m.norm_vec.size() : -1;
    *norm_b = m.use_norm ? m.norm_vec2.data() : nullptr;
    *count_b = m.use_norm ? (int64_t)m.norm_vec2.size() : -1;
    *length_a_bp = m.chrom_length;
    *length_b_bp = m.chrom_length2;
    return MST_IO_OK;
}

extern "C" int mst_hic_rawstream_info(mst_hic_rawstream *s, const double **norm_values, int64_t *norm_count,
                                      int64_t *chrom_length_bp) {
    if (!s || !norm_values || !norm_count || !chrom_length_bp) return fail(MST_IO_E_ARG, "mst_hic_rawstream_info: bad argument");
    *norm_values = s->matrix.use_norm ? s->matrix.norm_vec.data() : nullptr;
    *norm_count = s->matrix.use_norm ? (int64_t)s->matrix.norm_vec.size() : -1;
    *chrom_length_bp = s->matrix.chrom_length;
    return MST_IO_OK;
}

extern "C" int mst_hic_rawstream_next(mst_hic_rawstream *s, int32_t timeout_ms, int32_t *slab, int64_t *payload_bytes,
                                      int32_t *rows) {
    if (!s || !slab || !payload_bytes || !rows) return fail(MST_IO_E_ARG, "mst_hic_rawstream_next: bad argument");
    return s->q.wait_ready(timeout_ms, [&](int32_t i) {
        *slab = i;
        *payload_bytes = s->pay_bytes[(size_t)i];
        *rows = s->row_count[(size_t)i];
    });
}

extern "C" int mst_hic_rawstream_release(mst_hic_rawstream *s, int32_t slab) {
    if (!s || slab < 0 || slab >= s->n_slabs) return fail(MST_IO_E_ARG, "mst_hic_rawstream_release: bad argument");
    s->q.release(slab);
    return MST_IO_OK;
}

extern "C" int mst_hic_rawstream_close(mst_hic_rawstream *s, int64_t *rows_total, int64_t *bytes_total, int32_t *blocks_total,
                                       int32_t *blocks_mine) {
    if (!s) return MST_IO_OK;
    s->q.cancel_and_join();
    const int rc = s->q.failed ? decode_failed(s->q.error.c_str()) : MST_IO_OK;
    if (rows_total) *rows_total = s->rows_total;
    if (bytes_total) *bytes_total = s->bytes_total;
    if (blocks_total) *blocks_total = s->blocks_total;
    if (blocks_mine) *blocks_mine = (int32_t)s->matrix.todo.size();
    delete s;
    return rc;
}
