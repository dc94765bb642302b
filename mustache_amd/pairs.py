"""Loops straight from mapped read pairs: a 4DN `.pairs` / `.pairs.gz` file as an input format of both command lines
(`-f x.pairs --balance ICE|NEWTON`, `-f1` / `-f2` of diff_mustache).  The host parses (csrc/pairs_reader.cpp,
include/mustache_io_pairs.h), the device bins (csrc/mst_pairs.hip); tests/pairs_reference.py restates the rule below in NumPy
and plain Python.

The rule

File format: the 4DN pairs format.  A line whose first byte is `#` is a header line.  `#chromsize: NAME LENGTH` lines give the
chromosomes, in that order; `#columns:` names the columns and the reader takes `chr1 pos1 chr2 pos2` by name; without
`#columns:` the four are columns 2 to 5.  Both are honoured in the leading header block (`#` lines and blank lines); a `#` line
further down and a blank line are skipped.  Without a `#chromsize` line the chromosomes are the names in order of first
appearance (chr1 before chr2 of a row) and no upper position limit applies.  Fields are separated by runs of tabs or blanks.
A data line with too few fields, or with a pos1 / pos2 that is not a decimal integer ([+-]?[0-9]+), is an error that names the
line number (1-based) -- never a silent skip.

Which rows are kept: a row is cis when chr1 == chr2 (an exact string compare within the file); `-ch` matches names by is_chr
(the first chromosome of the table that matches).  Trans rows, and cis rows naming a chromosome that is not in the header, are
counted and otherwise ignored.  No pair_type or mapq filtering: that is `pairtools select`'s job, upstream.

Positions and bins: positions are 1-based and bin = (pos - 1) // res (the rule of `cooler cload pairs`);
`--pairs-zero-based` switches to pos // res.  A row with a position below 1 (with the switch: below 0) or above the
chromosome's length (with the switch: >= length) is dropped and counted as out of range; so is a position that does not fit
int32.

Pixels and counts: a pixel is (min(bin1, bin2), max(bin1, bin2)); its count is the number of kept rows that fall into it.
Counts are exact integers (uint32 counters, int64 sums) and are carried to float64 without passing through float32.

What follows: n = max bin + 1 over the kept pixels, as in balance_text and read_hic_balanced; from the pixel set onward the
path is balance.balance_records_device, the second half of a `.hic --balance` read: solve(method, ...) on the device-resident
records, the bias applied on the device as v' = (v / b[x]) / b[y] (a bias that is NaN or below 0.2 counts as +inf), records
kept where v' > 0 and y - x <= distance_in_bp // res.

Verbose output: one line per chromosome with the rows read (of the whole file), the chromosome's rows, the kept rows, the trans
rows (of the whole file), the out-of-range rows and the pixels.

Device work (csrc/mst_pairs.hip): mst_pairs_bin makes one pass over the rows.  Runs of adjacent rows of a wave that share a pixel
are merged first (pairs files are sorted); a pixel within K diagonals adds its run length to a uint32 counter array [K][n] in the
band's diagonal-major layout with one integer atomic, any other pixel appends (x * n + y, multiplicity) to a far list.
K = min(D + 1, n, budget // (4 n)), D = distance_in_bp // res; the budget defaults to a quarter of the device's free memory (a
choice, not a measurement; MUSTACHE_PAIRS_DENSE_BYTES overrides it) and K = 0 is legal: everything then goes through the far
list.  mst_pairs_compact turns the non-zero counters into records; torch sorts the far keys once and the multiplicities of equal
keys are summed from a cumulative sum (no atomics).  Every sum is an integer sum, so the pixel set is the same from run to run
and under any order of the rows; its record order is unspecified (BalanceCSR sorts, the bias does not depend on it).

Host memory is 8 bytes per cis pair for the length of a run: the file is parsed once, whatever -ch says, and the handle is
cached per path (PairsFile.OPENS counts the parses).

Trans rows on request (`--pairs-trans`, PairsFile(..., keep_trans=True); the file must have `#chromsize` lines): a trans row
whose two chromosomes are both in the table is stored as well, 8 bytes of host memory each, pair-major -- (0,1), (0,2), ...,
(1,2), ... in table order -- with the position on the lower table index first, whichever way round the row named them, and in
file order within the pair.  The rule of their binning stands above bin_trans_device; what follows it is
balance_genome.genome_bias (`--balance-genome`), whose second source a pairs file is.  tests/pairs_trans_reference.py restates
this half.
"""
import atexit
import ctypes
import os
import threading

import numpy as np

SUFFIXES = (".pairs", ".pairs.gz")
NO_LIMIT = 1 << 31                      # the `limit` of a chromosome without a `#chromsize` line


class PairsError(ValueError):
    """A request that a pairs file rules out (the text of the command lines' `Error:` line)."""


def is_pairs(path):
    return str(path).endswith(SUFFIXES)


# ----------------------------------------------------------------------------------------------------------------------
# the host reader
# ----------------------------------------------------------------------------------------------------------------------
_P = ctypes.c_void_p
_SIGNATURES = {
    "mst_pairs_open": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_P)]),
    "mst_pairs_open_chunked": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(_P)]),
    "mst_pairs_close": (None, [_P]),
    "mst_pairs_n_chromosomes": (ctypes.c_int32, [_P]),
    "mst_pairs_chromosome": (ctypes.c_int, [_P, ctypes.c_int32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_int64)]),
    "mst_pairs_rows": (ctypes.c_int64, [_P, ctypes.c_int32, ctypes.POINTER(_P), ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64)]),
    "mst_pairs_counters": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int64)]),
    "mst_pairs_open_ex": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                                         ctypes.POINTER(_P)]),
    "mst_pairs_trans_rows": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(_P), ctypes.POINTER(_P),
                                            ctypes.POINTER(_P), ctypes.POINTER(_P)]),
    "mst_pairs_trans_counters": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int64)]),
}
_bound = None


def exported_symbols():
    return sorted(_SIGNATURES)


def load():
    """libmustache_io.so with the pairs reader bound; a library from before the reader is refused by its missing symbols."""
    global _bound
    if _bound is None:
        from . import hicfile
        lib = hicfile.load()
        missing = [name for name in _SIGNATURES if not hasattr(lib, name)]
        if missing:
            raise ImportError("mustache_amd: %s lacks symbols %s (stale build?)" % (getattr(lib, "_name", "libmustache_io.so"), missing))
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _bound = lib
    return _bound


class PairsFile:
    """One parsed pairs file: the chromosome table, each chromosome's rows (borrowed int32 arrays, valid until close) and the
    counters.  OPENS counts the files parsed by this process.  keep_trans: the trans rows between chromosomes of the table
    are stored as well (trans_rows, trans_counters; 8 bytes of host memory each); the file must have `#chromsize` lines."""
    OPENS = 0

    def __init__(self, path, zero_based=False, threads=0, chunk_bytes=0, keep_trans=False):
        from .hicfile import _check
        self._lib, self._h = load(), _P()
        _check(self._lib, self._lib.mst_pairs_open_ex(os.fsencode(path), int(bool(zero_based)), int(threads), int(chunk_bytes),
                                                      int(bool(keep_trans)), ctypes.byref(self._h)))
        PairsFile.OPENS += 1
        self.path, self.zero_based, self.keep_trans = path, bool(zero_based), bool(keep_trans)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mst_pairs_close(self._h)
            self._h = _P()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def chromosomes(self):
        """[(name, length in bp)] in table order; length -1 when the file has no `#chromsize` line"""
        from .hicfile import _check
        out = []
        for i in range(self._lib.mst_pairs_n_chromosomes(self._h)):
            name, length = ctypes.c_char_p(), ctypes.c_int64()
            _check(self._lib, self._lib.mst_pairs_chromosome(self._h, i, ctypes.byref(name), ctypes.byref(length)))
            out.append((name.value.decode("utf-8", "surrogateescape"), int(length.value)))
        return out

    def index(self, chromosome):
        """the first chromosome of the table that `-ch chromosome` names (is_chr), or None"""
        want = str(chromosome).replace("chr", "")
        for i, (name, _) in enumerate(self.chromosomes()):
            if name.replace("chr", "") == want:
                return i
        return None

    def rows(self, index):
        """(pos1, pos2, out_of_range): int32 views of the handle's arrays (file order) and how many rows are out of range"""
        from .hicfile import _check
        p1, p2, oor = _P(), _P(), ctypes.c_int64()
        n = _check(self._lib, self._lib.mst_pairs_rows(self._h, int(index), ctypes.byref(p1), ctypes.byref(p2), ctypes.byref(oor)))
        if n == 0:
            return np.zeros(0, np.int32), np.zeros(0, np.int32), int(oor.value)
        a = np.ctypeslib.as_array(ctypes.cast(p1, ctypes.POINTER(ctypes.c_int32)), shape=(n,))
        b = np.ctypeslib.as_array(ctypes.cast(p2, ctypes.POINTER(ctypes.c_int32)), shape=(n,))
        return a, b, int(oor.value)

    def counters(self):
        """{"rows", "kept", "trans", "out_of_range", "unknown"} over the whole file"""
        from .hicfile import _check
        c = (ctypes.c_int64 * 5)()
        _check(self._lib, self._lib.mst_pairs_counters(self._h, c))
        return dict(zip(("rows", "kept", "trans", "out_of_range", "unknown"), (int(v) for v in c)))

    def trans_rows(self):
        """(posA, posB, seg_off, out_of_range) of a handle opened with keep_trans: the stored trans rows of the whole file as
        int32 views (valid until close) in pair-major order -- pair p = (a, b), a < b in table order, owns
        [seg_off[p], seg_off[p + 1]), posA on a and posB on b -- with seg_off int64 [P + 1] and the pairs' out-of-range counts
        int64 [P] as copies."""
        from .hicfile import _check
        P, seg, a, b, oor = ctypes.c_int64(), _P(), _P(), _P(), _P()
        _check(self._lib, self._lib.mst_pairs_trans_rows(self._h, ctypes.byref(P), ctypes.byref(seg), ctypes.byref(a), ctypes.byref(b),
                                                         ctypes.byref(oor)))
        P = int(P.value)
        seg_off = np.ctypeslib.as_array(ctypes.cast(seg, ctypes.POINTER(ctypes.c_int64)), shape=(P + 1,)).copy()
        out_of_range = np.ctypeslib.as_array(ctypes.cast(oor, ctypes.POINTER(ctypes.c_int64)), shape=(P,)).copy() if P \
            else np.zeros(0, np.int64)
        n = int(seg_off[-1])
        if n == 0:
            return np.zeros(0, np.int32), np.zeros(0, np.int32), seg_off, out_of_range
        pa = np.ctypeslib.as_array(ctypes.cast(a, ctypes.POINTER(ctypes.c_int32)), shape=(n,))
        pb = np.ctypeslib.as_array(ctypes.cast(b, ctypes.POINTER(ctypes.c_int32)), shape=(n,))
        return pa, pb, seg_off, out_of_range

    def trans_counters(self):
        """{"stored", "out_of_range", "unknown"} of the trans rows of a handle opened with keep_trans: stored + unknown =
        counters()["trans"]"""
        from .hicfile import _check
        c = (ctypes.c_int64 * 3)()
        _check(self._lib, self._lib.mst_pairs_trans_counters(self._h, c))
        return dict(zip(("stored", "out_of_range", "unknown"), (int(v) for v in c)))


_LOCK = threading.RLock()
_HANDLES = {}                            # absolute path -> PairsFile: a run parses each file once


WANT_TRANS = set()                       # absolute paths whose first parse keeps the trans rows (--pairs-trans)


def want_trans(path):
    """The command lines' --pairs-trans: the next parse of `path` keeps the trans rows, whoever asks for the handle first."""
    WANT_TRANS.add(os.path.abspath(str(path)))


def pairs_handle(path, zero_based=False, keep_trans=False):
    """The cached PairsFile of `path` (parsed on first use; parsed again only when the position convention changes, or when
    trans rows are wanted of a handle that holds none -- a handle that holds them serves cis requests too)."""
    key = os.path.abspath(str(path))
    with _LOCK:
        h = _HANDLES.get(key)
        if h is None or h.zero_based != bool(zero_based) or (keep_trans and not h.keep_trans):
            keep = bool(keep_trans) or key in WANT_TRANS or (h is not None and h.keep_trans)
            if h is not None:
                h.close()
                del _HANDLES[key]
            h = _HANDLES[key] = PairsFile(key, zero_based, keep_trans=keep)
        return h


def close_pairs_handles():
    """Release every cached handle (8 bytes of host memory per cis pair)."""
    with _LOCK:
        for h in _HANDLES.values():
            h.close()
        _HANDLES.clear()


atexit.register(close_pairs_handles)


def list_chromosomes(path, zero_based=False):
    """The chromosomes a run without -ch calls: every chromosome of the table, in table order."""
    return [name for name, _ in pairs_handle(path, zero_based).chromosomes()]


# ----------------------------------------------------------------------------------------------------------------------
# the device binning
# ----------------------------------------------------------------------------------------------------------------------
class Pixels:
    """bin_pairs_device's result: x, dist (int32) and count (int64) device tensors of the unique pixels (order unspecified);
    n = max bin + 1 over them (0 when there is none); dropped = rows out of range; dense_diags = K; far_entries = entries of
    the far list before they were summed; n_alloc = the bin count the kernels ran with."""

    def __init__(self, x, dist, count, n, dropped, dense_diags, far_entries, n_alloc):
        self.x, self.dist, self.count, self.n = x, dist, count, int(n)
        self.dropped, self.dense_diags, self.far_entries, self.n_alloc = int(dropped), int(dense_diags), int(far_entries), int(n_alloc)

    def __len__(self):
        return int(self.count.numel())


def dense_budget(device):
    """bytes the counter array [K][n] may take: MUSTACHE_PAIRS_DENSE_BYTES, else a quarter of the device's free memory"""
    env = os.environ.get("MUSTACHE_PAIRS_DENSE_BYTES")
    if env is not None:
        return max(0, int(env))
    import torch
    return torch.cuda.mem_get_info(device)[0] // 4


def dense_diagonals(n, distance_bins, budget):
    """K = min(D + 1, n, budget // (4 n))"""
    return int(max(0, min(int(distance_bins) + 1, int(n), int(budget) // (4 * int(n)))))


def sum_far_list(keys, mult):
    """The far list (int64 keys, integer multiplicities; device tensors) -> (unique keys ascending, int64 sums): one torch sort,
    then the sums of equal keys from a cumulative sum -- no atomics."""
    import torch
    keys, order = torch.sort(keys)
    if keys.numel() == 0:
        return keys, mult.to(torch.int64)
    total = torch.cumsum(mult.to(torch.int64)[order], 0)
    last = torch.ones_like(keys, dtype=torch.bool)
    last[:-1] = keys[1:] != keys[:-1]
    ends = total[last]
    counts = ends.clone()
    counts[1:] -= ends[:-1]
    return keys[last], counts


def _bin_and_collect(who, dev, rows, cells, far_capacity, n_words, far_word, launch, compact):
    """What bin_pairs_device and bin_trans_keys (`who`) share around their kernels: `cells` zeroed uint32 counters, a far list
    with room for far_capacity entries (None: one per row, which always suffices) and n_words zeroed int64 words, of which
    word far_word receives the far entries.  launch(dense, far_key, far_mult, cap, words) enqueues the binning;
    compact(dense, room, found) enqueues the compaction into arrays of `room` records that it returns, counts last, with the
    number of non-zero counters in found.  Returns (the words as a host array, the dense records cut to their number with int64
    counts or None, the summed far list (keys ascending, counts) or None).  Two host waits: the words, and found."""
    import torch
    from . import _lib
    cap = rows if far_capacity is None else int(far_capacity)
    dense = torch.zeros(cells, dtype=torch.int32, device=dev)                     # uint32 counters
    far_key = torch.empty(cap, dtype=torch.int64, device=dev)
    far_mult = torch.empty(cap, dtype=torch.int32, device=dev)                    # uint32, at most 64
    words = torch.zeros(n_words, dtype=torch.int64, device=dev)
    launch(dense, far_key, far_mult, cap, words)
    counted = words.cpu().numpy()
    far_entries = int(counted[far_word])
    if far_entries > cap:
        raise _lib.MstOverflow(_lib.MST_E_OVERFLOW, "%s: the far list holds %d entries, %d were needed" % (who, cap, far_entries))
    records = None
    if cells:
        room = min(rows, cells)
        found = torch.zeros(1, dtype=torch.int64, device=dev)
        records = compact(dense, room, found)
        m = int(found.item())
        if m > room:
            raise RuntimeError("%s: %d non-zero counters from %d rows" % (who, m, rows))
        records = tuple(r[:m] for r in records[:-1]) + (records[-1][:m].to(torch.int64) & 0xFFFFFFFF,)
    del dense
    far = sum_far_list(far_key[:far_entries], far_mult[:far_entries]) if far_entries else None
    return counted, records, far


def bin_pairs_device(pos1, pos2, res, zero_based=False, length=None, distance_bins=None, dense_bytes=None, device=None,
                     far_capacity=None, dense_diags=None):
    """Rows (pos1, pos2: int32 host arrays or device tensors) -> Pixels on the device.  length: the chromosome's length in bp
    (None or negative: no upper limit; the bin count then comes from the largest position).  distance_bins = D of the rule
    (None: every diagonal is wanted dense, budget permitting); dense_bytes: the budget (None: dense_budget()); dense_diags
    overrides K itself (clamped to n); far_capacity: room of the far list (None: one entry per row, which always suffices)."""
    import torch
    from . import _lib
    from ._lib import ptr as _ptr, stream as _stream, require_gpu
    lib = require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    res, lo = int(res), (0 if zero_based else 1)
    if res < 1:
        raise ValueError("bin_pairs_device: res must be >= 1")
    with torch.cuda.device(dev):
        as_dev = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))).to(
            device=dev, dtype=torch.int32).contiguous()
        p1, p2 = as_dev(pos1), as_dev(pos2)
        rows = int(p1.numel())
        if int(p2.numel()) != rows:
            raise ValueError("bin_pairs_device: pos1 and pos2 differ in length")
        i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)
        if rows == 0:
            return Pixels(i32(0), i32(0), torch.empty(0, dtype=torch.int64, device=dev), 0, 0, 0, 0, 0)
        if length is None or int(length) < 0:
            limit = NO_LIMIT
            top = max(int(p1.max().item()), int(p2.max().item()))
            n = (top - lo) // res + 1 if top >= lo else 1
        else:
            limit = int(length)
            n = max(1, (limit - 1) // res + 1)
        if dense_diags is None:
            budget = dense_budget(dev) if dense_bytes is None else int(dense_bytes)
            K = dense_diagonals(n, n if distance_bins is None else distance_bins, budget)
        else:
            K = max(0, min(int(dense_diags), n))

        def launch(dense, far_key, far_mult, cap, words):
            _lib.check(lib.mst_pairs_bin(_ptr(p1), _ptr(p2), rows, res, int(bool(zero_based)), limit, n, K, _ptr(dense) if K else None,
                                         _ptr(far_key) if cap else None, _ptr(far_mult) if cap else None, cap, _ptr(words), _stream()))

        def compact(dense, room, found):
            x, d, c = i32(room), i32(room), i32(room)
            ws = torch.empty(int(lib.mst_pairs_compact_workspace_bytes(K, n)), dtype=torch.uint8, device=dev)
            _lib.check(lib.mst_pairs_compact(_ptr(dense), K, n, _ptr(x), _ptr(d), _ptr(c), room, _ptr(found), _ptr(ws), ws.numel(),
                                             _stream()))
            return x, d, c

        counted, near, far = _bin_and_collect("bin_pairs_device", dev, rows, K * n, far_capacity, 2, 0, launch, compact)
        far_entries, dropped = (int(v) for v in counted)
        xs, ds, cs = ([r] for r in near) if near is not None else ([], [], [])
        if far is not None:
            keys, counts = far
            fx = torch.div(keys, n, rounding_mode="floor")
            xs.append(fx.to(torch.int32))
            ds.append((keys - fx * n - fx).to(torch.int32))
            cs.append(counts)
        if not xs:
            return Pixels(i32(0), i32(0), torch.empty(0, dtype=torch.int64, device=dev), 0, dropped, K, far_entries, n)
        x, d, c = (torch.cat(xs), torch.cat(ds), torch.cat(cs)) if len(xs) > 1 else (xs[0], ds[0], cs[0])
        top = int((x + d).max().item()) + 1 if x.numel() else 0
        return Pixels(x, d, c, top, dropped, K, far_entries, n)


# ----------------------------------------------------------------------------------------------------------------------
# the device binning of trans rows: every chromosome pair of the genome in one pass (csrc/mst_pairs_trans.hip)
#
# The rule.  The stored trans rows are pair-major (PairsFile.trans_rows): pair p = (a, b), a < b in table order, with the position
# on a first.  Each side is judged by its own chromosome's range, as a cis position is; x = bin on a, y = bin on b -- no min / max,
# the pair is oriented -- and a row whose bin is >= its chromosome's bin count is dropped as well.  Pair p's pixels live at the
# keys cell_off[p] + x * n_b + y, cell_off = the running sum of n_a * n_b over the pairs before p: keys are unique across pairs
# and ascending keys are pair-major.  A key below dense_cells is counted in a uint32 array, any other goes through the far list;
# counts are exact integers and reach float64 without passing through float32.
# ----------------------------------------------------------------------------------------------------------------------
def pair_list(n_chromosomes):
    """[(a, b)] of the table's pairs in pair-major order: (0,1), (0,2), ..., (1,2), ..."""
    return [(a, b) for a in range(int(n_chromosomes)) for b in range(a + 1, int(n_chromosomes))]


def trans_tables(lengths, bins):
    """int64 host arrays [5][P] -- limA, limB, nA, nB, cell_off -- and the cell total, for chromosome lengths (negative: no
    upper limit) and bin counts in table order"""
    pairs = pair_list(len(bins))
    t = np.zeros((5, len(pairs)), np.int64)
    total = 0
    for p, (a, b) in enumerate(pairs):
        la, lb = int(lengths[a]), int(lengths[b])
        t[:, p] = (NO_LIMIT if la < 0 else la, NO_LIMIT if lb < 0 else lb, int(bins[a]), int(bins[b]), total)
        total += int(bins[a]) * int(bins[b])
    return t, total


def bin_trans_keys(posA, posB, seg_off, tables, res, zero_based=False, dense_cells=0, far_capacity=None, device=None):
    """mst_pairs_bin_trans, mst_pairs_trans_compact and the far list's sort and sum: pair-major rows (posA, posB: int32 host
    arrays or device tensors; seg_off: int64 [P + 1]) and the per-pair tables (int64 [5][P]: limA, limB, nA, nB, cell_off) ->
    (keys int64 ascending and unique, counts int64, dropped int64 host array [P], far entries before they were summed).
    dense_cells: keys below it are counted in a uint32 array of that many counters.  far_capacity: room of the far list
    (None: one entry per row, which always suffices)."""
    import torch
    from . import _lib
    from ._lib import ptr as _ptr, stream as _stream, require_gpu
    lib = require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    res = int(res)
    if res < 1:
        raise ValueError("bin_trans_keys: res must be >= 1")
    tables = np.ascontiguousarray(tables, dtype=np.int64)
    P = int(tables.shape[1])
    seg_off = np.ascontiguousarray(seg_off, dtype=np.int64)
    if tables.shape[0] != 5 or seg_off.shape != (P + 1,):
        raise ValueError("bin_trans_keys: tables of [5][P] and seg_off of P + 1 entries")
    with torch.cuda.device(dev):
        as_dev = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))).to(
            device=dev, dtype=torch.int32).contiguous()
        pa, pb = as_dev(posA), as_dev(posB)
        rows = int(pa.numel())
        if int(pb.numel()) != rows or (P and (int(seg_off[0]) != 0 or int(seg_off[-1]) != rows or np.any(np.diff(seg_off) < 0))):
            raise ValueError("bin_trans_keys: posA and posB of seg_off[P] rows, seg_off ascending from 0")
        i64 = lambda k: torch.empty(k, dtype=torch.int64, device=dev)
        if rows == 0 or P == 0:
            return i64(0), i64(0), np.zeros(P, np.int64), 0
        dense_cells = max(0, int(dense_cells))
        table_d = torch.from_numpy(np.concatenate([tables.reshape(-1), seg_off])).to(dev)
        lim_a, lim_b, n_a, n_b, cell_off = (table_d[k * P:(k + 1) * P] for k in range(5))

        def launch(dense, far_key, far_mult, cap, words):               # words: [P] dropped rows, then the far entries
            _lib.check(lib.mst_pairs_bin_trans(_ptr(pa), _ptr(pb), rows, _ptr(table_d[5 * P:]), P, _ptr(lim_a), _ptr(lim_b), _ptr(n_a),
                                               _ptr(n_b), _ptr(cell_off), res, int(bool(zero_based)), dense_cells,
                                               _ptr(dense) if dense_cells else None, _ptr(far_key) if cap else None,
                                               _ptr(far_mult) if cap else None, cap, _ptr(words[P:]), _ptr(words), _stream()))

        def compact(dense, room, found):
            k, c = i64(room), torch.empty(room, dtype=torch.int32, device=dev)
            ws = torch.empty(int(lib.mst_pairs_trans_compact_workspace_bytes(dense_cells)), dtype=torch.uint8, device=dev)
            _lib.check(lib.mst_pairs_trans_compact(_ptr(dense), dense_cells, _ptr(k), _ptr(c), room, _ptr(found), _ptr(ws), ws.numel(),
                                                   _stream()))
            return k, c

        counted, near, far = _bin_and_collect("bin_trans_keys", dev, rows, dense_cells, far_capacity, P + 1, P, launch, compact)
        # every far key is >= dense_cells: behind the dense part, already ascending
        parts = [part for part in (near, far) if part is not None]
        if not parts:
            return i64(0), i64(0), counted[:P].copy(), int(counted[P])
        keys, counts = (torch.cat(kc) for kc in zip(*parts)) if len(parts) > 1 else parts[0]
        return keys, counts, counted[:P].copy(), int(counted[P])


def decode_trans_keys(keys, counts, tables):
    """mst_pairs_trans_decode: ascending unique keys and int64 counts (device tensors) -> {p: (x int32, y int32, v float64)}
    device tensors in key order for every pair p of `tables` that has a record"""
    import torch
    from . import _lib
    from ._lib import ptr as _ptr, stream as _stream, require_gpu
    lib = require_gpu()
    tables = np.ascontiguousarray(tables, dtype=np.int64)
    P, n, dev = int(tables.shape[1]), int(keys.numel()), keys.device
    if n == 0 or P == 0:
        return {}
    with torch.cuda.device(dev):
        keys, counts = keys.contiguous(), counts.to(torch.int64).contiguous()
        table_d = torch.from_numpy(np.concatenate([tables[4], tables[3]])).to(dev)
        x, y = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        v = torch.empty(n, dtype=torch.float64, device=dev)
        _lib.check(lib.mst_pairs_trans_decode(_ptr(keys), _ptr(counts), n, _ptr(table_d[:P]), _ptr(table_d[P:]), P, _ptr(x), _ptr(y),
                                              _ptr(v), _stream()))
        cuts = torch.searchsorted(keys, table_d[:P]).cpu().tolist() + [n]
    return {p: (x[cuts[p]:cuts[p + 1]], y[cuts[p]:cuts[p + 1]], v[cuts[p]:cuts[p + 1]]) for p in range(P) if cuts[p + 1] > cuts[p]}


def bin_trans_device(posA, posB, seg_off, lengths, res, zero_based=False, bins=None, out_of_range=None, dense_bytes=None,
                     dense_cells=None, far_capacity=None, device=None, names=None, stats=None):
    """The stored trans rows of a genome (PairsFile.trans_rows: posA, posB, seg_off) -> {(i, j): (x, y, v)}, i < j table indices,
    x = bins of i (int32), y = bins of j (int32), v = counts (float64) as device tensors in key order; pairs without a record
    are absent.  lengths: the table's chromosome lengths in bp; bins: the bin count of each chromosome (None: length // res + 1,
    balance_genome.genome_layout's).  dense_cells: None = every cell when 4 bytes per cell fit dense_bytes (None:
    dense_budget()), else 0.  out_of_range: the reader's per-pair counts; a pair whose device-dropped count differs raises.
    stats (a dict) receives "pixels", "pairs", "dropped", "dense_cells" and "far_entries"."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    bins = [int(length) // int(res) + 1 for length in lengths] if bins is None else [int(b) for b in bins]
    tables, cells = trans_tables(lengths, bins)
    pairs = pair_list(len(bins))
    if dense_cells is None:
        budget = dense_budget(dev) if dense_bytes is None else int(dense_bytes)
        dense_cells = cells if 4 * cells <= budget else 0
    dense_cells = max(0, min(int(dense_cells), cells))
    keys, counts, dropped, far_entries = bin_trans_keys(posA, posB, seg_off, tables, res, zero_based, dense_cells, far_capacity, dev)
    if out_of_range is not None:
        for p in np.flatnonzero(dropped != np.asarray(out_of_range, np.int64)):
            a, b = pairs[int(p)]
            label = "%s,%s" % (names[a], names[b]) if names else "(%d, %d)" % (a, b)
            raise RuntimeError("pairs: the device dropped %d trans rows of the pair %s as out of range, the host reader counted %d"
                               % (dropped[p], label, out_of_range[p]))
    got = decode_trans_keys(keys, counts, tables)
    if stats is not None:
        stats.update(pixels=int(keys.numel()), pairs=len(got), dropped=int(dropped.sum()), dense_cells=dense_cells,
                     far_entries=far_entries)
    return {pairs[p]: rec for p, rec in got.items()}


# ----------------------------------------------------------------------------------------------------------------------
# the reader under --balance
# ----------------------------------------------------------------------------------------------------------------------
def read_pairs_balanced(f, distance_in_bp, chromosome, res, device=None, method="ICE", zero_based=False, verbose=True, **kw):
    """A pairs file under --balance: the chromosome's rows binned on the device (read_pairs_raw), then
    balance.balance_records_device -> (x, y, v) host arrays, None when nothing is left."""
    import torch
    from .balance import balance_records_device
    raw = read_pairs_raw(f, distance_in_bp, chromosome, res, device=device, method=method, zero_based=zero_based, verbose=verbose)
    if raw is None:
        return None
    xd, dd, counts, dev, _ = raw
    return balance_records_device(xd, dd, counts.to(torch.float64), distance_in_bp, chromosome, res, dev, method=method, **kw)


def read_pairs_raw(f, distance_in_bp, chromosome, res, device=None, method="ICE", zero_based=False, verbose=True):
    """The first half of read_pairs_balanced, the raw pixel set on the device: -> (x int32, dist int32, count int64, device,
    kept rows by the host reader's counters), None when the chromosome has no pixel."""
    import torch
    from ._lib import require_gpu
    require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with _LOCK:
        h = pairs_handle(f, zero_based)
        i = h.index(chromosome)
        if i is None:
            raise NameError('wrong chromosome name!')
        name, length = h.chromosomes()[i]
        p1, p2, out_of_range = h.rows(i)
        totals = h.counters()
        print("reading %s through the native pairs reader, raw read pairs for %s balancing" % (os.path.basename(str(f)), str(method).upper()))
        with torch.cuda.device(dev):                 # the upload reads the handle's arrays: under the lock, like the parse
            d1, d2 = torch.from_numpy(p1).to(dev), torch.from_numpy(p2).to(dev)
    px = bin_pairs_device(d1, d2, res, zero_based=zero_based, length=length, distance_bins=int(distance_in_bp // res), device=dev)
    del d1, d2
    if px.dropped != out_of_range:
        raise RuntimeError("pairs: the device dropped %d rows of %s as out of range, the host reader counted %d"
                           % (px.dropped, name, out_of_range))
    if verbose:
        print("pairs %s: %d rows read, %d of chromosome %s, %d kept, %d trans, %d out of range, %d pixels"
              % (os.path.basename(str(f)), totals["rows"], len(p1), name, len(p1) - out_of_range, totals["trans"], out_of_range, len(px)))
    if len(px) == 0:
        print(f'There is no contact in chrmosome {chromosome} to work on.')
        return None
    return px.x, px.dist, px.count, dev, len(p1) - out_of_range
