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
    counters.  OPENS counts the files parsed by this process."""
    OPENS = 0

    def __init__(self, path, zero_based=False, threads=0, chunk_bytes=0):
        from .hicfile import _check
        self._lib, self._h = load(), _P()
        _check(self._lib, self._lib.mst_pairs_open_chunked(os.fsencode(path), int(bool(zero_based)), int(threads), int(chunk_bytes),
                                                           ctypes.byref(self._h)))
        PairsFile.OPENS += 1
        self.path, self.zero_based = path, bool(zero_based)

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


_LOCK = threading.RLock()
_HANDLES = {}                            # absolute path -> PairsFile: a run parses each file once


def pairs_handle(path, zero_based=False):
    """The cached PairsFile of `path` (parsed on first use; parsed again only when the position convention changes)."""
    key = os.path.abspath(str(path))
    with _LOCK:
        h = _HANDLES.get(key)
        if h is None or h.zero_based != bool(zero_based):
            if h is not None:
                h.close()
            h = _HANDLES[key] = PairsFile(key, zero_based)
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
# what the command lines refuse
# ----------------------------------------------------------------------------------------------------------------------
def refusal(files, balance, bias, norm_method, ch, ch2, trans_all, balance_genome, zero_based, world=1, bias_flag="-b"):
    """The text behind `Error:` of a run that its pairs input (or --pairs-zero-based without one) rules out, or None.  Reads
    nothing and touches no GPU.  files: the input path(s); ch / ch2: the -ch / -ch2 lists ('n' when absent)."""
    files = [files] if isinstance(files, str) else list(files)
    mine = [f for f in files if is_pairs(f)]
    if not mine:
        if zero_based:
            return "--pairs-zero-based is for .pairs / .pairs.gz input (%s is none)" % ", ".join(str(f) for f in files)
        return None
    if trans_all:
        return "--trans-all and %s: only intra-chromosomal loops are called from a pairs file" % mine[0]
    if balance_genome is not None:
        return "--balance-genome and %s: only intra-chromosomal loops are called from a pairs file; use --balance" % mine[0]
    if isinstance(ch2, list) and (not isinstance(ch, list) or len(ch) != len(ch2) or any(a != b for a, b in zip(ch, ch2))):
        return "-ch2 with another chromosome and %s: only intra-chromosomal loops are called from a pairs file" % mine[0]
    if balance is None:
        return "%s holds raw read pairs: give --balance ICE|NEWTON" % mine[0]
    from .balance import BalanceError, check_request
    try:
        check_request(balance, files, bias, norm_method, world, bias_flag=bias_flag)
    except BalanceError as e:
        return str(e)
    return None


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
        cap = rows if far_capacity is None else int(far_capacity)
        dense = torch.zeros(K * n, dtype=torch.int32, device=dev)                 # uint32 counters
        far_key = torch.empty(cap, dtype=torch.int64, device=dev)
        far_mult = i32(cap)                                                       # uint32, at most 64
        counters = torch.zeros(2, dtype=torch.int64, device=dev)
        _lib.check(lib.mst_pairs_bin(_ptr(p1), _ptr(p2), rows, res, int(bool(zero_based)), limit, n, K, _ptr(dense) if K else None,
                                     _ptr(far_key) if cap else None, _ptr(far_mult) if cap else None, cap, _ptr(counters), _stream()))
        far_entries, dropped = (int(v) for v in counters.cpu().tolist())
        if far_entries > cap:
            raise _lib.MstOverflow(_lib.MST_E_OVERFLOW, "bin_pairs_device: the far list holds %d entries, %d were needed"
                                   % (cap, far_entries))
        xs, ds, cs = [], [], []
        if K:
            room = min(rows, K * n)
            x, d, c = i32(room), i32(room), i32(room)
            found = torch.zeros(1, dtype=torch.int64, device=dev)
            ws = torch.empty(int(lib.mst_pairs_compact_workspace_bytes(K, n)), dtype=torch.uint8, device=dev)
            _lib.check(lib.mst_pairs_compact(_ptr(dense), K, n, _ptr(x), _ptr(d), _ptr(c), room, _ptr(found), _ptr(ws), ws.numel(),
                                             _stream()))
            m = int(found.item())
            if m > room:
                raise RuntimeError("bin_pairs_device: %d non-zero counters from %d rows" % (m, rows))
            xs.append(x[:m])
            ds.append(d[:m])
            cs.append(c[:m].to(torch.int64) & 0xFFFFFFFF)
            del dense, ws
        if far_entries:
            keys, counts = sum_far_list(far_key[:far_entries], far_mult[:far_entries])
            fx = torch.div(keys, n, rounding_mode="floor")
            xs.append(fx.to(torch.int32))
            ds.append((keys - fx * n - fx).to(torch.int32))
            cs.append(counts)
        del far_key, far_mult
        if not xs:
            return Pixels(i32(0), i32(0), torch.empty(0, dtype=torch.int64, device=dev), 0, dropped, K, far_entries, n)
        x, d, c = (torch.cat(xs), torch.cat(ds), torch.cat(cs)) if len(xs) > 1 else (xs[0], ds[0], cs[0])
        top = int((x + d).max().item()) + 1 if x.numel() else 0
        return Pixels(x, d, c, top, dropped, K, far_entries, n)


# ----------------------------------------------------------------------------------------------------------------------
# the reader under --balance
# ----------------------------------------------------------------------------------------------------------------------
def read_pairs_balanced(f, distance_in_bp, chromosome, res, device=None, method="ICE", zero_based=False, verbose=True, **kw):
    """A pairs file under --balance: the chromosome's rows binned on the device, then balance.balance_records_device -> (x, y, v)
    host arrays, None when nothing is left."""
    import torch
    from ._lib import require_gpu
    from .balance import balance_records_device
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
    return balance_records_device(px.x, px.dist, px.count.to(torch.float64), distance_in_bp, chromosome, res, dev, method=method, **kw)
