"""Thinning a raw contact map to a chosen depth on the GPU: `--downsample P` and `--seed S` on both command lines,
`--match-depth` on diff_mustache.  It stands between the pixel set and the balancing (pairs.read_pairs_raw or
balance.read_hic_raw, then thin_records, then balance.balance_records_device): both inputs share the device-resident
(x, dist, count) form there, so the thinning is the same for a pairs file and a `.hic` file.  csrc/mst_thin.hip holds the
kernel; tests/downsample_reference.py restates the rule below in NumPy.

The rule

A pixel (x, y), y = x + dist, in absolute bins of chromosome c, with a raw count n -- an integer, 0 <= n <= 2^32 - 1 -- keeps

    k = #{ j in [0, n) : u_j < T },      u_j = word j & 3 of Philox4x32-10(counter = (x, y, j >> 2, tag), key = (seed, sample)).

T is a 32-bit threshold, 0 < T < 2^32: every read is kept with probability exactly T / 2^32, each on its own draw (binomial
thinning).  tag = zlib.crc32 of the chromosome's name with a leading `chr` removed (computed on the host); seed = `--seed`, a
uint32, 0 by default; sample = 0 for the one-sample caller and for -f1, 1 for -f2.  Philox4x32-10 is the published Random123
generator: multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85, 10 rounds.  Integer arithmetic
only: k depends on nothing but (x, y, n, tag, seed, sample, T) -- not on the record order, the launch shape, the input format
or the rank.  Pixels with k = 0 are dropped before the balancing; from then on nothing knows the map was thinned.

`--downsample P`, a float 0 < P < 1: T = int(P * 4294967296), which is exact in double precision; T = 0 is refused.

`--match-depth` works per chromosome: N_k = the sum of sample k's raw cis counts on that chromosome, over all distances, after
the range check and before any filter.  The sample with the smaller N is left alone, the other is thinned with
T = (N_small << 32) // N_large in Python integers; equal depths thin neither.  Per chromosome on purpose: both pixel sets of a
chromosome are on the device before either is balanced, so no pre-pass over a file is needed, and the result does not depend
on which chromosomes a rank owns.

A `.hic` count that is not a non-negative integer value (float `.hic` files exist), or one above 2^32 - 1, ends the run with
an `Error:` line naming the chromosome: one flag word written by the kernel.

One line is printed per thinned chromosome:
    downsample chr1 (sample 1): 1234567 of 2469000 contacts kept, p = 0.5, seed 7

The whole genome's map: `--downsample-genome P` on both command lines, `--match-depth-genome` on diff_mustache, both with
`--balance-genome` (mustache_amd/balance_genome.py: the thinning stands between its read phase and its solve phase;
csrc/mst_thin_pairs.hip holds the kernel of the trans records; tests/downsample_genome_reference.py restates the rule).

Which pixels: the ones `--balance-genome` handles.  Under `--balance-pixels all` every cis pixel that enters the assembly (inside
its chromosome, j - i >= 2) and every resident trans record of every pair of the file, whichever pairs are called; a trans
record with a bin outside its chromosome is thinned like any other (it still never enters the assembly).  Under `inter` no cis
matrix is read and none is thinned.
A cis pixel of chromosome c draws exactly as above -- counter (x, y, j >> 2, chromosome_tag(c)), key (seed, sample) -- and so
keeps the k a `--downsample` run at the same T and seed gives it.
A trans pixel of the pair {A, B}: strip a leading `chr` from both names; the FIRST chromosome is the one whose stripped name is
smaller as UTF-8 bytes.  Counter (bin on first, bin on second, j >> 2, tag), tag = zlib.crc32(first + b"\t" + second); key
(seed, sample + 2).  The key words 2 and 3 keep every trans stream apart from every cis stream, whatever the tags; the
orientation comes from the names, not from the file's chromosome order or from how a record is stored: k depends on (pair,
pixel, n, seed, sample, T) alone.  Two chromosomes of one file whose stripped names are equal raise a DownsampleError.
k, the flag and the dropping are as above: pixels and records with k = 0 are dropped before the assembly, GenomeBias.records
holds the thinned records, and the balancing, the z-score and the caller see those.
Depth: N_k = the integer sum (from the kernels) of the raw counts of everything listed under "which pixels" for sample k.
`--downsample-genome P`: T = threshold_of(P) for every pixel of the genome.  `--match-depth-genome`: (T_1, T_2) =
match_depth(N_1, N_2) -- ONE T for the whole deeper sample, equal depths thin neither.  A single genome-wide probability is what
sequencing less deeply does; per-pair probabilities would change the cis / trans ratio, which the bias sees.

One line is printed per thinned sample:
    downsample genome (sample 1): 41960 of 84139 contacts kept (cis 11396 of 23074, trans 30564 of 61065), p = 0.5, seed 7

Host only at import: no torch and no native library until a function that needs the GPU is called.
"""
import zlib

HEAVY = 256                              # MST_THIN_HEAVY of include/mustache_hip.h: the count from which a whole wave thins a pixel
TWO32 = 1 << 32
_COUNT_KIND = {"torch.int64": 0, "torch.float32": 1, "torch.float64": 2}      # MST_THIN_COUNT_*


class DownsampleError(ValueError):
    """A thinning that cannot be done (the text of the command lines' `Error:` line)."""


def error_line(main):
    """A command line's main() with the `Error:` line of a thinning that failed while it ran: a `.hic` file whose counts are
    no integers is found out when the kernel reads them."""
    import functools

    @functools.wraps(main)
    def run(argv=None):
        try:
            return main(argv)
        except DownsampleError as e:
            print("Error: %s" % e)
    return run


def chromosome_tag(chromosome):
    """zlib.crc32 of the chromosome's name with a leading `chr` removed"""
    name = str(chromosome)
    return zlib.crc32((name[3:] if name.startswith("chr") else name).encode("utf-8")) & 0xFFFFFFFF


def _stripped(chromosome):
    name = str(chromosome)
    return (name[3:] if name.startswith("chr") else name).encode("utf-8")


def pair_tag(a, b):
    """The trans stream of the pair {a, b} -> (tag, swap): tag = zlib.crc32(first + b"\\t" + second), the two names with a
    leading `chr` removed and the one that is smaller as UTF-8 bytes first; swap = 1 when that is b, so that of records
    (x = bin on a, y = bin on b) the y leads the counter.  DownsampleError when the stripped names are equal."""
    sa, sb = _stripped(a), _stripped(b)
    if sa == sb:
        raise DownsampleError("chromosomes %s and %s bear the same name once a leading `chr` is removed: their "
                              "inter-chromosomal pixels cannot be told apart" % (a, b))
    first, second = (sa, sb) if sa < sb else (sb, sa)
    return zlib.crc32(first + b"\t" + second) & 0xFFFFFFFF, int(sb < sa)


def threshold_of(p, flag="--downsample"):
    """--downsample P (or `flag` P) -> T = int(P * 2^32); DownsampleError unless 0 < P < 1 and T > 0"""
    p = float(p)
    if not 0.0 < p < 1.0:
        raise DownsampleError("%s %r: the fraction to keep must lie strictly between 0 and 1" % (flag, p))
    T = int(p * 4294967296.0)
    if T < 1:
        raise DownsampleError("%s %r: the fraction is below 2^-32, nothing would be kept" % (flag, p))
    return T


def match_threshold(n_small, n_large):
    """the T that thins a sample of n_large contacts to n_small of them on average: (n_small << 32) // n_large"""
    n_small, n_large = int(n_small), int(n_large)
    if not 0 <= n_small < n_large:
        raise ValueError("match_threshold: 0 <= n_small < n_large")
    return (n_small << 32) // n_large


def match_depth(n1, n2):
    """--match-depth on depths (N_1, N_2) -> (T_1, T_2): None for the sample that is left alone (both when N_1 = N_2)"""
    n1, n2 = int(n1), int(n2)
    if n1 == n2:
        return None, None
    return (None, match_threshold(n1, n2)) if n1 < n2 else (match_threshold(n2, n1), None)


def check_seed(seed):
    """--seed -> the uint32; DownsampleError outside [0, 2^32 - 1]"""
    seed = int(seed)
    if not 0 <= seed < TWO32:
        raise DownsampleError("--seed %d: the seed is a 32-bit unsigned integer (0 .. 4294967295)" % seed)
    return seed


def _launch(xd, dd, counts, chromosome, T, seed, sample, device, draw):
    """mst_thin_counts on device records -> (k int64 tensor or None, the words as a host list)"""
    import torch
    from . import _lib
    from ._lib import ptr as _ptr, stream as _stream, require_gpu
    lib = require_gpu()
    dev = counts.device if device is None else torch.device(device)
    kind = _COUNT_KIND.get(str(counts.dtype))
    if kind is None:
        raise TypeError("downsample: counts of dtype %s (int64, float32 or float64 are taken)" % counts.dtype)
    n = int(counts.numel())
    if int(xd.numel()) != n or int(dd.numel()) != n or xd.dtype != torch.int32 or dd.dtype != torch.int32:
        raise ValueError("downsample: x and dist are int32 tensors as long as the counts")
    with torch.cuda.device(dev):
        xd, dd, counts = xd.contiguous(), dd.contiguous(), counts.contiguous()
        words = torch.zeros(3, dtype=torch.int64, device=dev)
        k = torch.empty(n, dtype=torch.int64, device=dev) if draw else None
        _lib.check(lib.mst_thin_counts(_ptr(xd), _ptr(dd), _ptr(counts), kind, n, chromosome_tag(chromosome), int(seed), int(sample),
                                       int(T), _ptr(k), _ptr(words), _stream()))
        total, kept, bad = (int(v) for v in words.cpu().tolist())
    if bad:
        raise DownsampleError("chromosome %s holds a count that is not an integer between 0 and 4294967295: thinning needs raw "
                              "integer counts" % chromosome)
    return k, total, kept


def depth_of(xd, dd, counts, chromosome, device=None):
    """N of the rule: the sum of the raw counts of device records, by the kernel's integer sum (nothing is drawn);
    DownsampleError when a count is no integer in [0, 2^32 - 1]"""
    return _launch(xd, dd, counts, chromosome, 0, 0, 0, device, draw=False)[1]


def thin_records(xd, dd, counts, chromosome, T, seed=0, sample=0, device=None):
    """The rule on device records (xd = bin, dd = distance: int32; counts: int64, or float32 / float64 as a `.hic` file
    stores them) -> ((xd, dd, counts int64) of the pixels with k > 0, in the order they came, contacts in, contacts kept)."""
    T, seed, sample = int(T), check_seed(seed), int(sample)
    if not 0 < T < TWO32:
        raise DownsampleError("downsample: the threshold T = %d must satisfy 0 < T < 2^32" % T)
    if sample not in (0, 1):
        raise ValueError("downsample: sample is 0 or 1")
    k, total, kept = _launch(xd, dd, counts, chromosome, T, seed, sample, device, draw=True)
    keep = k > 0
    return (xd[keep], dd[keep], k[keep]), total, kept


def report(chromosome, sample, total, kept, T, seed):
    """the line of one thinned chromosome"""
    print("downsample %s (sample %d): %d of %d contacts kept, p = %r, seed %d" % (chromosome, sample + 1, kept, total, T / TWO32, seed))


def launch_pairs(x, y, counts, seg_off, table, seed, key1, T, draw=True, max_blocks=0, device=None):
    """mst_thin_pairs on device records of P pairs (x, y: int32; counts: int64, float32 or float64; seg_off: P + 1 offsets, host
    or device; table: P rows of (tag, swap), host) -> (k int64 tensor or None, [(reads in, reads kept)] per pair as Python
    integers, the bad-count flag).  One launch and one wait, whatever P."""
    import numpy as np
    import torch
    from . import _lib
    from ._lib import ptr as _ptr, stream as _stream, require_gpu
    lib = require_gpu()
    dev = counts.device if device is None else torch.device(device)
    kind = _COUNT_KIND.get(str(counts.dtype))
    if kind is None:
        raise TypeError("downsample: counts of dtype %s (int64, float32 or float64 are taken)" % counts.dtype)
    n = int(counts.numel())
    table = np.ascontiguousarray(np.asarray(table, dtype=np.uint32).reshape(-1, 2))
    P = int(table.shape[0])
    if int(x.numel()) != n or int(y.numel()) != n or x.dtype != torch.int32 or y.dtype != torch.int32:
        raise ValueError("downsample: x and y are int32 tensors as long as the counts")
    with torch.cuda.device(dev):
        if not torch.is_tensor(seg_off):
            seg_off = torch.from_numpy(np.ascontiguousarray(seg_off, dtype=np.int64))
        seg_off = seg_off.to(device=dev, dtype=torch.int64).contiguous()
        if int(seg_off.numel()) != P + 1:
            raise ValueError("downsample: seg_off holds one offset more than there are pairs")
        x, y, counts = x.contiguous(), y.contiguous(), counts.contiguous()
        table_d = torch.from_numpy(table.view(np.int32)).to(dev)
        words = torch.zeros(2 * P + 1, dtype=torch.int64, device=dev)
        k = torch.empty(n, dtype=torch.int64, device=dev) if draw else None
        _lib.check(lib.mst_thin_pairs(_ptr(x), _ptr(y), _ptr(counts), kind, n, _ptr(seg_off), _ptr(table_d), P, int(seed), int(key1),
                                      int(T), _ptr(k), _ptr(words), int(max_blocks), _stream()))
        got = words.cpu().tolist()
    return k, [(int(got[2 * p]), int(got[2 * p + 1])) for p in range(P)], bool(got[2 * P])


BAD_TRANS_COUNT = "the genome holds an inter-chromosomal count that is not an integer between 0 and 4294967295: thinning needs " \
                  "raw integer counts"


def thin_pairs(x, y, counts, seg_off, pairs, T, seed=0, sample=0, device=None, max_blocks=0):
    """The trans rule on the concatenated device records of pairs = [(a, b)] (x = bins of a, y = bins of b; pair p in
    [seg_off[p], seg_off[p + 1])) -> (k int64 per record, [(contacts in, contacts kept)] per pair)."""
    T, seed, sample = int(T), check_seed(seed), int(sample)
    if not 0 < T < TWO32:
        raise DownsampleError("downsample: the threshold T = %d must satisfy 0 < T < 2^32" % T)
    if sample not in (0, 1):
        raise ValueError("downsample: sample is 0 or 1")
    k, totals, bad = launch_pairs(x, y, counts, seg_off, [pair_tag(a, b) for a, b in pairs], seed, sample + 2, T, True, max_blocks, device)
    if bad:
        raise DownsampleError(BAD_TRANS_COUNT)
    return k, totals


def depth_of_pairs(x, y, counts, seg_off, pairs, device=None):
    """the sum-only form of thin_pairs: the contacts of each pair by the kernel's integer sum (nothing is drawn)"""
    _, totals, bad = launch_pairs(x, y, counts, seg_off, [pair_tag(a, b) for a, b in pairs], 0, 0, 0, False, 0, device)
    if bad:
        raise DownsampleError(BAD_TRANS_COUNT)
    return [t[0] for t in totals]


def report_genome(sample, cis, trans, T, seed):
    """the line of one thinned genome; cis, trans = (contacts kept, contacts in)"""
    print("downsample genome (sample %d): %d of %d contacts kept (cis %d of %d, trans %d of %d), p = %r, seed %d"
          % (sample + 1, cis[0] + trans[0], cis[1] + trans[1], cis[0], cis[1], trans[0], trans[1], T / TWO32, seed))
