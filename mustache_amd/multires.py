"""Loops at several resolutions from one read: `-r 5kb --coarser 10kb 25kb [--merge-distance M]` of `python -m mustache_amd`.
One chromosome's raw pixel set (pairs.read_pairs_raw or balance.read_hic_raw, thinned once by downsample.thin_records when
`--downsample` is given) is coarsened on the device by each integer factor, every resolution is balanced and called on its own
as a run at that resolution would be, and the loop lists are merged.  csrc/mst_coarsen.hip holds the kernel;
tests/multires_reference.py restates both rules below in NumPy and plain Python.

Coarsening

A record (x, d, c) at resolution r -- the pixel (x, x + d) with the raw count c, an integer in [0, 2^32 - 1] -- goes, with the
factor k = R / r, to X = x // k, Y = (x + d) // k, D = Y - X.  The count of a coarse pixel is the integer sum of c over its
records: exact in int64 and independent of the order of the records.  Every record is a contribution: a fine pixel that is
listed twice adds twice (the readers list each pixel once).  A coarse pixel whose counts sum to 0 is no pixel.  Because
floor(floor((p - 1) / r) / k) == floor((p - 1) / (r k)), coarsening the binned read pairs equals binning them at R: the pixel
set is the one a run at R sees, which is why each resolution can be balanced and called as that run would.

A count that is not an integer value in [0, 2^32 - 1] (float `.hic` files exist) ends the run with an `Error:` line naming the
chromosome: one flag word written by the kernel, the thinning's rule.

Coarsening the genome's map (`--trans-all --balance-genome NEWTON -r 50kb --coarser-genome 250kb 500kb`)

A trans record (x, y, c) of the chromosome pair (A, B) at resolution r -- x a bin of A, y a bin of B, c an integer in
[0, 2^32 - 1] held as float64 in balance_genome.GenomeRead.records -- goes, with k = R / r, to X = x // k, Y = y // k.  The
count of a coarse pixel is the integer sum of c over its records, exact in 64-bit integers and independent of their order; a
fine pixel listed twice adds twice; a coarse pixel whose sum is 0 is no pixel.  The layout at R is
balance_genome.genome_layout(lengths, R): n'_c = length_c // R + 1.  A record with a negative bin, or with X >= n'_A or
Y >= n'_B, is dropped and counted -- before its key is formed, so that it aliases no other cell.  For a file whose positions lie
inside the chromosome lengths nothing is dropped (the pairs reader drops rows beyond the length, read_genome filters cis
pixels the same way), and coarsening the r pixels then equals binning the reads at R by the floor identity above; the equality
with a run at R is stated for that case only.  A count that is no integer in [0, 2^32 - 1] counts as 0, sets one flag word and
ends the run with an `Error:` line.  csrc/mst_coarsen_pairs.hip takes the records of many pairs in one launch (coarsen_pairs);
tests/coarsen_genome_reference.py restates the rule.

The cis parts of the genome's map (`--balance-pixels all`): each (c, x, dist, v) part goes through coarsen_records, unchanged;
afterwards D >= balance_genome.IGNORE_DIAGS and X + D < n'_c are kept.  That the fine pixels with dist < 2 were dropped by
read_genome is harmless: D >= 2 implies dist >= k + 1.  Under `inter` there are no cis parts.

The merge below runs per chromosome pair on that pair's lists (x in bins of A, y in bins of B): loops of different pairs
never meet.  The rows of a pair are written as those of a chromosome are, and one line is printed per pair and coarser
resolution:
    multires chr1,chr2: 500000 bp: 3 of 6 loops kept (merge distance 2 bins)

Merge

Take the resolutions r_0 < r_1 < ... and their loop lists L_i, rows [x, y, fdr, sigma] in bins.  The accepted set A starts as
L_0.  For i = 1, 2, ... a loop of L_i at bins (X, Y) is dropped when some a in A, at resolution r_a and bins (x, y), satisfies

    |2 x r_a + r_a - 2 X r_i - r_i| <= 2 M r_i      and      |2 y r_a + r_a - 2 Y r_i - r_i| <= 2 M r_i,

a Chebyshev distance between the pixel centres of at most M bins of the coarser resolution, in integers (twice the centre in
bp).  The survivors of L_i join A only after all of L_i has been judged: loops of one resolution never suppress each other, the
caller's clustering has done that already.  Loops of r_0 are never dropped.  M = `--merge-distance`, 2 by default.  This is the
project's own rule, in the spirit of the two-coarse-bin tolerance usual for such merges.

Per chromosome the rows of r_0 are written in the caller's order, then the survivors of each coarser resolution in ascending
resolution, each in its caller's order; a row's resolution is BIN1_END - BIN1_START.  One line is printed per chromosome and
coarser resolution:
    multires chr1: 10000 bp: 12 of 40 loops kept (merge distance 2 bins)

Host only at import: no torch and no native library until coarsen_records is called.
"""
import numpy as np

MERGE_DISTANCE = 2                       # --merge-distance's default
NOT_RAW = "coarsening sums raw integer counts; give --balance ICE|NEWTON alone"
_COUNT_KIND = {"torch.int64": 0, "torch.float32": 1, "torch.float64": 2}      # MST_THIN_COUNT_*


class MultiresError(ValueError):
    """A multi-resolution request or run that cannot be done (the text of the command line's `Error:` line)."""


def parse_resolutions(res, coarser, flag="--coarser"):
    """-r (bp) and the --coarser (or, by `flag`, --coarser-genome) strings -> the coarser resolutions in bp, ascending;
    MultiresError for a value that does not parse, is not greater than -r, is no integer multiple of -r or is given twice"""
    from .mustache import parseBP
    out = []
    for text in coarser:
        R = parseBP(str(text))
        if not R or R < 1:
            raise MultiresError("%s %s: not a resolution (give base pairs, or a number with kb or mb)" % (flag, text))
        if R <= res:
            raise MultiresError("%s %s: a coarser resolution is greater than -r (%d bp)" % (flag, text, res))
        if R % res:
            raise MultiresError("%s %s: %d bp is not an integer multiple of -r (%d bp)" % (flag, text, R, res))
        if R in out:
            raise MultiresError("%s %s: %d bp is given twice" % (flag, text, R))
        out.append(R)
    return sorted(out)


# ----------------------------------------------------------------------------------------------------------------------
# the merge (host: some 10^4 rows per chromosome)
# ----------------------------------------------------------------------------------------------------------------------
def _centres(loops, r):
    """twice the pixel centres in bp of rows [x, y, ...] at resolution r: (2 x r + r, 2 y r + r) as int64 arrays"""
    n = len(loops)
    x = np.fromiter((int(lp[0]) for lp in loops), dtype=np.int64, count=n)
    y = np.fromiter((int(lp[1]) for lp in loops), dtype=np.int64, count=n)
    return 2 * x * r + r, 2 * y * r + r


def _near_any(ax, ay, cx, cy, reach):
    """for each (cx, cy): is there an (ax, ay) with |ax - cx| <= reach and |ay - cy| <= reach?  ax ascending.  One
    searchsorted per side gives each query its slice of candidates in x; the slices are laid end to end and judged in y."""
    lo = np.searchsorted(ax, cx - reach, side="left")
    hi = np.searchsorted(ax, cx + reach, side="right")
    width = hi - lo
    total = int(width.sum())
    hit = np.zeros(len(cx), dtype=bool)
    if total == 0:
        return hit
    owner = np.repeat(np.arange(len(cx)), width)
    first = np.cumsum(width) - width                     # where each query's slice starts in the concatenation
    at = np.arange(total) - np.repeat(first, width) + np.repeat(lo, width)
    close = np.abs(ay[at] - cy[owner]) <= reach
    hit[owner[close]] = True
    return hit


def merge_loops(lists, resolutions, distance=MERGE_DISTANCE):
    """The merge rule on loop lists (rows [x, y, fdr, sigma], x and y in bins of their list's resolution) at ascending
    resolutions (bp) -> the lists of the kept rows, one per resolution, each in its input order; the first is lists[0] whole.
    All arithmetic is integer arithmetic on twice the centres in bp (int64: exact far beyond any genome)."""
    resolutions = [int(r) for r in resolutions]
    M = int(distance)
    if len(lists) != len(resolutions) or not lists:
        raise ValueError("merge_loops: one loop list per resolution, at least one")
    if M < 0 or any(r < 1 for r in resolutions) or any(b <= a for a, b in zip(resolutions, resolutions[1:])):
        raise ValueError("merge_loops: distance >= 0 and ascending resolutions >= 1")
    kept = [list(lists[0])]
    ax, ay = _centres(kept[0], resolutions[0])
    for loops, r in zip(lists[1:], resolutions[1:]):
        loops = list(loops)
        cx, cy = _centres(loops, r)
        order = np.argsort(ax, kind="stable")
        stay = ~_near_any(ax[order], ay[order], cx, cy, 2 * M * r)
        kept.append([lp for lp, s in zip(loops, stay.tolist()) if s])
        ax, ay = np.concatenate([ax, cx[stay]]), np.concatenate([ay, cy[stay]])
    return kept


def report(chromosome, res, kept, called, distance):
    """the line of one chromosome and coarser resolution"""
    print("multires %s: %d bp: %d of %d loops kept (merge distance %d bins)" % (chromosome, res, kept, called, distance))


# ----------------------------------------------------------------------------------------------------------------------
# the coarsening (device)
# ----------------------------------------------------------------------------------------------------------------------
def coarsen_records(xd, dd, counts, factor, distance_bins=None, device=None, chromosome=None, dense_diags=None, dense_bytes=None,
                    far_capacity=None, library=None, stats=None):
    """The coarsening rule on device records (xd = bin, dd = distance: int32; counts: int64, or float32 / float64 as a `.hic`
    file stores them) -> (x int32, dist int32, count int64) of the coarse pixels with a count above 0: device tensors, order
    unspecified.  factor: k >= 1 (1: the same pixels, summed where one is listed twice).  distance_bins: D of the run at the
    coarse resolution, for K = pairs.dense_diagonals(n', D, budget / 2) -- counters are 8 bytes -- (None: every diagonal is
    wanted dense, budget permitting); dense_bytes: the budget (None: pairs.dense_budget()); dense_diags overrides K itself
    (clamped to n'); far_capacity: room of the far list (None: one entry per record, which always suffices).  chromosome: named
    by the MultiresError of a count that is no integer in [0, 2^32 - 1].  library: another build of the same ABI (the timing
    script's plain build).  stats (a dict) receives "n", "dense_diags", "far_entries" and "total"."""
    import torch
    from . import _lib
    from ._lib import ptr as _ptr, stream as _stream, require_gpu
    from .pairs import dense_budget, dense_diagonals, sum_far_list
    lib = require_gpu() if library is None else library
    dev = counts.device if device is None else torch.device(device)
    k = int(factor)
    if k < 1 or k > 0x7FFFFFFF:
        raise ValueError("coarsen_records: the factor is an integer >= 1")
    kind = _COUNT_KIND.get(str(counts.dtype))
    if kind is None:
        raise TypeError("coarsen_records: counts of dtype %s (int64, float32 or float64 are taken)" % counts.dtype)
    rows = int(counts.numel())
    if int(xd.numel()) != rows or int(dd.numel()) != rows or xd.dtype != torch.int32 or dd.dtype != torch.int32:
        raise ValueError("coarsen_records: x and dist are int32 tensors as long as the counts")
    with torch.cuda.device(dev):
        i32 = lambda m: torch.empty(m, dtype=torch.int32, device=dev)
        i64 = lambda m: torch.empty(m, dtype=torch.int64, device=dev)
        if rows == 0:
            return i32(0), i32(0), i64(0)
        xd, dd, counts = xd.to(dev).contiguous(), dd.to(dev).contiguous(), counts.to(dev).contiguous()
        top = int((xd.to(torch.int64) + dd.to(torch.int64)).max().item())
        if top < 0:
            raise ValueError("coarsen_records: negative bins")
        n = top // k + 1
        if dense_diags is None:
            budget = dense_budget(dev) if dense_bytes is None else int(dense_bytes)
            K = dense_diagonals(n, n if distance_bins is None else distance_bins, budget // 2)
        else:
            K = max(0, min(int(dense_diags), n))
        cap = rows if far_capacity is None else int(far_capacity)
        dense = torch.zeros(K * n, dtype=torch.int64, device=dev)                    # uint64 counters
        far_key, far_count = i64(cap), i64(cap)
        words = torch.zeros(3, dtype=torch.int64, device=dev)
        _lib.check(lib.mst_coarsen_records(_ptr(xd), _ptr(dd), _ptr(counts), kind, rows, k, n, K, _ptr(dense) if K else None,
                                           _ptr(far_key) if cap else None, _ptr(far_count) if cap else None, cap, _ptr(words),
                                           _stream()))
        far_entries, total, bad = (int(v) for v in words.cpu().tolist())
        if bad:
            raise MultiresError("chromosome %s holds a count that is not an integer between 0 and 4294967295: coarsening needs raw "
                                "integer counts" % chromosome)
        if far_entries > cap:
            raise _lib.MstOverflow(_lib.MST_E_OVERFLOW, "coarsen_records: the far list holds %d entries, %d were needed" % (cap, far_entries))
        xs, ds, cs = [], [], []
        if K:
            room = min(rows, K * n)
            found = torch.zeros(1, dtype=torch.int64, device=dev)
            x, d, c = i32(room), i32(room), i64(room)
            ws = torch.empty(int(lib.mst_coarsen_compact_workspace_bytes(K, n)), dtype=torch.uint8, device=dev)
            _lib.check(lib.mst_coarsen_compact(_ptr(dense), K, n, _ptr(x), _ptr(d), _ptr(c), room, _ptr(found), _ptr(ws), ws.numel(),
                                               _stream()))
            m = int(found.item())
            if m > room:
                raise RuntimeError("coarsen_records: %d non-zero counters from %d records" % (m, rows))
            xs.append(x[:m]), ds.append(d[:m]), cs.append(c[:m])
        del dense
        if far_entries:
            keys, sums = sum_far_list(far_key[:far_entries], far_count[:far_entries])
            fx = torch.div(keys, n, rounding_mode="floor")
            xs.append(fx.to(torch.int32)), ds.append((keys - fx * n - fx).to(torch.int32)), cs.append(sums)
        x, d, c = (torch.cat(xs), torch.cat(ds), torch.cat(cs)) if len(xs) > 1 else (xs[0], ds[0], cs[0]) if xs else (i32(0), i32(0), i64(0))
        written = int(c.sum().item()) if c.numel() else 0
        if written != total:
            raise RuntimeError("coarsen_records: %d contacts were read and %d written (a record outside the map?)" % (total, written))
        if stats is not None:
            stats.update(n=n, dense_diags=K, far_entries=far_entries, total=total)
        return x, d, c


def coarsen_pairs(x, y, counts, seg_off, tables, factor, dense_bytes=None, dense_cells=None, far_capacity=None, device=None,
                  stats=None, max_blocks=0, library=None):
    """The genome's coarsening rule on the concatenated device records of P pairs (x, y int32; counts int64, float32 or
    float64; pair p in [seg_off[p], seg_off[p + 1]), seg_off a host int64 array of P + 1) -> {p: (x int32, y int32, v float64)}
    device tensors in key order for every pair that has a record.  tables: pairs.trans_tables(lengths, bins at the COARSE
    resolution)[0] (rows 2, 3, 4 -- nA, nB, cell_off -- are used); factor: k >= 1.  dense_cells: None = every cell when 8 bytes
    per cell fit dense_bytes (None: pairs.dense_budget()), else 0; a value is clamped to the cell total.  far_capacity: room of
    the far list (None: one entry per record, which always suffices; too small raises _lib.MstOverflow).  max_blocks: the most
    workgroups (0: the kernel's default).  library: another build of the same ABI (the timing script's plain build).
    MultiresError for a count that is no integer in [0, 2^32 - 1].  stats (a dict) receives "dense_cells", "far_entries",
    "total" (the contacts written), "outside" (the records dropped) and "pixels"."""
    import torch
    from . import _lib
    from ._lib import ptr as _ptr, stream as _stream, require_gpu
    from .pairs import decode_trans_keys, dense_budget, sum_far_list
    lib = require_gpu() if library is None else library
    dev = counts.device if device is None else torch.device(device)
    k = int(factor)
    if k < 1 or k > 0x7FFFFFFF:
        raise ValueError("coarsen_pairs: the factor is an integer >= 1")
    kind = _COUNT_KIND.get(str(counts.dtype))
    if kind is None:
        raise TypeError("coarsen_pairs: counts of dtype %s (int64, float32 or float64 are taken)" % counts.dtype)
    tables = np.ascontiguousarray(tables, dtype=np.int64)
    seg_off = np.ascontiguousarray(seg_off, dtype=np.int64)
    P, rows = int(tables.shape[1]), int(counts.numel())
    if tables.ndim != 2 or tables.shape[0] != 5 or seg_off.shape != (P + 1,):
        raise ValueError("coarsen_pairs: tables of [5][P] and seg_off of P + 1 entries")
    if int(x.numel()) != rows or int(y.numel()) != rows or x.dtype != torch.int32 or y.dtype != torch.int32:
        raise ValueError("coarsen_pairs: x and y are int32 tensors as long as the counts")
    if P and (int(seg_off[0]) != 0 or int(seg_off[-1]) != rows or np.any(np.diff(seg_off) < 0)):
        raise ValueError("coarsen_pairs: seg_off ascending from 0 to the number of records")
    cells = int((tables[2] * tables[3]).sum())
    if P and (np.any(tables[2:4] < 0) or np.any(tables[4] != np.cumsum(tables[2] * tables[3]) - tables[2] * tables[3])):
        raise ValueError("coarsen_pairs: cell_off is the running sum of nA * nB")
    if stats is not None:
        stats.update(dense_cells=0, far_entries=0, total=0, outside=0, pixels=0)
    if rows == 0 or P == 0:
        return {}
    with torch.cuda.device(dev):
        if dense_cells is None:
            budget = dense_budget(dev) if dense_bytes is None else int(dense_bytes)
            dense_cells = cells if 8 * cells <= budget else 0
        dense_cells = max(0, min(int(dense_cells), cells))
        x, y, counts = x.to(dev).contiguous(), y.to(dev).contiguous(), counts.to(dev).contiguous()
        i64 = lambda m: torch.empty(m, dtype=torch.int64, device=dev)
        table_d = torch.from_numpy(np.concatenate([tables[2], tables[3], tables[4], seg_off])).to(dev)
        cap = rows if far_capacity is None else int(far_capacity)
        dense = torch.zeros(dense_cells, dtype=torch.int64, device=dev)              # uint64 counters
        far_key, far_count = i64(cap), i64(cap)
        words = torch.zeros(4, dtype=torch.int64, device=dev)
        _lib.check(lib.mst_coarsen_pairs(_ptr(x), _ptr(y), _ptr(counts), kind, rows, _ptr(table_d[3 * P:]), _ptr(table_d[:P]),
                                         _ptr(table_d[P:2 * P]), _ptr(table_d[2 * P:3 * P]), P, k, dense_cells,
                                         _ptr(dense) if dense_cells else None, _ptr(far_key) if cap else None,
                                         _ptr(far_count) if cap else None, cap, _ptr(words), int(max_blocks), _stream()))
        far_entries, total, bad, outside = (int(v) for v in words.cpu().tolist())
        if bad:
            raise MultiresError("the genome holds an inter-chromosomal count that is not an integer between 0 and 4294967295: "
                                "coarsening needs raw integer counts")
        if far_entries > cap:
            raise _lib.MstOverflow(_lib.MST_E_OVERFLOW, "coarsen_pairs: the far list holds %d entries, %d were needed" % (cap, far_entries))
        parts = []
        if dense_cells:
            room = min(rows, dense_cells)
            found = torch.zeros(1, dtype=torch.int64, device=dev)
            keys, sums = i64(room), i64(room)
            ws = torch.empty(int(lib.mst_coarsen_pairs_compact_workspace_bytes(dense_cells)), dtype=torch.uint8, device=dev)
            _lib.check(lib.mst_coarsen_pairs_compact(_ptr(dense), dense_cells, _ptr(keys), _ptr(sums), room, _ptr(found), _ptr(ws),
                                                     ws.numel(), _stream()))
            m = int(found.item())
            if m > room:
                raise RuntimeError("coarsen_pairs: %d non-zero counters from %d records" % (m, rows))
            parts.append((keys[:m], sums[:m]))
        del dense
        if far_entries:                              # every far key is >= dense_cells: behind the dense part, ascending
            parts.append(sum_far_list(far_key[:far_entries], far_count[:far_entries]))
        keys, sums = (torch.cat(kc) for kc in zip(*parts)) if len(parts) > 1 else parts[0] if parts else (i64(0), i64(0))
        written = int(sums.sum().item()) if sums.numel() else 0
        if written != total:
            raise RuntimeError("coarsen_pairs: %d contacts were read and %d written" % (total, written))
        if stats is not None:
            stats.update(dense_cells=dense_cells, far_entries=far_entries, total=total, outside=outside, pixels=int(keys.numel()))
        return decode_trans_keys(keys, sums, tables)
