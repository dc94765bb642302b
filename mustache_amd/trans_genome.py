"""Inter-chromosomal (trans) loop calling for MANY chromosome pairs in shared launches.

The rules are those of mustache_amd/trans.py, pair by pair; every row this module returns for a pair equals the row
call_trans_coo returns for that pair alone.  What changes is how the work reaches the GPU:

* Pairs are held on the device until their records reach a budget, then go through as one batch: their records are
  concatenated, ONE segmented z-score (mst_trans_zscore_segmented) normalises every pair by its own mean and std -- bit for bit
  mst_trans_zscore of the pair alone -- and returns every pair's extent with the statistics in one copy to the host.
* The host builds the pair table (per pair C, K1 x K2 windows, the index of its first tile; tiles are numbered pair-major, then
  row-major) and mst_trans_count_tiles counts, for every tile of the batch, the records with v' != 0 inside its window.
* The skip rule: rule 4 says a tile with fewer than 10 000 tested pixels yields no loops.  A tile's tested pixels are its
  distinct pixels with v' != 0, never more than its records with v' != 0, so a tile whose count is below 10 000 yields no
  loops whatever the readers guarantee about duplicates, and is dropped before the scatter.  The rule never drops a tile that
  could report a loop; a tile it keeps still meets rule 4 in the tail.
* The kept tiles, in pair-major order, are cut into launch groups: runs of up to `tiles_per_launch` tiles of equal C.  A
  group's pairs are a contiguous range, so its records are one range of the batch; mst_trans_scatter_worklist writes them into
  the group's tiles, finding the windows that hold a record from its coordinates.  Everything after the scatter is the code
  TransCaller.run_tiles runs too: trans.tile_loops (mst_trans_prologue, the sigma loop, the batched tail) and trans.owned_rows.
"""
import numpy as np

from ._lib import ptr as _ptr, stream as _stream
from .trans import TRANS_CHUNK, TRANS_OVERLAP, owned_rows, tile_loops, tiles_per_launch_of, trans_tiling, window_start  # noqa: F401

TRANS_MIN_TESTED = 10000          # rule 4's second threshold: below it a tile yields no loops
RECORD_BYTES = 20                 # x int32, y int32, v float64 + its normalised value (in place): what a held record costs
MAX_BATCH_RECORDS = (1 << 31) - 1

# include/mustache_hip.h: mst_trans_pair
PAIR_DTYPE = np.dtype([("C", "<i4"), ("K1", "<i4"), ("K2", "<i4"), ("n1", "<i4"), ("n2", "<i4"), ("reserved", "<i4"),
                       ("tile_base", "<i8")])


def pair_table(dims, chunk=TRANS_CHUNK):
    """(table, T): the mst_trans_pair array of a batch and its tile count.  dims[p] = (n1, n2) of pair p, or None for a pair
    that is not tiled (no record, std = 0 or not finite): K1 = K2 = 0, no tile."""
    table = np.zeros(len(dims), dtype=PAIR_DTYPE)
    base = 0
    for p, d in enumerate(dims):
        table[p]["tile_base"] = base
        if d is None:
            continue
        n1, n2 = int(d[0]), int(d[1])
        C, (rs, _), (cs, _) = trans_tiling(n1, n2, chunk)         # refuses windows that cannot overlap by 256
        K1, K2 = len(rs), len(cs)
        table[p] = (C, K1, K2, n1, n2, 0, base)
        base += K1 * K2
    return table, base


def windows_holding(a, n, C, K):
    """The windows of an axis (length n, K windows of C) that hold coordinate a, as the kernels derive them: the regular range
    ceil((a - C + 1) / (C - 256)) .. floor(a / (C - 256)) clipped to [0, K - 2], then the last window if it holds a."""
    if not 0 <= a < n or K <= 0:
        return []
    out = []
    if K > 1:
        step = C - TRANS_OVERLAP
        lo = max(0, -((C - 1 - a) // step))                       # ceil((a - C + 1) / step)
        hi = min(a // step, K - 2)
        out = list(range(lo, hi + 1))
    if a >= max(0, n - C):
        out.append(K - 1)
    return out


def launch_groups(table, counts, tiles_per_launch, threshold=TRANS_MIN_TESTED):
    """The launches of a batch: [(tiles, C, p0, p1)] with `tiles` a run of up to `tiles_per_launch` consecutive kept tiles
    (counts >= threshold, batch numbering: pair-major) of equal C, from the pairs p0 .. p1 inclusive."""
    groups = []
    cur = None
    for p in range(len(table)):
        C, base, k = int(table[p]["C"]), int(table[p]["tile_base"]), int(table[p]["K1"]) * int(table[p]["K2"])
        for t in range(base, base + k):
            if counts[t] < threshold:
                continue
            if cur is None or cur[1] != C or len(cur[0]) >= tiles_per_launch:
                cur = [[], C, p, p]
                groups.append(cur)
            cur[0].append(t)
            cur[3] = p
    return [tuple(g) for g in groups]


def default_budget(device, chunk, tiles_per_launch):
    """Bytes of records (RECORD_BYTES each) a run may hold before it flushes them as one batch: what
    pipeline.genome_batch_budget allows, less the tile buffers of one launch (9 bytes per pixel: c and nz)."""
    from .pipeline import genome_batch_budget
    tile_bytes = 9 * int(tiles_per_launch) * int(chunk) * int(chunk)
    return max(0, genome_batch_budget(device) - tile_bytes)


class TransGenomeCaller:
    """add(index, records, label) pair by pair, flush() at the end; `emit(index, loops)` receives every pair's loops in the
    order the pairs were added.  `budget_bytes` bounds the records held (RECORD_BYTES each); the partition into batches
    changes no bit of the output, since every pair is normalised by its own statistics."""

    def __init__(self, octave_values, st, pt, emit, chunk=TRANS_CHUNK, tiles_per_launch=None, budget_bytes=None, stats=None,
                 verbose=False):
        from .mustache import _engine
        self.eng = _engine(octave_values)
        self.device = self.eng.device
        self.st, self.pt, self.emit, self.chunk, self.verbose = st, pt, emit, int(chunk), verbose
        self.tiles_per_launch = tiles_per_launch_of(tiles_per_launch)
        self.budget = budget_bytes
        self.stats = stats if stats is not None else {}
        for k in ("tiles_total", "tiles_skipped", "launches", "batches"):
            self.stats[k] = 0
        self.held, self.held_records = [], 0

    def add(self, index, records, label=None):
        """records: (x, y, v) host arrays or device tensors, or None / empty for a pair without a record"""
        import torch
        n = 0 if records is None else len(records[2])
        if n:
            dev = self.device
            x = torch.as_tensor(records[0]).to(dev, dtype=torch.int32)
            y = torch.as_tensor(records[1]).to(dev, dtype=torch.int32)
            v = torch.as_tensor(records[2]).to(dev, dtype=torch.float64)
            item = (index, x, y, v, label)
        else:
            item = (index, None, None, None, label)
        if self.budget is None:
            self.budget = default_budget(self.device, self.chunk, self.tiles_per_launch)
        over = (self.held_records + n) * RECORD_BYTES > self.budget or self.held_records + n > MAX_BATCH_RECORDS
        if self.held_records and over:
            self.flush()
        self.held.append(item)
        self.held_records += n
        if self.held_records * RECORD_BYTES > self.budget:       # over the budget by itself: a batch of one
            self.flush()

    def flush(self):
        held, self.held, self.held_records = self.held, [], 0
        if held:
            self._run_batch(held)

    def _no_contact(self, label):
        if label is not None:
            print("There is no contact in the chromosome pair %s to work on." % label)

    def _run_batch(self, items):
        import torch
        from . import _lib
        lib, dev = self.eng.lib, self.device
        P = len(items)
        lens = [0 if it[1] is None else int(it[3].numel()) for it in items]
        seg = np.zeros(P + 1, np.int64)
        np.cumsum(lens, out=seg[1:])
        N = int(seg[-1])
        out = [[] for _ in range(P)]
        self.stats["batches"] += 1
        if N == 0:
            for p, it in enumerate(items):
                self._no_contact(it[4])
                self.emit(it[0], out[p])
            return
        x = torch.empty(N, dtype=torch.int32, device=dev)
        y = torch.empty(N, dtype=torch.int32, device=dev)
        v = torch.empty(N, dtype=torch.float64, device=dev)
        for p in range(P):                                         # the batch owns its copy; the held tensors go one by one
            if lens[p]:
                x[seg[p]:seg[p + 1]].copy_(items[p][1])
                y[seg[p]:seg[p + 1]].copy_(items[p][2])
                v[seg[p]:seg[p + 1]].copy_(items[p][3])
                items[p] = (items[p][0], None, None, None, items[p][4])
        seg_d = torch.from_numpy(seg).to(dev)
        # stats f64 [4 P] and extent int32 [2 P] in ONE buffer: one copy brings every pair's mean, std, n1 and n2 to the host
        both = torch.empty(40 * P, dtype=torch.uint8, device=dev)
        stats_d, extent_d = both[:32 * P].view(torch.float64), both[32 * P:].view(torch.int32)
        ws_bytes = int(lib.mst_trans_zscore_segmented_workspace_bytes(P))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.mst_trans_zscore_segmented(_ptr(x), _ptr(y), _ptr(v), N, _ptr(seg_d), P, _ptr(v), _ptr(stats_d),
                                                      _ptr(extent_d), _ptr(ws), ws_bytes, _stream()))
        host = both.cpu().numpy()
        stats = host[:32 * P].view(np.float64).reshape(P, 4)
        extent = host[32 * P:].view(np.int32).reshape(P, 2)
        dims = []
        for p in range(P):
            mean, std = float(stats[p, 0]), float(stats[p, 1])
            if lens[p] == 0 or not (np.isfinite(mean) and np.isfinite(std)) or std == 0:
                self._no_contact(items[p][4])
                dims.append(None)
            else:
                dims.append((int(extent[p, 0]) + 1, int(extent[p, 1]) + 1))
        table, T = pair_table(dims, self.chunk)
        groups = []
        if T:
            table_d = torch.from_numpy(table.view(np.uint8)).to(dev)
            counts_d = torch.empty(T, dtype=torch.int32, device=dev)
            with torch.cuda.device(dev):
                _lib.check(lib.mst_trans_count_tiles(_ptr(x), _ptr(y), _ptr(v), N, _ptr(seg_d), _ptr(table_d), P, T,
                                                     _ptr(counts_d), _stream()))
            counts = counts_d.cpu().numpy().view(np.uint32)
            groups = launch_groups(table, counts, self.tiles_per_launch)
            kept = sum(len(g[0]) for g in groups)
            self.stats["tiles_total"] += T
            self.stats["tiles_skipped"] += T - kept
            if self.verbose:
                print("Loop calling (trans batch: %d pairs, %d records, %d of %d tiles in %d launches)..." % (
                    P, N, kept, T, len(groups)))
        if groups:
            slot = torch.full((T,), -1, dtype=torch.int32, device=dev)
            tile_pair = np.repeat(np.arange(P), table["K1"].astype(np.int64) * table["K2"])
            tilings = {}
            for tiles, C, p0, p1 in groups:
                self._run_group(x, y, v, seg, seg_d, table, table_d, T, slot, tiles, C, p0, p1, tile_pair, tilings, dims, out)
                self.stats["launches"] += 1
        for p, it in enumerate(items):
            out[p].sort(key=lambda r: (int(r[0]), int(r[1])))
            self.emit(it[0], out[p])

    def _run_group(self, x, y, v, seg, seg_d, table, table_d, T, slot, tiles, C, p0, p1, tile_pair, tilings, dims, out):
        """one launch: the tiles of a group through trans.tile_loops, scattered from the work list"""
        import torch
        from . import _lib
        dev, lib = self.device, self.eng.lib
        B = len(tiles)
        idx = torch.as_tensor(np.asarray(tiles, np.int64)).to(dev)
        slot[idx] = torch.arange(B, dtype=torch.int32, device=dev)

        def fill(c):
            _lib.check(lib.mst_trans_scatter_worklist(_ptr(x), _ptr(y), _ptr(v), _ptr(seg_d), _ptr(table_d), p0, p1 + 1,
                                                      int(seg[p1 + 1] - seg[p0]), T, _ptr(slot), B, C, _ptr(c), _stream()))
        loops = tile_loops(self.eng, dev, B, C, fill, self.st, self.pt)
        slot[idx] = -1
        for t, lp in zip(tiles, loops):
            p = int(tile_pair[t])
            if p not in tilings:
                tilings[p] = trans_tiling(dims[p][0], dims[p][1], self.chunk)
            i, j = divmod(t - int(table[p]["tile_base"]), int(table[p]["K2"]))
            out[p] += owned_rows(lp, tilings[p], i, j)


def call_trans_genome(pairs, octave_values, st, pt, chunk=TRANS_CHUNK, tiles_per_launch=None, budget_bytes=None, stats=None,
                      verbose=False, labels=None):
    """Loops of every chromosome pair of `pairs` (pairs[p] = (x, y, v) as host arrays or device tensors, None or empty for a
    pair without records): a list with, per pair, [[x, y, fdr, sigma], ...] sorted by (x, y) -- the rows call_trans_coo
    returns for that pair alone.  A pair with no record, a non-finite mean / std or std = 0 yields [] (and, when `labels`
    names the pairs, the "There is no contact ..." line).  `stats`, a dict, receives tiles_total, tiles_skipped, launches and
    batches."""
    pairs = list(pairs)
    result = [None] * len(pairs)

    def emit(i, loops):
        result[i] = loops

    caller = TransGenomeCaller(octave_values, st, pt, emit, chunk=chunk, tiles_per_launch=tiles_per_launch,
                               budget_bytes=budget_bytes, stats=stats, verbose=verbose)
    for i, rec in enumerate(pairs):
        caller.add(i, rec, None if labels is None else labels[i])
    caller.flush()
    return result
