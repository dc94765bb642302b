"""Inter-chromosomal (trans) loop calling for MANY chromosome pairs in shared launches.

The rules are those of mustache_amd/trans.py, pair by pair, and this module is the one host path they run on: a pair alone
(trans.call_trans_coo, `-ch A -ch2 B`) is a batch of one pair (PairBatcher.run_pair).  Every row of a pair is the row of that
pair run alone -- tests/trans_pair_alone.py keeps the independent single-pair form (mst_trans_zscore, mst_trans_scatter_tiles,
no skip rule) the tests compare with.  How the work reaches the GPU:

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
  the group's tiles, finding the windows that hold a record from its coordinates.  Behind the scatter: trans.tile_loops
  (mst_trans_prologue, the sigma loop, the batched tail) and trans.owned_rows.
The batch body (PairBatcher, SampleBatch) is written for S samples per pair: TransGenomeCaller is its one-sample form,
diff_trans_genome.DiffTransGenomeCaller its two-sample form (a pair's dimensions are the maxima over the samples' extents, a tile
is kept when every sample's count reaches the threshold, every sample is scattered into its own tiles of the launch).
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


def default_budget(device, chunk, tiles_per_launch, bytes_per_pixel=9):
    """Bytes of records (RECORD_BYTES each) a run may hold before it flushes them as one batch: what
    pipeline.genome_batch_budget allows, less the tile buffers of one launch (`bytes_per_pixel` of each of its
    `tiles_per_launch` tiles; one sample: 9, c and nz)."""
    from .pipeline import genome_batch_budget
    tile_bytes = int(bytes_per_pixel) * int(tiles_per_launch) * int(chunk) * int(chunk)
    return max(0, genome_batch_budget(device) - tile_bytes)


def joint_dims(per_sample):
    """dims of pair_table from the samples' own: per_sample[s][p] = (n1, n2) of pair p in sample s, or None where rule 2 leaves
    the sample nothing to tile (no record, std = 0, a non-finite mean or std).  Rule 3: a pair is tiled over the maxima of its
    samples' dimensions -- and not at all when one of them is None."""
    dims = []
    for of_pair in zip(*per_sample):
        if any(d is None for d in of_pair):
            dims.append(None)
        else:
            dims.append((max(int(d[0]) for d in of_pair), max(int(d[1]) for d in of_pair)))
    return dims


def joint_counts(counts):
    """the count the skip rule tests per tile: the smallest of the samples' counts (a tile pair is kept only when EVERY
    sample holds TRANS_MIN_TESTED records with v' != 0 in its window)"""
    out = np.asarray(counts[0])
    for c in counts[1:]:
        out = np.minimum(out, np.asarray(c))
    return out


class SampleBatch:
    """One sample's records of the P pairs of a batch: concatenated (x, y, v [N], seg [P + 1]), normalised in place pair by
    pair (mst_trans_zscore_segmented), with every pair's {mean, std, n, flags} (`stats` [P, 4]) and {max x, max y} (`extent`
    [P, 2]) on the host after ONE copy.  `recs[p]` = device (x int32, y int32, v float64) or None, at least one not None; the
    list is emptied as the records are copied.  The batch owns its `v`, which the z-score overwrites; x and y are only read,
    so a batch of one pair adopts them instead of holding the pair's coordinates twice."""

    def __init__(self, lib, dev, recs):
        import torch
        from . import _lib
        self.lib, self.dev = lib, dev
        P = self.P = len(recs)
        self.lens = [0 if r is None else int(r[2].numel()) for r in recs]
        seg = self.seg = np.zeros(P + 1, np.int64)
        np.cumsum(self.lens, out=seg[1:])
        N = self.N = int(seg[-1])
        v = self.v = torch.empty(N, dtype=torch.float64, device=dev)
        if P == 1:
            x, y = self.x, self.y = recs[0][0].contiguous(), recs[0][1].contiguous()
        else:
            x = self.x = torch.empty(N, dtype=torch.int32, device=dev)
            y = self.y = torch.empty(N, dtype=torch.int32, device=dev)
        for p in range(P):                                         # the batch owns its copy; the held tensors go one by one
            if self.lens[p]:
                if P > 1:
                    x[seg[p]:seg[p + 1]].copy_(recs[p][0])
                    y[seg[p]:seg[p + 1]].copy_(recs[p][1])
                v[seg[p]:seg[p + 1]].copy_(recs[p][2])
            recs[p] = None
        self.seg_d = torch.from_numpy(seg).to(dev)
        # stats f64 [4 P] and extent int32 [2 P] in ONE buffer: one copy brings every pair's mean, std, n1 and n2 to the host
        both = torch.empty(40 * P, dtype=torch.uint8, device=dev)
        stats_d, extent_d = both[:32 * P].view(torch.float64), both[32 * P:].view(torch.int32)
        ws_bytes = int(lib.mst_trans_zscore_segmented_workspace_bytes(P))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.mst_trans_zscore_segmented(_ptr(x), _ptr(y), _ptr(v), N, _ptr(self.seg_d), P, _ptr(v), _ptr(stats_d),
                                                      _ptr(extent_d), _ptr(ws), ws_bytes, _stream()))
        host = both.cpu().numpy()
        self.stats = host[:32 * P].view(np.float64).reshape(P, 4)
        self.extent = host[32 * P:].view(np.int32).reshape(P, 2)

    def dims(self):
        """per pair (n1, n2) = (max x + 1, max y + 1), or None (rule 2: no record, a non-finite mean or std, std = 0)"""
        out = []
        for p in range(self.P):
            mean, std = float(self.stats[p, 0]), float(self.stats[p, 1])
            if self.lens[p] == 0 or not (np.isfinite(mean) and np.isfinite(std)) or std == 0:
                out.append(None)
            else:
                out.append((int(self.extent[p, 0]) + 1, int(self.extent[p, 1]) + 1))
        return out

    def count_tiles(self, table_d, T):
        """per tile of the batch's pair table, this sample's records with v' != 0 inside its window (host, uint32 [T])"""
        import torch
        from . import _lib
        counts_d = torch.empty(T, dtype=torch.int32, device=self.dev)
        with torch.cuda.device(self.dev):
            _lib.check(self.lib.mst_trans_count_tiles(_ptr(self.x), _ptr(self.y), _ptr(self.v), self.N, _ptr(self.seg_d),
                                                      _ptr(table_d), self.P, T, _ptr(counts_d), _stream()))
        return counts_d.cpu().numpy().view(np.uint32)

    def scatter(self, table_d, p0, p1, T, slot, B, C, c):
        """this sample's records of the pairs p0 .. p1 into the B tiles `c` of one launch, chosen by slot[t]"""
        from . import _lib
        seg = self.seg
        _lib.check(self.lib.mst_trans_scatter_worklist(_ptr(self.x), _ptr(self.y), _ptr(self.v), _ptr(self.seg_d), _ptr(table_d),
                                                       p0, p1 + 1, int(seg[p1 + 1] - seg[p0]), T, _ptr(slot), B, C, _ptr(c),
                                                       _stream()))


class PairBatcher:
    """What the all-pairs callers of one sample (TransGenomeCaller) and of two (diff_trans_genome.DiffTransGenomeCaller) share:
    pairs held on the device under a byte budget, the flush, batches of one (run_pair: a pair alone, without the budget); per
    batch the samples' segmented z-scores, the joint pair table, the counts and the skip rule, the launch groups and the slot
    table of the work-list scatter.  A subclass says how a launch turns B filled tiles (per sample) into rows: tile_rows,
    owned and the order of a pair's rows."""

    SAMPLES = 1
    UNIT = "tiles"                 # what `stats` and the verbose line count

    def __init__(self, octave_values, emit, chunk=TRANS_CHUNK, tiles_per_launch=None, budget_bytes=None, stats=None,
                 verbose=False):
        from .mustache import _engine
        self.eng = _engine(octave_values)
        self.device = self.eng.device
        self.emit, self.chunk, self.verbose = emit, int(chunk), verbose
        self.tiles_per_launch = tiles_per_launch_of(tiles_per_launch)
        self.budget = budget_bytes
        self.stats = stats if stats is not None else {}
        for k in ("tiles_total", "tiles_skipped", "launches", "batches"):
            self.stats[k] = 0
        self.held, self.held_records = [], 0

    # ---- what a subclass says ---------------------------------------------------------------------------------------------
    def default_budget(self):
        return default_budget(self.device, self.chunk, self.tiles_per_launch)

    def no_contact(self, label):
        raise NotImplementedError

    def tile_rows(self, B, C, fill):
        """per tile of a launch what `owned` takes; fill(s, c) scatters sample s's records into the B tiles c"""
        raise NotImplementedError

    def owned(self, got, tiling, i, j):
        raise NotImplementedError

    def row_order(self, r):
        raise NotImplementedError

    # ---- holding ----------------------------------------------------------------------------------------------------------
    def on_device(self, records):
        """(recs, n): per sample device (x int32, y int32, v float64) -- the caller's own tensors where they already are that
        -- or None for a sample without a record, and the records of all samples"""
        import torch
        dev = self.device
        recs, n = [], 0
        for rec in records:
            k = 0 if rec is None else len(rec[2])
            if k:
                rec = (torch.as_tensor(rec[0]).to(dev, dtype=torch.int32), torch.as_tensor(rec[1]).to(dev, dtype=torch.int32),
                       torch.as_tensor(rec[2]).to(dev, dtype=torch.float64))
            recs.append(rec if k else None)
            n += k
        return recs, n

    def run_pair(self, records, label=""):
        """One pair alone (records as hold() takes them), now, as a batch of one: its rows.  Nothing is held, so no budget is
        asked for (default_budget queries the device's free memory); `label` is printed as given, "" too."""
        return self._run_batch([(0, self.on_device(records)[0], label)], alone=True)[0]

    def hold(self, index, records, label=None):
        """records: per sample (x, y, v) host arrays or device tensors, or None / empty for a sample without a record"""
        recs, n = self.on_device(records)
        if self.budget is None:
            self.budget = self.default_budget()
        over = (self.held_records + n) * RECORD_BYTES > self.budget or self.held_records + n > MAX_BATCH_RECORDS
        if self.held_records and over:
            self.flush()
        self.held.append((index, recs, label))
        self.held_records += n
        if self.held_records * RECORD_BYTES > self.budget:       # over the budget by itself: a batch of one
            self.flush()

    def flush(self):
        held, self.held, self.held_records = self.held, [], 0
        if held:
            for it, rows in zip(held, self._run_batch(held)):
                self.emit(it[0], rows)

    # ---- one batch --------------------------------------------------------------------------------------------------------
    def _run_batch(self, items, alone=False):
        """the rows of every pair of `items` = [(index, recs, label)], in their order; `alone`: the verbose line of a pair"""
        import torch
        lib, dev = self.eng.lib, self.device
        P = len(items)
        out = [[] for _ in range(P)]
        self.stats["batches"] += 1
        # a sample that holds no record of the whole batch leaves no pair to tile: decided before anything is concatenated
        if any(all(it[1][s] is None for it in items) for s in range(self.SAMPLES)):
            for it in items:
                self.no_contact(it[2])
            return out
        samples = []
        for s in range(self.SAMPLES):
            recs = [it[1][s] for it in items]
            for it in items:
                it[1][s] = None
            samples.append(SampleBatch(lib, dev, recs))
        dims = joint_dims([s.dims() for s in samples])
        for p, d in enumerate(dims):
            if d is None:
                self.no_contact(items[p][2])
        table, T = pair_table(dims, self.chunk)
        groups = []
        if T:
            table_d = torch.from_numpy(table.view(np.uint8)).to(dev)
            counts = joint_counts([s.count_tiles(table_d, T) for s in samples])
            groups = launch_groups(table, counts, self.tiles_per_launch)
            kept = sum(len(g[0]) for g in groups)
            self.stats["tiles_total"] += T
            self.stats["tiles_skipped"] += T - kept
            if self.verbose and alone:
                print("Loop calling (trans %s: %d x %d bins, %d %s of %d)..." % (items[0][2], dims[0][0], dims[0][1], T, self.UNIT,
                                                                                 int(table[0]["C"])))
            elif self.verbose:
                print("Loop calling (trans batch: %d pairs, %d records, %d of %d %s in %d launches)..." % (
                    P, sum(s.N for s in samples), kept, T, self.UNIT, len(groups)))
        if groups:
            tile_pair = np.repeat(np.arange(P), table["K1"].astype(np.int64) * table["K2"])
            tilings = {}
            for tiles, C, p0, p1 in groups:
                self._run_group(samples, table, table_d, T, tiles, C, p0, p1, tile_pair, tilings, dims, out)
                self.stats["launches"] += 1
        for rows in out:
            rows.sort(key=self.row_order)
        return out

    def _run_group(self, samples, table, table_d, T, tiles, C, p0, p1, tile_pair, tilings, dims, out):
        """one launch: the tiles of a group, scattered from the work list sample by sample, through tile_rows"""
        import torch
        B = len(tiles)
        slot = np.full(T, -1, np.int32)                            # the work list: tile t of the batch -> its place in the launch
        slot[tiles] = np.arange(B, dtype=np.int32)
        slot = torch.from_numpy(slot).to(self.device)

        def fill(s, c):
            samples[s].scatter(table_d, p0, p1, T, slot, B, C, c)
        got = self.tile_rows(B, C, fill)
        for t, g in zip(tiles, got):
            p = int(tile_pair[t])
            if p not in tilings:
                tilings[p] = trans_tiling(dims[p][0], dims[p][1], self.chunk)
            i, j = divmod(t - int(table[p]["tile_base"]), int(table[p]["K2"]))
            out[p] += self.owned(g, tilings[p], i, j)


class TransGenomeCaller(PairBatcher):
    """add(index, records, label) pair by pair, flush() at the end; `emit(index, loops)` receives every pair's loops in the
    order the pairs were added.  `budget_bytes` bounds the records held (RECORD_BYTES each); the partition into batches
    changes no bit of the output, since every pair is normalised by its own statistics.  run_pair([(x, y, v)], label): one
    pair alone (`emit` may be None)."""

    def __init__(self, octave_values, st, pt, emit, chunk=TRANS_CHUNK, tiles_per_launch=None, budget_bytes=None, stats=None,
                 verbose=False):
        super().__init__(octave_values, emit, chunk, tiles_per_launch, budget_bytes, stats, verbose)
        self.st, self.pt = st, pt

    def add(self, index, records, label=None):
        """records: (x, y, v) host arrays or device tensors, or None / empty for a pair without a record"""
        self.hold(index, [records], label)

    def no_contact(self, label):
        if label is not None:
            print("There is no contact in the chromosome pair %s to work on." % label)

    def tile_rows(self, B, C, fill):
        """trans.tile_loops on the B tiles of one launch"""
        return tile_loops(self.eng, self.device, B, C, lambda c: fill(0, c), self.st, self.pt)

    def owned(self, loops, tiling, i, j):
        return owned_rows(loops, tiling, i, j)

    def row_order(self, r):
        return (int(r[0]), int(r[1]))


def call_trans_genome(pairs, octave_values, st, pt, chunk=TRANS_CHUNK, tiles_per_launch=None, budget_bytes=None, stats=None,
                      verbose=False, labels=None):
    """Loops of every chromosome pair of `pairs` (pairs[p] = (x, y, v) as host arrays or device tensors, None or empty for a
    pair without records): a list with, per pair, [[x, y, fdr, sigma], ...] sorted by (x, y) -- the rows of that pair
    alone.  A pair with no record, a non-finite mean / std or std = 0 yields [] (and, when `labels`
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
