"""Balancing of the WHOLE GENOME's contact matrix on the GPU, for inter-chromosomal (trans) calling on `.hic` files that carry no
usable normalisation vector, and on `.pairs` / `.pairs.gz` files, which carry none at all (`--pairs-trans`): `--balance-genome ICE|NEWTON` (with `--balance-pixels all|inter`) on the command lines,
genome_bias() / balanced_pair() / balanced_pairs() in Python.  `--balance` balances one chromosome's own map and so says nothing
about a trans pair; the bias a trans pair needs has seen the trans pixels (what Juicer's GW_* / INTER_* vectors are).

The rule (tests/balance_genome_reference.py restates it in NumPy):

Genome.  Every chromosome of the file in file order, as readers.list_chromosomes(f, res) returns them.  It does not depend on
  -ch: the bias is a property of (file, resolution, method, pixels), not of which pairs are called.  Chromosome c has
  n_c = length_c // res + 1 bins and the genome offset off_c = the sum of the n before it; n = sum n_c.  (A bin nothing is
  recorded in is masked and changes nothing else: an appended empty bin adds exact zeros to every sum of the kernels.)
Pixels (`--balance-pixels`).  `all`, the default: every cis and every trans matrix.  `inter`: the trans matrices only; no cis
  matrix is read.  A cis pixel (i, j) of chromosome c, i <= j, is dropped when j - i < 2 (balance.py's ignore_diags = 2) and
  otherwise becomes the genome pixel (off_c + i, off_c + j).  A trans pixel (x of A, y of B) becomes (off_A + x, off_B + y) --
  in the same cell whether the file stores the pair as (A, B) or as (B, A) -- and is NEVER dropped for its genome distance:
  the pixel (last bin of A, first bin of A + 1) is kept.  The distance rule is therefore applied inside a chromosome, before
  the assembly, and the assembled set goes to the solver with ignore_diags = 0.  A record with a bin outside its chromosome
  (x >= n_A or y >= n_B) is dropped.
Steps 2-6 of balance.py run unchanged on the n x n genome matrix: min_nnz, the MAD filter, ICE or NEWTON, kappa
  (balance.solve(method, lo, hi, v, n, ignore_diags=0) on balance.BalanceCSR).
Application.  v' = (v / b[off_A + x]) / b[off_B + y] in float64, with mst_balance_apply_packed's rule for b: a NaN bias or one
  below 0.2 counts as +inf.  A record whose v' is not > 0 is removed before rule 2 (the z-score) of trans.py.  There is no
  float32 rounding: this is deliberately the arithmetic of `-b` / `--balance` (mustache.read_pd), NOT that of
  mst_trans_decode_hic_rows, which rounds count / (norm_x * norm_y) to straw's float32.

Device path.  The host inflate dominates a `.hic` run, so every matrix is read exactly once: a trans pair through
trans.read_hic_trans(f, "NONE", a, b, res), whose device tensors stay resident (GenomeBias.records) and are later called from; a
cis matrix (`all` only) through hicfile.read_intra_packed(..., "NONE", -1, ...), uploaded, turned into genome coordinates and
dropped.  The reader does not expose a matrix's record count before it is read, so the memory check runs after each matrix:
what the records read so far will need (estimate_bytes) against torch.cuda.mem_get_info.  The assembly is plain torch
(BalanceCSR's sort makes the result independent of the record order, so the bias has the same bits whichever way round a pair
is stored and whichever `.hic` version holds it); the application is one launch of mst_balance_apply_pairs
(csrc/mst_balance.hip) for any number of pairs.  balanced_pairs / balanced_batches hand each pair its records with v' > 0;
balanced_segments hands a batch over as the launch left it -- concatenated, unfiltered, with the host segment table -- for a
consumer that skips such records itself (the pile-up of mustache_amd/pileup.py's genome mode).

A pairs file is the second source of the same assembly (mustache_amd/pairs.py states its rules).  The chromosomes and their
lengths are the `#chromsize` table's, in table order; the file is parsed once with its trans rows kept (8 bytes of host memory
each).  The trans rows of the whole genome are uploaded and binned in one pass (pairs.bin_trans_device, csrc/mst_pairs_trans.hip)
into the same resident (x, y, v) records a `.hic` pair gives; under `all` each chromosome's cis rows are binned by
pairs.bin_pairs_device with every diagonal and lose their pixels below IGNORE_DIAGS; under `inter` no cis row is uploaded.
Unlike a `.hic` matrix the rows' count is known before the upload, so the memory check comes first: pairs_upload_bytes against
torch.cuda.mem_get_info.  Integer counts reach float64 unrounded, so a pairs file and a `.hic` file of the same contacts give
the same bias to the bit.

genome_bias is two phases: read_genome (everything above up to the assembly: the per-chromosome cis parts, kept apart, and the
resident trans records) and solve_genome (the assembly and the solver).  Between them an optional thin_genome
(`--downsample-genome`, `--match-depth-genome`; the rule is mustache_amd/downsample.py's): each cis part through
mst_thin_counts, one launch per chromosome; the resident trans records through mst_thin_pairs, consecutive pairs sharing a
launch up to APPLY_BATCH_RECORDS records, as balanced_batches forms its batches.  The memory check counts what a launch adds
(THIN_CIS_BYTES, THIN_TRANS_BYTES per record), and under `--match-depth-genome` that both samples' raw sets are resident before
either is solved (check_solve_memory).

coarsen_genome (`--coarser-genome`; the rule is mustache_amd/multires.py's) derives a NEW GenomeRead at R = k r from one at r,
after the thinning and before any solve: each cis part through mst_coarsen_records, the resident trans records through
mst_coarsen_pairs in the same batches of pairs, each batch with a key space of its own.  Its memory check counts what a launch
adds (COARSEN_CIS_BYTES, COARSEN_TRANS_BYTES per record and 8 bytes per dense counter).
"""
import numpy as np

from .balance import METHODS, BalanceError

PIXELS = ("all", "inter")
IGNORE_DIAGS = 2                  # inside a chromosome only
RESIDENT_BYTES = 16               # a resident trans record: x int32, y int32, v float64
ASSEMBLED_BYTES = 24              # a pixel in genome coordinates: lo int64, hi int64, v float64
CSR_BUILD_BYTES = 160             # BalanceCSR's peak per pixel: the filtered copy, two sorts with their keys, orders and scratch,
                                  # both triangles of (row, col, val) -- an estimate, rounded up
APPLY_BATCH_RECORDS = 1 << 26     # records of one mst_balance_apply_pairs launch in balanced_batches (its copy: 24 bytes each)


def _canon(name):
    return "chr" + str(name).replace("chr", "")


def estimate_bytes(records):
    """Device bytes the balancing will have asked for once `records` pixels are assembled: the assembled set and BalanceCSR's
    build, beside what is already resident."""
    return int(records) * (ASSEMBLED_BYTES + CSR_BUILD_BYTES)


def genome_layout(lengths, res):
    """(bins per chromosome, offsets, n) of chromosome lengths in bp, file order"""
    bins = [int(length) // int(res) + 1 for length in lengths]
    offsets = [0] * len(bins)
    for c in range(1, len(bins)):
        offsets[c] = offsets[c - 1] + bins[c - 1]
    return bins, offsets, int(sum(bins))


def check_genome_request(method, pixels, files, bias, norm_method, balance, world, trans, pairs_trans=False):
    """Raise BalanceError with the text of the `Error:` line when `--balance-genome method --balance-pixels pixels` cannot be
    honoured; return (method in upper case, pixels).  files: the input path(s); bias: a -b / -b1 / -b2 file or None; balance:
    what --balance was given; world: the ranks of the run; trans: "all" when every pair of the run is inter-chromosomal,
    "some" when only some are, "none" when none is (True / False: "all" / "none"); pairs_trans: --pairs-trans, with which a
    `.pairs` / `.pairs.gz` file is an input like a `.hic` file (its trans rows are kept and binned: mustache_amd/pairs.py)."""
    from .request import balance_on_trans, trans_input
    trans = {True: "all", False: "none"}.get(trans, trans)
    if trans != "none" and balance_on_trans(balance):
        raise BalanceError(balance_on_trans(balance))
    if method is None:
        raise BalanceError("--balance-pixels %s without --balance-genome: it chooses the pixels --balance-genome balances on"
                           % pixels)
    m = str(method).upper()
    if m not in METHODS:
        raise BalanceError("--balance-genome %s: unknown method (supported: %s)" % (method, ", ".join(METHODS)))
    px = str(pixels).lower()
    if px not in PIXELS:
        raise BalanceError("--balance-pixels %s: unknown value (supported: %s)" % (pixels, ", ".join(PIXELS)))
    if trans != "all":
        raise BalanceError("--balance-genome is for inter-chromosomal calls; use --balance")
    files = [files] if isinstance(files, str) else list(files or [])
    if trans_input(files, pairs_trans):
        raise BalanceError(trans_input(files, pairs_trans))
    if bias:
        raise BalanceError("--balance-genome %s and a bias file (-b / -b1 / -b2): give either a bias file or --balance-genome, "
                           "not both" % m)
    if norm_method and str(norm_method).upper() != "NONE":
        raise BalanceError("--balance-genome %s and -norm %s: --balance-genome reads raw counts; leave -norm unset or NONE"
                           % (m, norm_method))
    for p in files:
        if str(p).endswith((".cool", ".mcool")):
            raise BalanceError("--balance-genome %s and %s: .cool/.mcool files carry their own `weight` column; "
                               "--balance-genome is for .hic input" % (m, p))
    if world > 1:
        raise BalanceError("--balance-genome %s in a multi-rank run (world size %d): balancing runs on one GPU; "
                           "start a single process" % (m, world))
    return m, px


def add_arguments(parser):
    """--balance-genome and --balance-pixels of both command lines; `balance_pixels_given` tells a given `all` from the default"""
    import argparse

    class _Given(argparse.Action):
        def __call__(self, parser, namespace, values, option_string=None):
            namespace.balance_pixels, namespace.balance_pixels_given = values, True

    parser.add_argument("--balance-genome", dest="balance_genome", default=None, metavar="ICE|NEWTON",
                        help="OPTIONAL: for inter-chromosomal calls (-ch A -ch2 B, --trans-all) on .hic input: balance the whole "
                             "genome's raw matrix on the GPU and call from the balanced records, instead of -norm")
    parser.add_argument("--balance-pixels", dest="balance_pixels", default="all", metavar="all|inter", action=_Given,
                        help="OPTIONAL: the pixels --balance-genome balances on: all (cis and trans, default) or inter (trans only)")
    parser.add_argument("--pairs-trans", dest="pairs_trans", action="store_true",
                        help="OPTIONAL: .pairs / .pairs.gz input only: keep the file's inter-chromosomal rows (8 bytes of host "
                             "memory each) so that -ch A -ch2 B and --trans-all run from it; needs --balance-genome")
    parser.set_defaults(balance_pixels_given=False)


class GenomeBias:
    """What genome_bias returns.  chromosomes: the names in file order; bins / offsets: n_c and off_c; n; bias: host float64 [n]
    (NaN on masked bins); info: balance.solve's info dict plus "pixels" and "records" (the pixels assembled); records(a, b): the
    resident raw device records of a pair."""

    def __init__(self, chromosomes, bins, offsets, n, bias, info, device, records):
        self.chromosomes, self.bins, self.offsets, self.n = list(chromosomes), list(bins), list(offsets), int(n)
        self.bias, self.info, self.device = bias, info, device
        self._records = records                     # {(i, j), i < j: (x of i, y of j, v)} device tensors
        self._index = {}
        for i, name in enumerate(self.chromosomes):
            self._index.setdefault(str(name), i)
        for i, name in enumerate(self.chromosomes):
            self._index.setdefault(_canon(name), i)
        self._bias_d = None

    def index(self, chrom):
        i = self._index.get(str(chrom), self._index.get(_canon(chrom)))
        if i is None:
            raise NameError('wrong chromosome name!')
        return i

    def of(self, chrom):
        """that chromosome's slice of the bias"""
        i = self.index(chrom)
        return self.bias[self.offsets[i]:self.offsets[i] + self.bins[i]]

    def bias_device(self):
        import torch
        if self._bias_d is None:
            self._bias_d = torch.from_numpy(np.ascontiguousarray(self.bias, np.float64)).to(self.device)
        return self._bias_d

    def records(self, a, b):
        """(x = bins of a, y = bins of b, v) of the pair's raw records as resident device tensors, or None when it has none (or
        when they were not kept, or have been released)"""
        i, j = self.index(a), self.index(b)
        rec = self._records.get((min(i, j), max(i, j)))
        if rec is None or i == j:
            return None
        return rec if i < j else (rec[1], rec[0], rec[2])

    def release(self, a, b):
        i, j = self.index(a), self.index(b)
        self._records.pop((min(i, j), max(i, j)), None)

    @property
    def label(self):
        return "the genome (%s pixels)" % self.info["pixels"]


def _no_matrix(e):
    """a HicError that only says the file holds no matrix for this pair / chromosome: an empty matrix"""
    return getattr(e, "code", None) == -4 and "matrix for" in str(e)


def _check_memory(records, resident):
    import torch
    free = int(torch.cuda.mem_get_info()[0])
    need = estimate_bytes(records)
    if need > free:
        raise BalanceError("--balance-genome: balancing the %d pixels read so far needs about %d bytes of device memory beside the "
                           "%d resident ones, %d bytes are free" % (records, need, resident, free))


def _hic_source(f, res, dev, pixels, verbose):
    """The `.hic` source of genome_bias: (names, lengths, cis, trans).  cis() yields (c, x, d, v) int64 / float64 device tensors
    of chromosome c's raw matrix through hicfile.read_intra_packed; trans() yields ((i, j), (x, y, v)) through
    trans.read_hic_trans.  Every matrix is read once."""
    import torch
    from . import readers
    from .hicfile import HicError, read_intra_packed
    from .trans import read_hic_trans
    names = list(readers.list_chromosomes(f, res))
    with readers._HIC_LOCK:
        lengths_of = dict(readers._hic_handle(f).chromosomes())

    def cis():
        for c, name in enumerate(names):
            with readers._HIC_LOCK:
                try:
                    pc = read_intra_packed(readers._hic_handle(f), name, res, "NONE", -1, int(lengths_of[name]))
                except HicError as e:
                    if not _no_matrix(e):
                        raise
                    continue
            if len(pc) == 0:
                continue
            x = torch.from_numpy(pc.x[:pc.count]).to(dev).to(torch.int64)
            d = torch.from_numpy(pc.dist[:pc.count]).to(dev).to(torch.int64)
            v = torch.from_numpy(pc.v[:pc.count]).to(dev).to(torch.float64)
            del pc
            yield c, x, d, v

    def trans():
        for i in range(len(names)):
            for j in range(i + 1, len(names)):
                try:
                    rec = read_hic_trans(f, "NONE", names[i], names[j], res, device=dev)
                except HicError as e:
                    if not _no_matrix(e):
                        raise
                    continue
                yield (i, j), rec

    return names, [lengths_of[c] for c in names], cis, trans


def pairs_upload_bytes(rows, cells, budget):
    """Device bytes the binning of `rows` stored trans rows asks for before a record exists: the rows (8 bytes each), the far
    list (12 bytes each: one entry per row always suffices) and the counter array (4 bytes per cell of the genome's trans
    matrices when that fits `budget`, pairs.dense_budget(); none otherwise)"""
    return int(rows) * (8 + 12) + (4 * int(cells) if 4 * int(cells) <= int(budget) else 0)


def pairs_open(f, zero_based):
    """the parsed pairs file with its trans rows (the cached handle; the one parse of a run); a file the reader refuses -- one
    without `#chromsize` lines above all -- is a BalanceError with the reader's text.  Touches no GPU."""
    from . import pairs as pr
    from .hicfile import HicError
    with pr._LOCK:
        try:
            return pr.pairs_handle(f, zero_based, keep_trans=True)
        except HicError as e:
            raise BalanceError(str(e))


def _pairs_source(h, f, res, dev, pixels, verbose, zero_based):
    """The pairs source of genome_bias (mustache_amd/pairs.py): chromosomes and lengths are the `#chromsize` table's, in table
    order; cis() bins each chromosome's cis rows (pairs.bin_pairs_device, every diagonal); trans() bins the stored trans rows of
    the whole file in one pass (pairs.bin_trans_device).  The file is parsed once, with its trans rows kept."""
    import os
    import torch
    from . import pairs as pr
    with pr._LOCK:
        table = h.chromosomes()
        totals, tcount = h.counters(), h.trans_counters()
    names, lengths = [n for n, _ in table], [length for _, length in table]
    bins = genome_layout(lengths, res)[0]
    stats = {}

    def check_upload(rows):
        need = pairs_upload_bytes(rows, pr.trans_tables(lengths, bins)[1], pr.dense_budget(dev))
        free = int(torch.cuda.mem_get_info()[0])
        if need > free:
            raise BalanceError("--balance-genome: binning the %d trans rows of %s needs about %d bytes of device memory, "
                               "%d bytes are free" % (rows, os.path.basename(str(f)), need, free))

    check_upload(tcount["stored"])           # known since the parse: a run that cannot hold them ends before any upload

    def cis():
        for c, name in enumerate(names):
            with pr._LOCK:
                p1, p2, out_of_range = h.rows(c)
                if len(p1) == 0:
                    continue
                d1, d2 = torch.from_numpy(p1).to(dev), torch.from_numpy(p2).to(dev)
            px = pr.bin_pairs_device(d1, d2, res, zero_based=zero_based, length=lengths[c], distance_bins=None, device=dev)
            del d1, d2
            if px.dropped != out_of_range:
                raise RuntimeError("pairs: the device dropped %d rows of %s as out of range, the host reader counted %d"
                                   % (px.dropped, name, out_of_range))
            if len(px):
                yield c, px.x.to(torch.int64), px.dist.to(torch.int64), px.count.to(torch.float64)

    def trans():
        with pr._LOCK:
            pa, pb, seg_off, out_of_range = h.trans_rows()
            check_upload(len(pa))
            da, db = torch.from_numpy(pa).to(dev), torch.from_numpy(pb).to(dev)
        got = pr.bin_trans_device(da, db, seg_off, lengths, res, zero_based=zero_based, bins=bins, out_of_range=out_of_range,
                                  device=dev, names=names, stats=stats)
        del da, db
        if verbose:
            print("pairs %s: %d rows read, %d trans rows (%d stored, %d naming a chromosome the table lacks, %d out of range), "
                  "%d trans pixels, %d pairs with records"
                  % (os.path.basename(str(f)), totals["rows"], totals["trans"], tcount["stored"], tcount["unknown"],
                     tcount["out_of_range"], stats["pixels"], stats["pairs"]))
        for key in sorted(got):
            yield key, got.pop(key)

    return names, lengths, cis, trans


class GenomeRead:
    """What read_genome returns, and solve_genome takes: the genome's raw pixels on the device, not yet assembled.  names,
    lengths, bins, offsets, n: the layout; pixels: `all` or `inter`; cis: [(c, x, dist, v)] int64 / int64 / float64 device
    tensors of chromosome c's pixels that enter the assembly (inside the chromosome, dist >= IGNORE_DIAGS; `all` only), kept
    apart; records: {(i, j), i < j: (x of i, y of j, v)} int32 / int32 / float64 resident device tensors of every pair that
    has any, in reading order; source: the file's name; res: the resolution in bp (None: not stated)."""

    def __init__(self, names, lengths, bins, offsets, n, pixels, device, source, res=None):
        self.res = None if res is None else int(res)
        self.names, self.lengths, self.bins, self.offsets, self.n = list(names), list(lengths), list(bins), list(offsets), int(n)
        self.pixels, self.device, self.source = pixels, device, source
        self.cis, self.records = [], {}

    def entering(self):
        """the pixels the assembly will hold"""
        total = sum(int(v.numel()) for _, _, _, v in self.cis)
        for (i, j), (x, y, v) in self.records.items():
            total += int(((x >= 0) & (x < self.bins[i]) & (y >= 0) & (y < self.bins[j])).sum())
        return total

    def resident(self):
        return sum(int(v.numel()) for _, _, v in self.records.values())


def read_genome(f, res, pixels="all", device=None, pairs_zero_based=False, verbose=False):
    """The read phase of genome_bias: every matrix of f read once (a pairs file parsed once and binned on the device) ->
    GenomeRead.  The memory check runs after each matrix, as the module's header says.  pixels is `all` or `inter` as
    check_genome_request returns it."""
    import torch
    from . import pairs as pairs_mod
    from ._lib import require_gpu
    from_pairs = pairs_mod.is_pairs(f)
    handle = pairs_open(f, pairs_zero_based) if from_pairs else None
    require_gpu()
    res = int(res)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(dev):
        if from_pairs:
            names, lengths, cis, trans = _pairs_source(handle, f, res, dev, pixels, verbose, pairs_zero_based)
        else:
            names, lengths, cis, trans = _hic_source(f, res, dev, pixels, verbose)
        bins, offsets, n = genome_layout(lengths, res)
        read = GenomeRead(names, lengths, bins, offsets, n, pixels, dev, f, res)
        total, resident = 0, 0
        if pixels == "all":
            for c, x, d, v in cis():
                keep = (d >= IGNORE_DIAGS) & (x >= 0) & (x + d < bins[c])
                read.cis.append((c, x[keep], d[keep], v[keep]))
                del x, d, v
                total += int(read.cis[-1][3].numel())
                _check_memory(total, resident)
        for (i, j), (x, y, v) in trans():
            if v.numel() == 0:
                continue
            read.records[(i, j)] = (x, y, v)
            resident += RESIDENT_BYTES * int(v.numel())
            total += int(((x >= 0) & (x < bins[i]) & (y >= 0) & (y < bins[j])).sum())
            _check_memory(total, resident)
    return read


THIN_CIS_BYTES = 8 + 8 + 1 + 24   # thinning a cis part, per pixel: the int32 x and dist, k, the mask, the compacted copy
THIN_TRANS_BYTES = 16 + 8 + 1 + 16   # thinning a batch of pairs, per record: the concatenated copy, k, the mask, the compacted copy


def _check_thin_memory(records, per_record, resident):
    import torch
    free = int(torch.cuda.mem_get_info()[0])
    need = int(records) * per_record
    if need > free:
        raise BalanceError("--balance-genome: thinning %d pixels needs about %d bytes of device memory beside the %d resident "
                           "ones, %d bytes are free" % (records, need, resident, free))


def check_solve_memory(reads):
    """Under --match-depth-genome both samples' raw sets are on the device before either is solved: BalanceError unless the
    larger assembly fits what is free now."""
    import torch
    if not reads:
        return
    most = max(r.entering() for r in reads)
    free = int(torch.cuda.mem_get_info()[0])
    if estimate_bytes(most) > free:
        raise BalanceError("--balance-genome: balancing %d pixels needs about %d bytes of device memory beside the %d resident "
                           "ones of both samples, %d bytes are free"
                           % (most, estimate_bytes(most), RESIDENT_BYTES * sum(r.resident() for r in reads), free))


def _pair_batches(read, max_records):
    """the keys of read.records in order, consecutive pairs together until their records reach max_records"""
    batch, held = [], 0
    for key, (_, _, v) in read.records.items():
        batch.append(key)
        held += int(v.numel())
        if held >= max_records:
            yield batch
            batch, held = [], 0
    if batch:
        yield batch


def _batch_tensors(read, keys):
    import torch
    recs = [read.records[key] for key in keys]
    seg = np.zeros(len(keys) + 1, np.int64)
    np.cumsum([int(r[2].numel()) for r in recs], out=seg[1:])
    if len(recs) == 1:
        return tuple(t.contiguous() for t in recs[0]) + (seg,)
    return tuple(torch.cat([r[k] for r in recs]) for k in range(3)) + (seg,)


def genome_depth(read, max_records=APPLY_BATCH_RECORDS):
    """N of mustache_amd/downsample.py for a GenomeRead: (the cis contacts, the trans contacts), integer sums from the kernels
    (mst_thin_counts per chromosome, mst_thin_pairs per batch of pairs; nothing is drawn).  DownsampleError for a count that
    is no integer."""
    import torch
    from .downsample import depth_of, depth_of_pairs
    n_cis = n_trans = 0
    with torch.cuda.device(read.device):
        for c, x, d, v in read.cis:
            n_cis += depth_of(x.to(torch.int32), d.to(torch.int32), v, read.names[c], device=read.device)
        for keys in _pair_batches(read, max_records):
            x, y, v, seg = _batch_tensors(read, keys)
            n_trans += sum(depth_of_pairs(x, y, v, seg, [(read.names[i], read.names[j]) for i, j in keys], device=read.device))
    return n_cis, n_trans


def thin_genome(read, T, seed=0, sample=0, max_records=APPLY_BATCH_RECORDS):
    """The optional step between read_genome and solve_genome: the rule of mustache_amd/downsample.py on a GenomeRead, in place.
    Each cis part goes through mst_thin_counts (one launch per chromosome, the one-chromosome draw unchanged), the resident
    trans records through mst_thin_pairs, consecutive pairs sharing a launch until their records reach max_records.  Pixels
    and records with k = 0 are dropped, a pair left without a record leaves `records`, the counts come back as float64: from
    here on nothing knows the map was thinned.  -> ((cis contacts kept, in), (trans contacts kept, in)).  DownsampleError for
    a count that is no integer and for two chromosomes whose stripped names are equal; BalanceError when the device's free
    memory cannot hold what a launch adds."""
    import torch
    from .downsample import pair_tag, thin_pairs, thin_records
    for i in range(len(read.names)):                  # before anything is drawn: every pair of the file has a stream of its own
        for j in range(i + 1, len(read.names)):
            pair_tag(read.names[i], read.names[j])
    cis_kept = cis_in = trans_kept = trans_in = 0
    with torch.cuda.device(read.device):
        resident = RESIDENT_BYTES * read.resident()
        for at, (c, x, d, v) in enumerate(read.cis):
            _check_thin_memory(int(v.numel()), THIN_CIS_BYTES, resident)
            (tx, td, tk), total, kept = thin_records(x.to(torch.int32), d.to(torch.int32), v, read.names[c], T, seed=seed,
                                                     sample=sample, device=read.device)
            read.cis[at] = (c, tx.to(torch.int64), td.to(torch.int64), tk.to(torch.float64))
            cis_in, cis_kept = cis_in + total, cis_kept + kept
            del x, d, v, tx, td, tk
        for keys in list(_pair_batches(read, max_records)):
            _check_thin_memory(sum(int(read.records[key][2].numel()) for key in keys), THIN_TRANS_BYTES, resident)
            x, y, v, seg = _batch_tensors(read, keys)
            k, totals = thin_pairs(x, y, v, seg, [(read.names[i], read.names[j]) for i, j in keys], T, seed=seed, sample=sample,
                                   device=read.device)
            del v
            keep = k > 0
            for p, key in enumerate(keys):
                s, e = int(seg[p]), int(seg[p + 1])
                m = keep[s:e]
                got = (x[s:e][m], y[s:e][m], k[s:e][m].to(torch.float64))
                if got[2].numel():
                    read.records[key] = got
                else:
                    del read.records[key]
                trans_in, trans_kept = trans_in + totals[p][0], trans_kept + totals[p][1]
            del x, y, k, keep
    return (cis_kept, cis_in), (trans_kept, trans_in)


COARSEN_CIS_BYTES = 8 + 16 + 16 + 24   # coarsening a cis part, per pixel: the int32 x and dist, a far entry, a compacted record, its int64 / float64 copy
COARSEN_TRANS_BYTES = 16 + 16 + 16 + 16   # coarsening a batch of pairs, per record: the concatenated copy, a far entry, key and sum, the decoded record
COARSEN_CELL_BYTES = 8            # a dense counter


def _check_coarsen_memory(records, per_record, cells, resident):
    import torch
    free = int(torch.cuda.mem_get_info()[0])
    need = int(records) * per_record + COARSEN_CELL_BYTES * int(cells)
    if need > free:
        raise BalanceError("--balance-genome: coarsening %d pixels needs about %d bytes of device memory beside the %d resident "
                           "ones, %d bytes are free" % (records, need, resident, free))


def coarsen_genome(read, factor, max_records=APPLY_BATCH_RECORDS):
    """The genome's map of a GenomeRead at r -> a NEW GenomeRead at R = factor * r (mustache_amd/multires.py states the rule):
    the names, lengths and pixels of `read`, genome_layout(lengths, R).  Each cis part goes through multires.coarsen_records
    and keeps D >= IGNORE_DIAGS, X + D < n'_c; the resident trans records go through multires.coarsen_pairs, consecutive pairs
    sharing a launch until their records reach max_records (_pair_batches).  `read` is left untouched.  MultiresError for a
    count that is no integer; BalanceError when the device's free memory cannot hold what a launch adds."""
    import torch
    from .multires import coarsen_pairs, coarsen_records
    from .pairs import dense_budget, pair_list, trans_tables
    k = int(factor)
    if k < 1:
        raise ValueError("coarsen_genome: the factor is an integer >= 1")
    if not read.res:
        raise ValueError("coarsen_genome: the GenomeRead does not know its resolution (read_genome sets it)")
    R = int(read.res) * k
    bins, offsets, n = genome_layout(read.lengths, R)
    out = GenomeRead(read.names, read.lengths, bins, offsets, n, read.pixels, read.device, read.source, R)
    tables = trans_tables(read.lengths, bins)[0]
    index = {pair: p for p, pair in enumerate(pair_list(len(bins)))}
    with torch.cuda.device(read.device):
        resident = RESIDENT_BYTES * read.resident()
        for c, x, d, v in read.cis:
            _check_coarsen_memory(int(v.numel()), COARSEN_CIS_BYTES, 0, resident)
            X, D, V = coarsen_records(x.to(torch.int32), d.to(torch.int32), v, k, device=read.device, chromosome=read.names[c])
            keep = (D >= IGNORE_DIAGS) & (X + D < bins[c])
            if bool(keep.any()):
                out.cis.append((c, X[keep].to(torch.int64), D[keep].to(torch.int64), V[keep].to(torch.float64)))
            del X, D, V, keep
        budget = dense_budget(read.device)
        for keys in _pair_batches(read, max_records):
            # the batch's pairs get a key space of their own: the counters cover their cells only
            sub = np.ascontiguousarray(tables[:, [index[key] for key in keys]])
            cells = sub[2] * sub[3]
            sub[4] = np.cumsum(cells) - cells
            dense = int(cells.sum()) if COARSEN_CELL_BYTES * int(cells.sum()) <= budget else 0
            _check_coarsen_memory(sum(int(read.records[key][2].numel()) for key in keys), COARSEN_TRANS_BYTES, dense, resident)
            x, y, v, seg = _batch_tensors(read, keys)
            got = coarsen_pairs(x, y, v, seg, sub, k, dense_cells=dense, device=read.device)
            del x, y, v
            for p in sorted(got):
                out.records[keys[p]] = got[p]
    return out


def solve_genome(read, method="NEWTON", keep_records=True, **solver_args):
    """The solve phase of genome_bias: the assembly of a GenomeRead's pixels in genome coordinates, then
    solve(..., ignore_diags=0) -> GenomeBias.  The cis parts are consumed."""
    import torch
    from .balance import solve
    dev, bins, offsets = read.device, read.bins, read.offsets
    with torch.cuda.device(dev):
        los, his, vs = [], [], []
        total = 0
        while read.cis:
            c, x, d, v = read.cis.pop(0)
            los.append(x + offsets[c])
            his.append(x + d + offsets[c])
            vs.append(v)
            total += int(v.numel())
            del x, d, v
        for (i, j), (x, y, v) in read.records.items():
            inside = (x >= 0) & (x < bins[i]) & (y >= 0) & (y < bins[j])
            los.append(x[inside].to(torch.int64) + offsets[i])
            his.append(y[inside].to(torch.int64) + offsets[j])
            vs.append(v[inside])
            total += int(vs[-1].numel())
        if vs:
            lo, hi, v = torch.cat(los), torch.cat(his), torch.cat(vs)
        else:
            lo = hi = torch.zeros(0, dtype=torch.int64, device=dev)
            v = torch.zeros(0, dtype=torch.float64, device=dev)
        del los, his, vs
        bias, info = solve(method, lo, hi, v, read.n, ignore_diags=0, device=dev, **solver_args)
    info["pixels"], info["records"] = read.pixels, total
    return GenomeBias(read.names, bins, offsets, read.n, bias, info, dev, read.records if keep_records else {})


def genome_bias(f, res, method="NEWTON", pixels="all", device=None, keep_records=True, pairs_zero_based=False, verbose=False,
                **solver_args):
    """Balance the whole genome of f at resolution res -> GenomeBias.  f is a `.hic` file, or a `.pairs` / `.pairs.gz` file with
    `#chromsize` lines (pairs_zero_based: its position convention).  Every matrix is read once -- a pairs file is parsed once
    and its rows are binned on the device; the trans pairs' raw records stay on the device when keep_records.  Both sources
    feed one assembly: per-chromosome cis pixels (`all` only), per-pair trans records, then solve(..., ignore_diags=0) --
    read_genome, then solve_genome; a thinning (thin_genome) may stand between the two.
    Raises BalanceError for an unknown method or pixels value and when the records do not fit the device's free memory."""
    from . import pairs as pairs_mod
    method, pixels = check_genome_request(method, pixels, [f], None, None, None, 1, True, pairs_trans=pairs_mod.is_pairs(f))
    read = read_genome(f, res, pixels, device, pairs_zero_based, verbose)
    return solve_genome(read, method, keep_records, **solver_args)


def apply_pairs(x, y, v, seg_off, row_off, col_off, bias, out=None):
    """mst_balance_apply_pairs on device tensors: x, y int32 [N], v float64 [N], seg_off int64 [P + 1], row_off / col_off int64
    [P], bias float64 [n] -> v' float64 [N] (`out`, which may be v itself; a new tensor by default)"""
    import torch
    from . import _lib
    from ._lib import ptr as _ptr, stream as _stream
    lib = _lib.require_gpu()
    N, P = int(v.numel()), int(row_off.numel())
    if int(x.numel()) != N or int(y.numel()) != N or int(seg_off.numel()) != P + 1 or int(col_off.numel()) != P:
        raise ValueError("apply_pairs: x, y, v of one length, seg_off of P + 1 and row_off, col_off of P entries")
    for t, dt in ((x, torch.int32), (y, torch.int32), (v, torch.float64), (seg_off, torch.int64), (row_off, torch.int64),
                  (col_off, torch.int64), (bias, torch.float64)):
        if t.dtype != dt or not t.is_cuda or not t.is_contiguous():
            raise ValueError("apply_pairs: contiguous device tensors of the documented types")
    if out is None:
        out = torch.empty_like(v)
    with torch.cuda.device(v.device):
        _lib.check(lib.mst_balance_apply_pairs(_ptr(x), _ptr(y), _ptr(v), N, _ptr(seg_off), _ptr(row_off), _ptr(col_off), P,
                                               _ptr(bias), int(bias.numel()), _ptr(out), _stream()))
    return out


def _apply_batch(gb, pairs, release):
    """ONE launch of mst_balance_apply_pairs over the resident raw records of `pairs` = [(a, b)]: (x, y, v', seg) with the
    pairs' records concatenated in order, v' unfiltered and seg the host int64 [P + 1] segment table (a pair without a record
    is an empty segment); None when no pair has a record.  release: the pairs' raw records leave `gb` once they are applied."""
    import torch
    dev = gb.device
    recs = [gb.records(a, b) for a, b in pairs]
    lens = [0 if r is None else int(r[2].numel()) for r in recs]
    if sum(lens) == 0:
        return None
    seg = np.zeros(len(pairs) + 1, np.int64)
    np.cumsum(lens, out=seg[1:])
    row = np.asarray([gb.offsets[gb.index(a)] for a, _ in pairs], np.int64)
    col = np.asarray([gb.offsets[gb.index(b)] for _, b in pairs], np.int64)
    with torch.cuda.device(dev):
        live = [r for r in recs if r is not None]
        if len(live) == 1:
            x, y, v = (t.contiguous() for t in live[0])
        else:
            x, y, v = (torch.cat([r[k] for r in live]) for k in range(3))
        del live, recs
        if release:
            for a, b in pairs:
                gb.release(a, b)
        table = torch.from_numpy(np.concatenate([seg, row, col])).to(dev)
        P = len(pairs)
        vb = apply_pairs(x, y, v, table[:P + 1], table[P + 1:2 * P + 1], table[2 * P + 1:], gb.bias_device())
    return x, y, vb, seg


def balanced_pairs(gb, pairs, release=False):
    """The batch form: the balanced records of every pair of `pairs` = [(a, b)] through ONE launch of mst_balance_apply_pairs.
    Per pair (x = bins of a, y = bins of b, v') on the device with the records of v' > 0 only, or None when nothing is left.
    release: the pairs' raw records leave `gb` once they are applied."""
    import torch
    out = [None] * len(pairs)
    got = _apply_batch(gb, pairs, release)
    if got is None:
        return out
    x, y, vb, seg = got
    with torch.cuda.device(gb.device):
        keep = vb > 0
        for p in range(len(pairs)):
            s, e = int(seg[p]), int(seg[p + 1])
            if e > s:
                k = keep[s:e]
                got = (x[s:e][k], y[s:e][k], vb[s:e][k])
                out[p] = got if got[2].numel() else None
    return out


def balanced_pair(gb, a, b):
    """(x, y, v') of one pair (device tensors, v' > 0 only), or None: balanced_pairs for a batch of one"""
    return balanced_pairs(gb, [(a, b)])[0]


def balanced_batches(gb, pairs, release=True, max_records=APPLY_BATCH_RECORDS):
    """(k, balanced records of pairs[k] or None) for every k in order; consecutive pairs share a launch until their raw records
    reach max_records"""
    for k, j in _batch_ends(gb, pairs, max_records):
        for i, rec in enumerate(balanced_pairs(gb, pairs[k:j], release=release)):
            yield k + i, rec


def _batch_ends(gb, pairs, max_records):
    """balanced_batches' rule as (k, j) index ranges: consecutive pairs until their raw records reach max_records"""
    k = 0
    while k < len(pairs):
        j, held = k, 0
        while j < len(pairs):
            r = gb.records(*pairs[j])
            held += 0 if r is None else int(r[2].numel())
            j += 1
            if held >= max_records:
                break
        yield k, j
        k = j


def balanced_segments(gb, pairs, release=True, max_records=APPLY_BATCH_RECORDS):
    """balanced_batches without the filter: (k, j, x, y, v', seg) per batch of the consecutive pairs pairs[k:j] -- the
    concatenated records (device int32 / int32 / float64) straight from one mst_balance_apply_pairs launch and the host int64
    segment table seg [j - k + 1].  Nothing is compacted and the host waits for nothing: a record the balancing removes has
    v' = 0 (NaN for a NaN count) and the consumer skips it (mst_pileup_trans_batch does).  A batch none of whose pairs has a
    record comes with x = y = v' = None and a table of zeros.  The batch rule and `release` are balanced_batches'."""
    for k, j in _batch_ends(gb, pairs, max_records):
        got = _apply_batch(gb, pairs[k:j], release)
        if got is None:
            yield k, j, None, None, None, np.zeros(j - k + 1, np.int64)
        else:
            yield (k, j) + got
