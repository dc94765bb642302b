"""Balancing of the WHOLE GENOME's contact matrix on the GPU, for inter-chromosomal (trans) calling on `.hic` files that carry no
usable normalisation vector: `--balance-genome ICE|NEWTON` (with `--balance-pixels all|inter`) on the command lines,
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
(csrc/mst_balance.hip) for any number of pairs.
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


def check_genome_request(method, pixels, files, bias, norm_method, balance, world, trans):
    """Raise BalanceError with the text of the `Error:` line when `--balance-genome method --balance-pixels pixels` cannot be
    honoured; return (method in upper case, pixels).  files: the input path(s); bias: a -b / -b1 / -b2 file or None; balance:
    what --balance was given; world: the ranks of the run; trans: "all" when every pair of the run is inter-chromosomal,
    "some" when only some are, "none" when none is (True / False: "all" / "none")."""
    trans = {True: "all", False: "none"}.get(trans, trans)
    if balance is not None and trans != "none":
        raise BalanceError("--balance does not apply to inter-chromosomal pairs")
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
    if not all(str(p).endswith((".hic", ".cool", ".mcool")) for p in files):
        raise BalanceError("Interchromosomal analysis is only supported for .hic and .cool input formats.")
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
    parser.set_defaults(balance_pixels_given=False)


def request_of(args, files, bias, world, pairs):
    """The command lines' use of check_genome_request: None when neither option was given, else (method, pixels); raises
    BalanceError.  pairs: the run's (chromosome, chromosome2) list."""
    if args.balance_genome is None and not args.balance_pixels_given:
        return None
    n_trans = sum(1 for a, b in pairs if a != b)
    trans = "none" if n_trans == 0 else ("all" if n_trans == len(pairs) else "some")
    return check_genome_request(args.balance_genome, args.balance_pixels, files, bias, args.norm_method, args.balance, world, trans)


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


def genome_bias(f, res, method="NEWTON", pixels="all", device=None, keep_records=True, **solver_args):
    """Balance the whole genome of the `.hic` file f at resolution res -> GenomeBias.  Every matrix is read once; the trans
    pairs' raw records stay on the device when keep_records.  Raises BalanceError for an unknown method or pixels value and
    when the records do not fit the device's free memory."""
    import torch
    from . import readers
    from .balance import solve
    from .hicfile import HicError, read_intra_packed
    from ._lib import require_gpu
    from .trans import read_hic_trans
    method, pixels = check_genome_request(method, pixels, [f], None, None, None, 1, True)
    require_gpu()
    res = int(res)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    names = list(readers.list_chromosomes(f, res))
    with readers._HIC_LOCK:
        lengths_of = dict(readers._hic_handle(f).chromosomes())
    bins, offsets, n = genome_layout([lengths_of[c] for c in names], res)
    los, his, vs = [], [], []
    records, total, resident = {}, 0, 0
    with torch.cuda.device(dev):
        if pixels == "all":
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
                keep = (d >= IGNORE_DIAGS) & (x >= 0) & (x + d < bins[c])
                x, d, v = x[keep], d[keep], v[keep]
                los.append(x + offsets[c])
                his.append(x + d + offsets[c])
                vs.append(v)
                total += int(v.numel())
                _check_memory(total, resident)
        for i in range(len(names)):
            for j in range(i + 1, len(names)):
                try:
                    x, y, v = read_hic_trans(f, "NONE", names[i], names[j], res, device=dev)
                except HicError as e:
                    if not _no_matrix(e):
                        raise
                    continue
                if v.numel() == 0:
                    continue
                if keep_records:
                    records[(i, j)] = (x, y, v)
                    resident += RESIDENT_BYTES * int(v.numel())
                inside = (x >= 0) & (x < bins[i]) & (y >= 0) & (y < bins[j])
                los.append(x[inside].to(torch.int64) + offsets[i])
                his.append(y[inside].to(torch.int64) + offsets[j])
                vs.append(v[inside])
                total += int(vs[-1].numel())
                _check_memory(total, resident)
        if vs:
            lo, hi, v = torch.cat(los), torch.cat(his), torch.cat(vs)
        else:
            lo = hi = torch.zeros(0, dtype=torch.int64, device=dev)
            v = torch.zeros(0, dtype=torch.float64, device=dev)
        del los, his, vs
        bias, info = solve(method, lo, hi, v, n, ignore_diags=0, device=dev, **solver_args)
    info["pixels"], info["records"] = pixels, total
    return GenomeBias(names, bins, offsets, n, bias, info, dev, records)


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


def balanced_pairs(gb, pairs, release=False):
    """The batch form: the balanced records of every pair of `pairs` = [(a, b)] through ONE launch of mst_balance_apply_pairs.
    Per pair (x = bins of a, y = bins of b, v') on the device with the records of v' > 0 only, or None when nothing is left.
    release: the pairs' raw records leave `gb` once they are applied."""
    import torch
    dev = gb.device
    recs = [gb.records(a, b) for a, b in pairs]
    lens = [0 if r is None else int(r[2].numel()) for r in recs]
    out = [None] * len(pairs)
    if sum(lens) == 0:
        return out
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
        keep = vb > 0
        for p in range(P):
            if lens[p]:
                s, e = int(seg[p]), int(seg[p + 1])
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
    k = 0
    while k < len(pairs):
        j, held = k, 0
        while j < len(pairs):
            r = gb.records(*pairs[j])
            held += 0 if r is None else int(r[2].numel())
            j += 1
            if held >= max_records:
                break
        for i, rec in enumerate(balanced_pairs(gb, pairs[k:j], release=release)):
            yield k + i, rec
        k = j
