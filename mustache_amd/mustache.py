#!/usr/bin/env python3
"""Drop-in host side for the reference's per-chromosome run (ay-lab/mustache v1.3.3, mustache/mustache.py).

Same function names, argument meaning and return types as the reference for everything on the hot path:

    mustache(c, chromosome, chromosome2, res, pval_weights, start, end, mask_size, distance_in_px,
             octave_values, st, pt)                      <- mustache.py:697-850
    process_block(...)                                   <- mustache.py:945-960
    normalize_sparse(x, y, v, resolution, distance_in_px) <- mustache.py:622-686
    regulator(f, norm_method, CHRM_SIZE, outdir, ...)    <- mustache.py:853-942
    read_pd / read_bias / get_sep / is_chr / parseBP / parse_args / main  (text input, CLI)

but the arithmetic runs in HIP kernels on an MI355X (mustache_amd/csrc, C ABI in include/mustache_hip.h).
Where the reference forks one OS process per block, this host keeps all blocks of a chromosome resident in HBM
and launches each kernel once over the whole batch.
"""
import argparse
import math
import os
import sys
import time
from collections import defaultdict

import numpy as np

from .downsample import error_line
from .tail import block_tail

_ENGINES = {}


def _engine(octave_values):
    from .engine import ScaleSpaceEngine
    key = tuple(float(o) for o in octave_values)
    eng = _ENGINES.get(key)
    if eng is None:
        eng = _ENGINES[key] = ScaleSpaceEngine(key)
    return eng


# --------------------------------------------------------------------------------------------------------------
# per-block entry point (reference mustache.py:697-850)
# --------------------------------------------------------------------------------------------------------------
def mustache(c, chromosome, chromosome2, res, pval_weights, start, end, mask_size, distance_in_px, octave_values,
             st, pt):
    """Loops of one dense block.  `c` is a square float64 array; like the reference, it is modified in place
    (diagonals <= 4 and > distance_in_px are set to 2).  `res`, `pval_weights`, `end` and `mask_size` are
    accepted and ignored, exactly as in the reference body.  Returns [[x+start, y+start, fdr, sigma], ...]."""
    import torch
    eng = _engine(octave_values)
    c = np.asarray(c)
    if c.ndim != 2 or c.shape[0] != c.shape[1] or c.dtype != np.float64:
        raise ValueError("mustache(): c must be a square float64 array")
    from .batches import BlockBatch
    intra = chromosome == chromosome2
    n = c.shape[0]
    dev = torch.from_numpy(np.ascontiguousarray(c)).to(eng.device).unsqueeze(0)
    nz, nzc = eng.prologue(dev, distance_in_px, intra)
    # BH and the selection q < pt on the device, only the selected records come back (what the per-chromosome driver does)
    found, fits = eng.sigma_loop(dev, nz, nzc, with_value=False, select_below=pt)
    batch = BlockBatch(eng, dev, nz, n, 1, nzc, found, fits)
    if int(batch.nz_count[0]) < 50:
        return []                            # mustache.py:701-702 returns before the fills of :703-706: `c` stays untouched
    # the caller's block gets the fills of mustache.py:703-706 written on the host -- the same values the device copy holds
    # (tests/test_gpu_block.py), without 128 MB coming back over PCIe per 4000 x 4000 block
    fill_like_reference(c, distance_in_px, intra)
    return block_tail(batch, 0, start, pt, st, intra=intra)


def fill_like_reference(c, distance_in_px, intra):
    """The in-place fills of mustache.py:703-706 on the caller's host block: 2 on and below diagonal 4 and, within a
    chromosome, from diagonal distance_in_px + 1 outwards."""
    n = c.shape[0]
    if c.strides[1] == 8 and c.strides[0] % 8 == 0 and c.strides[0] >= 8 * n and c.flags.writeable:
        from . import hicfile                       # rows of contiguous doubles: the threaded form in libmustache_io.so
        lib = hicfile.load()
        hicfile._check(lib, lib.mst_host_fill_block(c.ctypes.data, n, c.strides[0] // 8, int(distance_in_px), 1 if intra else 0, 8))
        return
    for r in range(n):                              # any other layout (a transposed view, ...): NumPy row slices
        c[r, :min(n, r + 5)] = 2.0
        if intra:
            c[r, r + distance_in_px + 1:] = 2.0


def process_block(i, start, end, overlap_size, cc, chromosome, chromosome2, res, pval_weights, distance_in_px,
                  octave_values, o, st, pt):
    """reference mustache.py:945-960: run one block and append the loops that survive the overlap mask to `o`."""
    mask_size = block_mask_size(i, start, end, overlap_size)
    loops = mustache(cc, chromosome, chromosome2, res, pval_weights, start[i], end[i], mask_size, distance_in_px,
                     octave_values, st, pt)
    for loop in loops:
        if loop[0] >= start[i] + mask_size or loop[1] >= start[i] + mask_size:
            o.append([loop[0], loop[1], loop[2], loop[3]])


# --------------------------------------------------------------------------------------------------------------
# tiling (reference mustache.py:896-910, :948-953)
# --------------------------------------------------------------------------------------------------------------
def block_tiling(n, distance_in_px):
    """(CHUNK_SIZE, start[], end[]) exactly as regulator computes them."""
    chunk = max(2 * distance_in_px, 2000)
    if n <= chunk:
        return chunk, [0], [n]
    start, end = [0], [chunk]
    while end[-1] < n:
        start.append(end[-1] - distance_in_px)
        end.append(start[-1] + chunk)
    end[-1] = n
    start[-1] = end[-1] - chunk
    return chunk, start, end


def block_mask_size(i, start, end, overlap_size):
    if i == 0:
        return -1
    if i == len(start) - 1:
        return end[i - 1] - start[i]
    return overlap_size


# --------------------------------------------------------------------------------------------------------------
# text readers (reference mustache.py:191-297) -- host I/O, pandas like the reference
# --------------------------------------------------------------------------------------------------------------
def parseBP(s):
    """'5kb' / '1mb' / '5000' -> base pairs; False when unparsable (reference mustache.py:29-49)."""
    if not s:
        return False
    if s.isnumeric():
        return int(s)
    s = s.lower()
    for unit, mult in (("kb", 1000), ("mb", 1000000)):
        if unit in s:
            head = s.split(unit)[0]
            return int(head) * mult if head.isnumeric() else False
    return False


def is_chr(s, c):
    return str(c).replace('chr', '') == str(s).replace('chr', '')


def get_sep(f):
    """Guess the column separator from the first line (reference mustache.py:199-215)."""
    with open(f) as fh:
        for line in fh:
            if "\t" in line:
                return '\t'
            if " " in line.strip():
                return ' '
            if "," in line:
                return ','
            if len(line.split(' ')) == 1:
                return ' '
            break
    raise FileNotFoundError


def read_bias(f, chromosome, res):
    """bin -> bias factor; NaN or < 0.2 become +inf so the contact is dropped (reference mustache.py:218-251)."""
    d = defaultdict(lambda: 1.0)
    if not f:
        return False
    sep = get_sep(f)
    with open(f) as fh:
        for pos, line in enumerate(fh):
            cols = line.strip().split(sep)
            if len(cols) == 3:
                if is_chr(cols[0], chromosome):
                    val = float(cols[2])
                    d[float(cols[1]) // res] = val if (not np.isnan(val) and val >= 0.2) else np.inf
            elif len(cols) == 1:
                val = float(cols[0])
                d[pos] = val if (not np.isnan(val) and val >= 0.2) else np.inf
    return d


def _parse_contacts_native(f, sep, chromosome):
    """(n_cols, pos1, pos2, count) through libmustache_io.so's text parser (bit for bit what pandas' C parser yields, see
    include/mustache_io.h), or None when the file needs pandas itself / MUSTACHE_TEXT_BACKEND=pandas asks for it."""
    if os.environ.get("MUSTACHE_TEXT_BACKEND", "native").lower() == "pandas":
        return None
    from .hicfile import HicError, read_text_contacts
    try:
        return read_text_contacts(f, sep, chromosome)
    except HicError as e:
        if e.code == -3:                    # a construct the native parser does not cover: let pandas decide
            return None
        raise


def _finish_text(p1, p2, cnt, distance_in_bp, bias, res):
    """read_pd after the parse: distance filter, bins, counts divided by bias[pos1 bin] then bias[pos2 bin] (`bias` = what
    read_bias returns, or False), non-positive rows dropped."""
    keep = np.abs(p1 - p2) <= ((distance_in_bp / res + 1) * res)           # (:267, :283)
    a = np.floor_divide(p1[keep], res)                                     # df[1] //= res
    b = np.floor_divide(p2[keep], res)
    cnt = cnt[keep]
    if bias:
        cnt = np.divide(cnt, np.vectorize(bias.get)(a, 1)) if len(a) else cnt
        cnt = np.divide(cnt, np.vectorize(bias.get)(b, 1)) if len(b) else cnt
    pos = cnt > 0
    a, b, cnt = a[pos].astype(np.int64), b[pos].astype(np.int64), cnt[pos]
    return np.minimum(a, b), np.maximum(a, b), cnt


def _text_records(f, sep, chromosome):
    """(pos1, pos2, count) float64 of every record read_pd reads, before its distance filter; None when a 5-column file has
    no record of the chromosome."""
    native = _parse_contacts_native(f, sep, chromosome)
    if native is not None:
        ncols, p1, p2, cnt = native
        if ncols == 5 and len(cnt) == 0:
            return None
        return p1, p2, cnt
    import pandas as pd
    df = pd.read_csv(f, sep=sep, header=None)
    df.dropna(inplace=True)
    if df.shape[1] == 5:
        df = df[np.vectorize(is_chr)(df[0], chromosome)]
        if df.shape[0] == 0:
            return None
        df = df[np.vectorize(is_chr)(df[2], chromosome)]
        a, b, cnt = 1, 3, 4
    elif df.shape[1] == 3:
        a, b, cnt = 0, 1, 2
    else:
        raise ValueError("contact text file must have 3 or 5 columns")
    return (np.asarray(df[a], np.float64), np.asarray(df[b], np.float64), np.asarray(df[cnt], np.float64))


def read_pd_balanced(f, distance_in_bp, chromosome, res, device=None, method="ICE", **solver_args):
    """read_pd under `--balance`: every record of the chromosome, before the distance filter, is balanced on the GPU
    (balance.solve with `method`); the bias is then applied as read_pd applies a -b vector.  Returns read_pd's triple, or
    None."""
    from .balance import balance_text, bias_lookup, report
    recs = _text_records(f, get_sep(f), chromosome)
    if recs is None:
        print('Could\'t read any interaction for this chromosome!')
        return
    p1, p2, cnt = recs
    bias, info = balance_text(p1, p2, cnt, res, method=method, device=device, **solver_args)
    if len(bias):
        report(info, "chromosome %s" % chromosome)
    return _finish_text(p1, p2, cnt, distance_in_bp, bias_lookup(bias), res)


def read_pd(f, distance_in_bp, bias, chromosome, res):
    """3-column (pos1 pos2 count) or 5-column (chr1 pos1 chr2 pos2 count) text -> upper-triangular COO in bin
    units, counts divided by bias[x]*bias[y], non-positive rows dropped (reference mustache.py:254-297)."""
    sep = get_sep(f)
    native = _parse_contacts_native(f, sep, chromosome)
    if native is not None:
        ncols, p1, p2, cnt = native                                        # read_csv + dropna (+ the is_chr filters)
        if ncols == 5 and len(cnt) == 0:
            print('Could\'t read any interaction for this chromosome!')
            return
        return _finish_text(p1, p2, cnt, distance_in_bp, read_bias(bias, chromosome, res), res)
    import pandas as pd
    df = pd.read_csv(f, sep=sep, header=None)
    df.dropna(inplace=True)
    if df.shape[1] == 5:
        df = df[np.vectorize(is_chr)(df[0], chromosome)]
        if df.shape[0] == 0:
            print('Could\'t read any interaction for this chromosome!')
            return
        df = df[np.vectorize(is_chr)(df[2], chromosome)]
        a, b, cnt = 1, 3, 4
    elif df.shape[1] == 3:
        a, b, cnt = 0, 1, 2
    else:
        raise ValueError("contact text file must have 3 or 5 columns")
    df = df.loc[np.abs(df[a] - df[b]) <= ((distance_in_bp / res + 1) * res), :].copy()
    df[a] //= res
    df[b] //= res
    bias = read_bias(bias, chromosome, res)
    if bias:
        df[cnt] = np.divide(df[cnt], np.vectorize(bias.get)(df[a], 1))
        df[cnt] = np.divide(df[cnt], np.vectorize(bias.get)(df[b], 1))
    df = df.loc[df[cnt] > 0, :]
    x = np.min(df.loc[:, [a, b]], axis=1)
    y = np.max(df.loc[:, [a, b]], axis=1)
    return x, y, np.array(df[cnt])


# --------------------------------------------------------------------------------------------------------------
# normalisation (reference mustache.py:622-686) -- on the GPU, diagonal-major band layout
# --------------------------------------------------------------------------------------------------------------
def normalize_sparse(x, y, v, resolution, distance_in_px):
    """Per-diagonal sliding-window z-score, in place on `v` (host arrays in, host array out), computed on the GPU.
    Returns the per-diagonal weight list like the reference (unused downstream)."""
    from .normalize import normalize_sparse_device
    return normalize_sparse_device(x, y, v, resolution, distance_in_px)


# --------------------------------------------------------------------------------------------------------------
# per-chromosome driver (reference mustache.py:853-942)
# --------------------------------------------------------------------------------------------------------------
def call_loops_coo(x, y, v, res, distance_in_px, octave_values, st, pt, chromosome='n', chromosome2=None,
                   verbose=True, normalized=False, timings=None, distributed=True):
    """regulator's body after the reader: normalise, tile, run every block, de-duplicate the overlaps.
    x, y, v are host arrays (the reference's COO).  Returns the reference's list of [x, y, fdr, sigma]."""
    from .pipeline import ChromosomePipeline
    pipe = ChromosomePipeline(octave_values)
    return pipe.run(x, y, v, res, distance_in_px, st, pt, normalized=normalized, verbose=verbose, timings=timings,
                    distributed=distributed)


def _check_pair(f, chromosome, chromosome2):
    """chromosome2, defaulted; a trans pair on text input ends as in the reference (mustache.py:869-871): request.Raises"""
    from .request import Raises, refuse, trans_input
    if not chromosome2 or chromosome2 == 'n':
        chromosome2 = chromosome
    if chromosome != chromosome2 and trans_input([f]):
        refuse(Raises(trans_input([f])))
    return chromosome2


def call_trans_coo(x, y, v, octave_values, st, pt, verbose=True, label=""):
    """The trans pair's body after the reader (mustache_amd/trans.py rules 2-6): z-score, square tiles with row / column
    origins, the sigma loop and the tail per tile, ownership.  x = bins of the first chromosome, y = bins of the second, v > 0
    (host arrays or device tensors).  Returns [[x, y, fdr, sigma], ...] sorted by (x, y)."""
    from .trans import call_trans_coo as _call
    return _call(x, y, v, octave_values, st, pt, verbose=verbose, label=label)


def read_contacts(f, norm_method, CHRM_SIZE, res, distance_filter, bias, chromosome, chromosome2, verbose=True,
                  packed=False, part=(0, 1), device=None, balance=None, pairs_zero_based=False, downsample=None, seed=0):
    """The reading half of regulator() (reference mustache.py:866-889): host I/O only, so main() can fetch the next
    chromosome while the GPU works on the current one.  Returns (x, y, v, res) or None when nothing was read.
    packed=True: a `.hic` file read by the native reader comes back as hicfile.PackedContacts (12 bytes per record, what
    the GPU loader takes) instead of the int64 / float64 triple.
    balance="ICE" or "NEWTON": the map's raw counts are balanced on the GPU (mustache_amd.balance) instead of using a bias file or a
    stored normalisation; the result is always the int64 / float64 triple.
    pairs_zero_based: the position convention of a `.pairs` / `.pairs.gz` file (mustache_amd/pairs.py), which needs `balance`.
    downsample=P, seed=S: the raw map of a `.hic` or pairs file is thinned to the fraction P before the balancing
    (mustache_amd/downsample.py); intra-chromosomal only, and it needs `balance`."""
    chromosome2 = _check_pair(f, chromosome, chromosome2)
    distance_in_bp = distance_filter
    if verbose:
        print("Reading contact map...")
    if chromosome != chromosome2:          # a trans pair: every record of the matrix, no distance limit (trans.py rule 1)
        from .request import balance_on_trans, trans_ranks
        from .trans import TransError, read_trans_contacts
        why = balance_on_trans(balance or None) or trans_ranks(part[1], count=False)
        if why:
            raise TransError(why)
        if downsample is not None:
            raise TransError("--downsample on a run with an inter-chromosomal pair: only intra-chromosomal maps are thinned")
        return read_trans_contacts(f, norm_method, chromosome, chromosome2, res, device=device)
    if balance:
        from .balance import check_request
        check_request(balance, f, bias, norm_method, world=part[1])
    r = read_sample(f, norm_method, CHRM_SIZE, res, distance_in_bp, bias, chromosome, packed=packed, part=part,
                    device=device, balance=balance, pairs_zero_based=pairs_zero_based, verbose=verbose, downsample=downsample,
                    seed=seed)
    if isinstance(r, tuple) and len(r[2]) == 0:
        return None
    return r


def read_raw_sample(f, CHRM_SIZE, res, distance_in_bp, chromosome, device=None, balance=None, pairs_zero_based=False, verbose=True):
    """The raw pixel set of one chromosome on the device, the form mustache_amd/downsample.py thins: a `.hic` file
    (balance.read_hic_raw) or a pairs file (pairs.read_pairs_raw) -> (x int32, dist int32, counts, device, the host reader's
    depth or None), None when the chromosome has no pixel.  balance: the method the balancing that follows will use."""
    from .balance import method_of
    from .pairs import is_pairs
    if not balance:
        from .downsample import DownsampleError
        raise DownsampleError("thinning needs raw integer counts; give balance='ICE' or 'NEWTON'")
    if is_pairs(f):
        from .pairs import read_pairs_raw
        return read_pairs_raw(f, distance_in_bp, chromosome, res, device=device, method=method_of(balance),
                              zero_based=pairs_zero_based, verbose=verbose)
    if not str(f).endswith(".hic"):
        from .downsample import DownsampleError
        from .request import THIN_INPUT
        raise DownsampleError(THIN_INPUT % ("downsample", f))
    from .balance import read_hic_raw
    raw = read_hic_raw(f, CHRM_SIZE, chromosome, res, device=device, method=method_of(balance))
    return None if raw is None else raw + (None,)


def thin_raw(raw, T, seed, sample, chromosome):
    """read_raw_sample's result thinned with the threshold T of downsample.thin_records (one printed line) -> the same tuple
    with the kept pixels and int64 counts, None when nothing is kept"""
    from .downsample import report, thin_records
    xd, dd, counts, dev, host_depth = raw
    (xd, dd, counts), total, kept = thin_records(xd, dd, counts, chromosome, T, seed, sample, dev)
    if host_depth is not None and total != host_depth:
        raise RuntimeError("downsample: the device summed %d contacts of %s, the host reader counted %d" % (total, chromosome, host_depth))
    report(chromosome, sample, total, kept, T, seed)
    if kept == 0:
        print(f'There is no contact in chrmosome {chromosome} to work on.')
        return None
    return xd, dd, counts, dev, host_depth


def thin_and_balance(raw, T, seed, sample, distance_in_bp, chromosome, res, balance):
    """What follows read_raw_sample: the optional thinning (T = the threshold of downsample.thin_records, None: none; one
    printed line), then balance.balance_records_device -> (x, y, v) host arrays, None when nothing is left."""
    import torch
    from .balance import balance_records_device, method_of
    if T is not None:
        raw = thin_raw(raw, T, seed, sample, chromosome)
        if raw is None:
            return None
    xd, dd, counts, dev, _ = raw
    vd = counts if counts.dtype == torch.float32 else counts.to(torch.float64)
    return balance_records_device(xd, dd, vd, distance_in_bp, chromosome, res, dev, method=method_of(balance))


def read_sample(f, norm_method, CHRM_SIZE, res, distance_in_bp, bias, chromosome, packed=True, part=(0, 1), device=None,
                balance=None, pairs_zero_based=False, verbose=True, downsample=None, seed=0, sample=0):
    """One sample's intra-chromosomal records by file type, for read_contacts and diff_mustache.read_pair.  Returns
    (x, y, v, res) host arrays (res: the file's own for `.cool`), possibly empty; hicfile.PackedContacts for a `.hic` file
    when `packed` and the native reader serves it (a rank's share of `part` may be empty and is still returned: every
    rank takes part in the exchange); None when a text reader finds no record of the chromosome.
    balance="ICE" or "NEWTON": the raw counts balanced on the GPU by that method (`.hic` through the native reader whatever MUSTACHE_HIC_BACKEND says,
    text otherwise); the caller has already checked the request (balance.check_request).
    A `.pairs` / `.pairs.gz` file (raw read pairs, mustache_amd/pairs.py) is binned on the GPU and needs `balance`.
    downsample=P (0 < P < 1; `.hic` and pairs input under `balance`): every raw contact is kept with probability P before the
    balancing (mustache_amd/downsample.py), seeded by `seed`; `sample` = 0 or 1 is the sample's place in a two-sample run."""
    from .pairs import is_pairs
    if downsample is not None:
        from .downsample import threshold_of
        raw = read_raw_sample(f, CHRM_SIZE, res, distance_in_bp, chromosome, device=device, balance=balance,
                              pairs_zero_based=pairs_zero_based, verbose=verbose)
        r = None if raw is None else thin_and_balance(raw, threshold_of(downsample), seed, sample, distance_in_bp, chromosome, res,
                                                      balance)
    elif is_pairs(f):
        from .pairs import PairsError, read_pairs_balanced
        if not balance:
            from .request import RAW_PAIRS
            raise PairsError(RAW_PAIRS % f)
        from .balance import method_of
        r = read_pairs_balanced(f, distance_in_bp, chromosome, res, device=device, method=method_of(balance),
                                zero_based=pairs_zero_based, verbose=verbose)
    elif balance:
        from .balance import method_of, read_hic_balanced
        if f.endswith(".hic"):
            r = read_hic_balanced(f, CHRM_SIZE, distance_in_bp, chromosome, res, device=device, method=method_of(balance))
        else:
            r = read_pd_balanced(f, distance_in_bp, chromosome, res, device=device, method=method_of(balance))
    elif f.endswith(".hic"):
        from .readers import hic_backend, read_hic_file, read_hic_packed
        if packed and hic_backend() == "native":
            return read_hic_packed(f, norm_method, CHRM_SIZE, distance_in_bp, chromosome, res, part=part, device=device)
        r = read_hic_file(f, norm_method, CHRM_SIZE, distance_in_bp, chromosome, chromosome, res)
    elif f.endswith(".cool"):
        from .readers import read_cooler
        *r, res = read_cooler(f, distance_in_bp, chromosome, chromosome, norm_method)
    elif f.endswith(".mcool"):
        from .readers import read_mcooler
        r = read_mcooler(f, distance_in_bp, chromosome, chromosome, res, norm_method)
    else:
        r = read_pd(f, distance_in_bp, bias, chromosome, res)
    if r is None:
        return None
    x, y, v = r
    return np.asarray(x), np.asarray(y), np.asarray(v, dtype=np.float64), res


def regulator(f, norm_method, CHRM_SIZE, outdir, bed="", res=5000, sigma0=1.6, s=10, pt=0.1, st=0.88, octaves=2,
              verbose=True, nprocesses=4, distance_filter=2000000, bias=False, chromosome='n', chromosome2=None,
              contacts=None, shard_blocks=True, balance=None, pairs_zero_based=False, downsample=None, seed=0):
    """Loop calling for one chromosome (reference mustache.py:853-942).  `s` is accepted and ignored like in the
    reference (s = 10 is hard-wired at :711); `nprocesses` is ignored: all blocks run as one GPU batch.
    `contacts` (not in the reference): what read_contacts() returned for this chromosome, when the caller read ahead;
    `shard_blocks=False`: in a multi-GPU job this rank runs the whole chromosome alone (whole-genome sharding by chromosome).
    `balance="ICE"` or `"NEWTON"` (not in the reference): balance the raw map on the GPU instead of applying `bias`
    (read_contacts); `pairs_zero_based`: the position convention of `.pairs` input (read_contacts); `downsample=P`, `seed=S`:
    thin the raw map to the fraction P before the balancing (read_contacts)."""
    if contacts is None:
        chromosome2 = _check_pair(f, chromosome, chromosome2)
    elif not chromosome2 or chromosome2 == 'n':            # read already (a pairs file's trans records among them): nothing to refuse
        chromosome2 = chromosome
    octave_values = [sigma0 * (2 ** i) for i in range(octaves)]
    if chromosome != chromosome2:          # chromosome2 = B: the trans pair (A, B), mustache_amd/trans.py
        if contacts is None:
            contacts = read_contacts(f, norm_method, CHRM_SIZE, res, distance_filter, bias, chromosome, chromosome2, verbose,
                                     balance=balance, pairs_zero_based=pairs_zero_based, downsample=downsample, seed=seed)
            if contacts is None:
                return []
        x, y, v, _res = contacts
        return call_trans_coo(x, y, v, octave_values, st, pt, verbose=verbose, label="%s,%s" % (chromosome, chromosome2))
    if contacts is None:
        contacts = read_contacts(f, norm_method, CHRM_SIZE, res, distance_filter, bias, chromosome, chromosome2, verbose,
                                 balance=balance, pairs_zero_based=pairs_zero_based, downsample=downsample, seed=seed)
        if contacts is None:
            return []
    from .hicfile import PackedContacts
    if isinstance(contacts, PackedContacts):
        from .pipeline import ChromosomePipeline
        distance_in_px = int(math.ceil(distance_filter // contacts.res))
        return ChromosomePipeline(octave_values).run_packed(contacts, distance_in_px, st, pt, verbose=verbose,
                                                            distributed=shard_blocks)
    x, y, v, res = contacts
    distance_in_px = int(math.ceil(distance_filter // res))
    return call_loops_coo(x, y, v, res, distance_in_px, octave_values, st, pt, chromosome, chromosome2, verbose=verbose,
                          distributed=shard_blocks)


# --------------------------------------------------------------------------------------------------------------
# CLI (reference mustache.py:52-178, :963-1111): same flags and defaults
# --------------------------------------------------------------------------------------------------------------
def parse_args(args):
    p = argparse.ArgumentParser(description="Check the help flag")
    p.add_argument("-f", "--file", dest="f_path", help="REQUIRED: Contact map", required=False)
    p.add_argument("-d", "--distance", dest="distFilter",
                   help="REQUIRED: Maximum distance (in bp) allowed between loop loci", required=False)
    p.add_argument("-o", "--outfile", dest="outdir", help="REQUIRED: Name of the output file.", required=True)
    p.add_argument("-r", "--resolution", dest="resolution", help="REQUIRED: Resolution used for the contact maps",
                   required=True)
    p.add_argument("-bed", "--bed", dest="bed", help="BED file for HiC-Pro type input", default="", required=False)
    p.add_argument("-m", "--matrix", dest="mat", help="MATRIX file for HiC-Pro type input", default="",
                   required=False)
    p.add_argument("-b", "--biases", dest="biasfile",
                   help="RECOMMENDED: biases calculated by ICE or KR norm for each locus", required=False)
    p.add_argument("-cz", "--chromosomeSize", default="", dest="chrSize_file",
                   help="RECOMMENDED: .hic corresponding chromosome size file.", required=False)
    p.add_argument("-norm", "--normalization", default=False, dest="norm_method",
                   help="RECOMMENDED: Hi-C normalization method (KR, VC,...).", required=False)
    p.add_argument("-st", "--sparsityThreshold", dest="st", type=float, default=0.88,
                   help="OPTIONAL: sparsity threshold, default 0.88 (relax for sparse data, e.g. 0.8).")
    p.add_argument("-pt", "--pThreshold", dest="pt", type=float, default=0.2,
                   help="OPTIONAL: FDR threshold for the output. Default is 0.2")
    p.add_argument("-sz", "--sigmaZero", dest="s_z", type=float, default=1.6,
                   help="OPTIONAL: sigma0 of the scale space. DEFAULT is 1.6.")
    p.add_argument("-oc", "--octaves", dest="octaves", default=2, type=int, help="OPTIONAL: octave count. DEFAULT 2.")
    p.add_argument("-i", "--iterations", dest="s", default=10, type=int,
                   help="OPTIONAL: accepted for compatibility; the reference ignores it as well.")
    p.add_argument("-p", "--processes", dest="nprocesses", default=4, type=int,
                   help="OPTIONAL: accepted for compatibility; blocks are batched on the GPU instead.")
    p.add_argument("-ch", "--chromosome", dest="chromosome", nargs='+', default='n', required=False,
                   help="REQUIRED: chromosome(s) to run on. Optional for cooler files.")
    p.add_argument("-ch2", "--chromosome2", dest="chromosome2", nargs='+', default='n', required=False,
                   help="OPTIONAL: second chromosome of each pair, zipped with -ch (same count).  A pair of two different "
                        "chromosomes is called inter-chromosomally on the GPU (.hic / .cool / .mcool input, one GPU, no "
                        "--balance); a pair of one chromosome runs the intra-chromosomal path.")
    p.add_argument("-v", "--verbose", dest="verbose", type=bool, default=True, help="OPTIONAL: verbosity")
    p.add_argument("--balance", dest="balance", default=None, metavar="ICE|NEWTON",
                   help="OPTIONAL: balance the raw contact map on the GPU (ICE: iterative correction; NEWTON: Knight-Ruiz, "
                        "far fewer passes over the map) instead of -b / -norm; text and .hic input")
    p.add_argument("--trans-all", dest="trans_all", action="store_true",
                   help="OPTIONAL: call inter-chromosomal loops for every unordered pair of the -ch list (without -ch: of "
                        "every chromosome of a .hic / .cool / .mcool file) in shared launches; no intra-chromosomal rows.")
    p.add_argument("--pairs-zero-based", dest="pairs_zero_based", action="store_true",
                   help="OPTIONAL: .pairs / .pairs.gz input only: positions are 0-based (bin = pos // res) instead of the "
                        "format's 1-based ones (bin = (pos - 1) // res)")
    add_downsample_arguments(p)
    p.add_argument("--coarser", dest="coarser", nargs='+', default=None, metavar="R",
                   help="OPTIONAL: further resolutions, integer multiples of -r, to call from the same read and merge into one "
                        "list (mustache_amd/multires.py): .hic and .pairs / .pairs.gz input under --balance, intra-chromosomal "
                        "runs, one GPU")
    p.add_argument("--merge-distance", dest="merge_distance", type=int, default=None, metavar="M",
                   help="OPTIONAL: with --coarser, a coarser loop is dropped when a kept loop lies within M bins of the coarser "
                        "resolution in both coordinates (default 2)")
    p.add_argument("--coarser-genome", dest="coarser_genome", nargs='+', default=None, metavar="R",
                   help="OPTIONAL: with --balance-genome (--trans-all, or -ch A -ch2 B): further resolutions, integer multiples "
                        "of -r, at which the genome's map -- coarsened on the GPU from the one read at -r -- is balanced and "
                        "called as well; each pair's loop lists are merged (--merge-distance)")
    from .balance_genome import add_arguments
    add_arguments(p)
    return p.parse_args(args)


def add_downsample_arguments(p):
    """--downsample, --seed and --downsample-genome of both command lines (mustache_amd/downsample.py)"""
    p.add_argument("--downsample", dest="downsample", type=float, default=None, metavar="P",
                   help="OPTIONAL: keep every raw contact with probability P (0 < P < 1) before --balance: binomial thinning on the "
                        "GPU, .hic and .pairs / .pairs.gz input, intra-chromosomal runs")
    p.add_argument("--seed", dest="seed", type=int, default=None, metavar="S",
                   help="OPTIONAL: the seed of the thinning, a 32-bit unsigned integer (default 0)")
    p.add_argument("--downsample-genome", dest="downsample_genome", type=float, default=None, metavar="P",
                   help="OPTIONAL: with --balance-genome: keep every raw contact of the genome's map (the cis pixels it balances on "
                        "and every inter-chromosomal record) with probability P (0 < P < 1) before the balancing")


def resolve_distance_filter(dist_arg, res, quiet=False):
    """reference mustache.py:996-1015: default and clamps of -d."""
    say = (lambda *a: None) if quiet else print
    distFilter = parseBP(dist_arg)
    if not distFilter:
        if 200 * res >= 2000000:
            distFilter = 200 * res
            say("The distance limit is set to {}bp".format(200 * res))
        elif 2000 * res <= 2000000:
            distFilter = 2000 * res
            say("The distance limit is set to {}bp".format(2000 * res))
        else:
            distFilter = 2000000
            say("The distance limit is set to 2Mbp")
    elif distFilter < 200 * res:
        say("The distance limit is set to {}bp".format(200 * res))
        distFilter = 200 * res
    elif distFilter > 10000 * res:
        say("The distance limit is set to {}bp".format(10000 * res))
        distFilter = 10000 * res
    elif distFilter > 10000000:
        distFilter = 10000000
        say("The distance limit is set to 10Mbp")
    return distFilter


def write_loops(path, chromosome, chromosome2, res, loops, first):
    """reference mustache.py:1081-1103: header once, then one TSV row per loop."""
    if first:
        with open(path, 'w') as out_file:
            out_file.write("BIN1_CHR\tBIN1_START\tBIN1_END\tBIN2_CHROMOSOME\tBIN2_START\tBIN2_END\tFDR\tDETECTION_SCALE\n")
    # the reference writes str() of NumPy scalars; Python ints and repr() of Python floats give the same text (held by
    # tests/test_host_logic.py) without NumPy scalar arithmetic and str() per field: 4 x faster on 13 000 rows
    c1, c2, res = str(chromosome), str(chromosome2), int(res)
    loops = list(loops)
    if loops and all(isinstance(v, (int, np.integer)) for v in loops[0][:2]) and \
            all(isinstance(v, (float, np.float64)) for v in loops[0][2:4]):
        n = len(loops)
        try:
            xs = np.fromiter((lp[0] for lp in loops), dtype=np.int64, count=n).tolist()
            ys = np.fromiter((lp[1] for lp in loops), dtype=np.int64, count=n).tolist()
            qs = np.fromiter((lp[2] for lp in loops), dtype=np.float64, count=n).tolist()
            ss = np.fromiter((lp[3] for lp in loops), dtype=np.float64, count=n).tolist()
            rows = ["%s\t%d\t%d\t%s\t%d\t%d\t%r\t%r\n" % (c1, x * res, (x + 1) * res, c2, y * res, (y + 1) * res, q, sg)
                    for x, y, q, sg in zip(xs, ys, qs, ss)]
        except (TypeError, ValueError):
            rows = None
    else:
        rows = None
    if rows is None:                      # rows of other types: field by field, as the reference spells it
        rows = [c1 + '\t' + str(lp[0] * res) + '\t' + str((lp[0] + 1) * res) + '\t' + c2 + '\t' + str(lp[1] * res) + '\t' +
                str((lp[1] + 1) * res) + '\t' + _scalar_text(lp[2]) + '\t' + _scalar_text(lp[3]) + '\n' for lp in loops]
    with open(path, 'a') as out_file:
        out_file.write("".join(rows))


def _scalar_text(v):
    """str(v) for what a loop row holds: np.float64 / float -> repr(float(v)) (the same text), anything else -> str(v)."""
    return repr(float(v)) if isinstance(v, (float, np.float64)) else str(v)      # str(np.float32) is NOT repr(float(v)): left to str()


def read_ahead(count, fetch):
    """(k, fetch(k)) for k = 0 .. count - 1 in order, fetch(k + 1) running on a reader thread while the caller works on k; what
    fetch raises is re-raised here, at its item's turn"""
    from concurrent.futures import ThreadPoolExecutor

    def guarded(k):
        try:
            return fetch(k)
        except BaseException as e:
            return e

    with ThreadPoolExecutor(max_workers=1) as pool:
        ahead = pool.submit(guarded, 0) if count else None
        for k in range(count):
            got = ahead.result()
            ahead = pool.submit(guarded, k + 1) if k + 1 < count else None
            if isinstance(got, BaseException):
                raise got
            yield k, got


def octave_values(args):
    """-sz / -oc of either command line -> the first sigma of each octave"""
    return [args.s_z * (2 ** i) for i in range(args.octaves)]


def genome_biases_or_error(files, res, request, device=None, pairs_zero_based=False, verbose=True, thinning=None):
    """--balance-genome: each sample's file balanced on its own (`.hic` or, under --pairs-trans, a pairs file), one
    balance.report line each -> their GenomeBias in order; None after the `Error:` line of a run the device's memory cannot hold
    (or of a pairs file without `#chromsize` lines).  request = (method, pixels): request.Plan.genome.
    thinning = (T, seed) (--downsample-genome: each sample is read, thinned with the threshold T and solved in turn), or
    ("match", seed) (--match-depth-genome: both are read, the depths N_1 and N_2 compared, the deeper one thinned, both
    solved, after one line that states both depths), or None; one downsample.report_genome line per thinned sample.  A count
    that is no integer raises downsample.DownsampleError (the command lines' error_line prints it)."""
    from .balance import BalanceError, report
    from .balance_genome import check_solve_memory, genome_depth, read_genome, solve_genome, thin_genome
    from .downsample import match_depth, report_genome
    how, seed = thinning if thinning is not None else (None, 0)
    out = []
    try:
        thresholds, waiting = [how] * len(files), []
        if how == "match":
            waiting = [read_genome(f, res, request[1], device, pairs_zero_based, verbose) for f in files]
            check_solve_memory(waiting)
            depths = [sum(genome_depth(r)) for r in waiting]
            print("depth of the genome: sample 1 holds %d contacts, sample 2 holds %d" % tuple(depths))
            thresholds = match_depth(*depths)
        for k, f in enumerate(files):
            read = waiting.pop(0) if waiting else read_genome(f, res, request[1], device, pairs_zero_based, verbose)
            if thresholds[k] is not None:
                cis, trans = thin_genome(read, thresholds[k], seed, k)
                report_genome(k, cis, trans, thresholds[k], seed)
            gb = solve_genome(read, request[0])
            del read
            report(gb.info, gb.label)
            out.append(gb)
    except BalanceError as e:
        print("Error: %s" % e)
        return None
    return out


def run_trans_all(files, args, res, pairs, caller, device=None, genomes=None):
    """The --trans-all run of one sample or two: pair k's records of every file of `files`, read on a reader thread while pair
    k - 1 joins the batch (read_ahead), are held by `caller` (a trans_genome.PairBatcher over len(files) samples), which emits
    the pairs' rows in pair order.  genomes (the files' balance_genome.GenomeBias, --balance-genome): nothing is read again --
    the pairs' resident records are balanced in shared launches (balance_genome.balanced_batches) and join the batch."""
    from .trans import read_trans_contacts
    if genomes is not None:
        from .balance_genome import balanced_batches
        for per_sample in zip(*(balanced_batches(gb, pairs) for gb in genomes)):
            k = per_sample[0][0]
            caller.hold(k, [records for _, records in per_sample], "%s,%s" % pairs[k])
        return caller.flush()

    def fetch(k):
        got = [read_trans_contacts(f, args.norm_method, pairs[k][0], pairs[k][1], res, device=device) for f in files]
        if len({g[3] for g in got if g is not None}) > 1:
            raise ValueError('Both contact maps should have the same resolution.')
        return [None if g is None else g[:3] for g in got]

    for k, records in read_ahead(len(pairs), fetch):
        if args.verbose:
            print("Reading contact map (pair %s,%s)..." % pairs[k])
        caller.hold(k, records, "%s,%s" % pairs[k])
        del records
    caller.flush()


def owned_chromosomes(f, res, pairs, rank, world):
    """Indices of the pairs rank `rank` runs when a multi-GPU run is sharded by chromosome: whole chromosomes, largest
    first, to the least loaded rank (sharding.assign_chromosomes on the chromosome sizes of `f`)."""
    from .readers import chromosome_sizes
    from .sharding import assign_chromosomes
    sizes = chromosome_sizes(f, res)
    weights = [sizes.get(str(c), sizes.get("chr" + str(c).replace("chr", ""), 1)) for c, _ in pairs]
    owner = assign_chromosomes(weights, world)
    return [i for i in range(len(pairs)) if owner[i] == rank]


def call_trans_all(f, args, res, run):
    """mustache's --trans-all run (run_trans_all): rows are written in pair order, the header with the first pair's"""
    import torch
    from .trans_genome import TransGenomeCaller
    device = torch.device("cuda", torch.cuda.current_device())
    genomes = None
    if run.genome is not None:
        genomes = genome_biases_or_error([f], res, run.genome, device, args.pairs_zero_based, args.verbose,
                                         thinning=getattr(args, "genome_thinning", None))
        if genomes is None:
            return
    state = {"first": True, "t0": time.time()}

    def emit(k, o):
        chromosome, chromosome2 = run.trans[k]
        print("{0} loops found for chrmosome pair={1},{2}, fdr<{3} in {4}sec".format(
            len(o), chromosome, chromosome2, args.pt, "%.2f" % (time.time() - state["t0"])))
        if state["first"] or o:
            write_loops(args.outdir, chromosome, chromosome2, res, o, first=state["first"])
            state["first"] = False
        state["t0"] = time.time()

    caller = TransGenomeCaller(octave_values(args), args.st, args.pt, emit, verbose=args.verbose)
    run_trans_all([f], args, res, run.trans, caller, device, genomes)


def call_cis_pairs(f, args, res, pairs, balance, distFilter, rank, world, device, start_time, new_pipeline):
    """The intra-chromosomal pairs of a mustache run.  Returns None when the rows are written (by rank 0, chromosome by
    chromosome), and {pair index: rows} of this rank's chromosomes when a multi-GPU run is sharded by chromosome (main gathers).
    new_pipeline(): the ChromosomePipeline of a run that batches several chromosomes, made when the first one is at hand."""
    chrSize_in_bp = False
    if args.chrSize_file:
        import pandas as pd
        csz = pd.read_csv(args.chrSize_file, header=None, sep='\t')
        chrSize_in_bp = {"chr" + str(csz.iloc[i, 0]).replace('chr', ''): csz.iloc[i, 1] for i in range(csz.shape[0])}
    biasf = args.biasfile if args.biasfile else False
    # Multi-GPU: a single chromosome (or fewer chromosomes than GPUs) is sharded by BLOCKS, every rank reading the same
    # input; a whole-genome run is sharded by CHROMOSOME (largest first, sharding.assign_chromosomes), each rank reading and
    # running only its own -- small chromosomes would otherwise be cut into launches of a few blocks per GPU.
    by_chromosome = world > 1 and len(pairs) >= world
    mine = owned_chromosomes(f, res, pairs, rank, world) if by_chromosome else list(range(len(pairs)))

    def fetch(k):                            # on the reader thread: it must upload to THIS thread's device, not to GPU 0
        chromosome, chromosome2 = pairs[mine[k]]
        CHRM_SIZE = chrSize_in_bp["chr" + str(chromosome).replace('chr', '')] if chrSize_in_bp else False
        from ._lib import stage
        with stage("read %s" % chromosome):
            return read_contacts(f, args.norm_method, CHRM_SIZE, res, distFilter, biasf, chromosome, chromosome2,
                                 verbose=args.verbose, packed=True, part=(0, 1) if by_chromosome else (rank, world),
                                 device=device, balance=balance, pairs_zero_based=args.pairs_zero_based,
                                 downsample=args.downsample, seed=args.seed or 0)

    results = {}

    def emit(i, o):
        nonlocal start_time
        chromosome, chromosome2 = pairs[i]
        print("{0} loops found for chrmosome={1}, fdr<{2} in {3}sec".format(
            len(o), chromosome, args.pt, "%.2f" % (time.time() - start_time)))
        if args.verbose:
            # beside the reference's line (mustache.py:1075-1076): what the GPU stage did -- blocks, Mpix, the fused kernel's time
            from .pipeline import LAST_RUN, run_summary
            line = run_summary()
            if line:
                print(line)
                LAST_RUN.clear()
        if by_chromosome:
            results[i] = o
        elif rank == 0 and (i == 0 or o):
            write_loops(args.outdir, chromosome, chromosome2, res, o, first=(i == 0))
        start_time = time.time()

    # Several chromosomes on this rank (a whole-genome run): their normalised bands are collected in HBM and ALL their
    # blocks go through one sequence of launches (pipeline.run_genome) -- same loops as chromosome by chromosome, without
    # the launch-bound tail of 5-31 blocks per chromosome.  pipeline.GenomeBatcher bounds the bands held at once.
    batched = len(mine) > 1 and (world == 1 or by_chromosome)
    from .pipeline import GenomeBatcher
    pipe = None
    genome = GenomeBatcher(lambda: pipe.device, lambda bands, ns, dpx: pipe.run_genome(bands, ns, dpx, args.st, args.pt),
                           lambda band, n, dpx: pipe.run_band(band, n, dpx, args.st, args.pt, distributed=False), emit)

    # the next chromosome is read (host I/O; the native .hic reader and pandas release the GIL) while the GPU works on
    # the current one -- the reference reads and computes strictly in turn (mustache.py:1057-1080)
    for k, contacts in read_ahead(len(mine), fetch):
        i = mine[k]
        chromosome, chromosome2 = pairs[i]
        if not batched:
            emit(i, [] if contacts is None else regulator(
                f, args.norm_method, False, args.outdir, bed=args.bed, res=getattr(contacts, "res", None) or contacts[3],
                sigma0=args.s_z, s=args.s, verbose=args.verbose, pt=args.pt, st=args.st, distance_filter=distFilter,
                nprocesses=args.nprocesses, bias=biasf, chromosome=chromosome, chromosome2=chromosome2,
                octaves=args.octaves, contacts=contacts, shard_blocks=not by_chromosome))
            continue
        if contacts is None:
            genome.skip(i)
            continue
        if pipe is None:
            pipe = new_pipeline()
        from .hicfile import PackedContacts
        is_packed = isinstance(contacts, PackedContacts)
        res_c = contacts.res if is_packed else contacts[3]
        dpx = int(math.ceil(distFilter // res_c))
        if args.verbose:
            print("Normalizing contact map...")
        if is_packed:
            band, n = pipe.normalized_band_packed(contacts, dpx)
        else:
            band, n = pipe.normalized_band(contacts[0], contacts[1], contacts[2], res_c, dpx)
        del contacts
        genome.add(i, band, n, dpx, band.numel() * 8)
        del band                          # the batcher's reference is the only one: run_genome releases it as it copies
    genome.flush()
    return results if by_chromosome else None


def call_multires(f, args, res, coarser, pairs, balance, device):
    """The --coarser run (mustache_amd/multires.py): per chromosome one read of the raw pixel set at -r -- the next
    chromosome's on a reader thread meanwhile --, one thinning under --downsample, then for -r and each coarser resolution in
    ascending order the coarsening (factor > 1), the balancing and the call, each with the distance limit a run at that
    resolution resolves; the merged lists are written chromosome by chromosome."""
    from .balance import balance_records_device, method_of
    from .downsample import threshold_of
    from .multires import MERGE_DISTANCE, coarsen_records, merge_loops, report
    import torch
    resolutions = [res] + list(coarser)
    limits = [resolve_distance_filter(args.distFilter, R) for R in resolutions]
    M = MERGE_DISTANCE if args.merge_distance is None else args.merge_distance
    T = None if args.downsample is None else threshold_of(args.downsample)
    chrSize_in_bp = False
    if args.chrSize_file:
        import pandas as pd
        csz = pd.read_csv(args.chrSize_file, header=None, sep='\t')
        chrSize_in_bp = {"chr" + str(csz.iloc[i, 0]).replace('chr', ''): csz.iloc[i, 1] for i in range(csz.shape[0])}

    def fetch(k):                            # on the reader thread: the parse (or inflate) and the binning at -r
        chromosome = pairs[k][0]
        CHRM_SIZE = chrSize_in_bp["chr" + str(chromosome).replace('chr', '')] if chrSize_in_bp else False
        from ._lib import stage
        if args.verbose:
            print("Reading contact map...")
        with stage("read %s" % chromosome):
            return read_raw_sample(f, CHRM_SIZE, res, limits[0], chromosome, device=device, balance=balance,
                                   pairs_zero_based=args.pairs_zero_based, verbose=args.verbose)

    for i, raw in read_ahead(len(pairs), fetch):
        start_time = time.time()
        chromosome = pairs[i][0]
        if raw is not None and T is not None:
            raw = thin_raw(raw, T, args.seed or 0, 0, chromosome)
        lists = [[] for _ in resolutions]
        if raw is not None:
            xd, dd, counts, dev, _ = raw
            del raw
            # every coarse pixel set first: a count that is no integer ends the run before anything of the chromosome is called
            sets = [(xd, dd, counts)] + [coarsen_records(xd, dd, counts, R // res, distance_bins=limit // R, device=dev,
                                                         chromosome=chromosome)
                                         for R, limit in zip(resolutions[1:], limits[1:])]
            del xd, dd, counts
            for j, (R, limit) in enumerate(zip(resolutions, limits)):
                x, d, c = sets[j]
                sets[j] = None                   # the raw records of a resolution are released once it is balanced
                contacts = None
                if c.numel():
                    vd = c if c.dtype == torch.float32 else c.to(torch.float64)
                    contacts = balance_records_device(x, d, vd, limit, chromosome, R, dev, method=method_of(balance))
                    del vd
                del x, d, c
                if contacts is not None:
                    lists[j] = regulator(f, args.norm_method, False, args.outdir, bed=args.bed, res=R, sigma0=args.s_z, s=args.s,
                                         verbose=args.verbose, pt=args.pt, st=args.st, distance_filter=limit,
                                         nprocesses=args.nprocesses, chromosome=chromosome, chromosome2=chromosome,
                                         octaves=args.octaves, contacts=contacts + (R,))
                print("{0} loops found for chrmosome={1} at {2} bp, fdr<{3} in {4}sec".format(
                    len(lists[j]), chromosome, R, args.pt, "%.2f" % (time.time() - start_time)))
                start_time = time.time()
        kept = merge_loops(lists, resolutions, M)
        for j, R in enumerate(resolutions):
            if j:
                report(chromosome, R, len(kept[j]), len(lists[j]), M)
            if kept[j] or (i == 0 and j == 0):
                write_loops(args.outdir, chromosome, chromosome, R, kept[j], first=(i == 0 and j == 0))


def call_trans_multires(f, args, res, coarser, run, device):
    """The --coarser-genome run (mustache_amd/multires.py), for --trans-all and for -ch A -ch2 B: the genome is read once at
    -r and thinned once under --downsample-genome; EVERY coarse GenomeRead is derived from the fine one before anything is
    solved, so that a count that is no integer or a memory refusal ends the run before anything is called or written; then for
    -r and each coarser resolution in ascending order the genome is balanced (one balance.report line) and the run's pairs
    are called from the balanced records in shared launches; at the end each pair's lists are merged and written in pair
    order."""
    from .balance import BalanceError, report as balance_report
    from .balance_genome import balanced_batches, coarsen_genome, read_genome, solve_genome, thin_genome
    from .downsample import report_genome
    from .multires import MERGE_DISTANCE, merge_loops, report
    from .trans_genome import TransGenomeCaller
    resolutions = [res] + list(coarser)
    M = MERGE_DISTANCE if args.merge_distance is None else args.merge_distance
    pairs = list(run.trans)
    thinning = getattr(args, "genome_thinning", None)
    try:
        fine = read_genome(f, res, run.genome[1], device, args.pairs_zero_based, args.verbose)
        if thinning is not None:
            cis, trans = thin_genome(fine, thinning[0], thinning[1], 0)
            report_genome(0, cis, trans, thinning[0], thinning[1])
        reads = [fine] + [coarsen_genome(fine, R // res) for R in coarser]
        del fine
        lists = [[[] for _ in resolutions] for _ in pairs]
        for j, R in enumerate(resolutions):
            gb = solve_genome(reads[j], run.genome[0])
            reads[j] = None                      # the raw records of a resolution leave as its pairs are applied
            balance_report(gb.info, gb.label)
            state = {"t0": time.time()}

            def emit(k, o):
                lists[k][j] = o
                print("{0} loops found for chrmosome pair={1},{2} at {3} bp, fdr<{4} in {5}sec".format(
                    len(o), pairs[k][0], pairs[k][1], R, args.pt, "%.2f" % (time.time() - state["t0"])))
                state["t0"] = time.time()

            caller = TransGenomeCaller(octave_values(args), args.st, args.pt, emit, verbose=args.verbose)
            for k, records in balanced_batches(gb, pairs):
                caller.hold(k, [records], "%s,%s" % pairs[k])
            caller.flush()
            del gb, caller
    except BalanceError as e:
        print("Error: %s" % e)
        return None
    first = True
    for k, (chromosome, chromosome2) in enumerate(pairs):
        kept = merge_loops(lists[k], resolutions, M)
        for j, R in enumerate(resolutions):
            if j:
                report("%s,%s" % (chromosome, chromosome2), R, len(kept[j]), len(lists[k][j]), M)
            if kept[j] or first:
                write_loops(args.outdir, chromosome, chromosome2, R, kept[j], first=first)
                first = False


def call_trans_pairs(f, args, res, run, distFilter, device):
    """The inter-chromosomal pairs of a mustache run (mustache_amd/trans.py), one by one in pair order after every
    intra-chromosomal pair; the header is written with the run's first pair's rows."""
    biasf = args.biasfile if args.biasfile else False
    first = not run.cis
    gbias = None
    if run.genome is not None:               # --balance-genome: every matrix is read once, here; the pairs are called from it
        from .balance_genome import balanced_pair
        gbias = genome_biases_or_error([f], res, run.genome, device, args.pairs_zero_based, args.verbose,
                                       thinning=getattr(args, "genome_thinning", None))
        if gbias is None:
            return
    for chromosome, chromosome2 in run.trans:
        start_time = time.time()
        if gbias is not None:
            contacts = balanced_pair(gbias[0], chromosome, chromosome2)
            if contacts is None:
                print("There is no contact in the chromosome pair %s,%s to work on." % (chromosome, chromosome2))
            else:
                contacts = contacts + (res,)
        else:
            contacts = read_contacts(f, args.norm_method, False, res, distFilter, biasf, chromosome, chromosome2,
                                     verbose=args.verbose, device=device)
        o = [] if contacts is None else regulator(
            f, args.norm_method, False, args.outdir, res=contacts[3], sigma0=args.s_z, verbose=args.verbose, pt=args.pt,
            st=args.st, distance_filter=distFilter, chromosome=chromosome, chromosome2=chromosome2, octaves=args.octaves,
            contacts=contacts)
        print("{0} loops found for chrmosome pair={1},{2}, fdr<{3} in {4}sec".format(
            len(o), chromosome, chromosome2, args.pt, "%.2f" % (time.time() - start_time)))
        if first or o:
            write_loops(args.outdir, chromosome, chromosome2, res, o, first=first)
            first = False


@error_line
def main(argv=None):
    start_time = time.time()
    args = parse_args(sys.argv[1:] if argv is None else argv)
    from .request import coarser_genome_resolutions, coarser_resolutions, genome_thinning_of, plan, refuse, request_of
    from .sharding import init_from_env
    rank, world = init_from_env()       # multi-GPU: blocks of each chromosome are sharded, rank 0 writes the TSV
    print("\n")
    f = args.mat if args.bed and args.mat else args.f_path
    res = parseBP(args.resolution)
    asked = request_of(args, [f], [(args.biasfile, "Couldn't find specified bias file")], "-b", world, text_pair_raises=True)
    run = plan(asked, res)
    if isinstance(run, str):
        return refuse(run)
    args.genome_thinning = genome_thinning_of(asked)
    coarser_genome = coarser_genome_resolutions(asked, res)
    if coarser_genome:                   # plan() has refused every run but a single-rank --balance-genome run of trans pairs
        import torch
        from .multires import MultiresError
        try:
            return call_trans_multires(f, args, res, coarser_genome, run, torch.device("cuda", torch.cuda.current_device()))
        except MultiresError as e:
            print("Error: %s" % e)
            return None
    if run.trans_all:
        return call_trans_all(f, args, res, run)
    coarser = coarser_resolutions(asked, res)
    if coarser:                          # plan() has refused every run but a single-rank, intra-chromosomal --balance run
        import torch
        from .multires import MultiresError
        try:
            return call_multires(f, args, res, coarser, run.cis, run.balance, torch.device("cuda", torch.cuda.current_device()))
        except MultiresError as e:
            print("Error: %s" % e)
            return None
    distFilter = resolve_distance_filter(args.distFilter, res)
    try:
        import torch
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    except ImportError:
        device = None
    def new_pipeline():
        from .engine import settle_gc
        from .pipeline import ChromosomePipeline
        pipe = ChromosomePipeline(octave_values(args))
        settle_gc()                       # the command-line process only; the library leaves the collector alone
        return pipe

    results = call_cis_pairs(f, args, res, run.cis, run.balance, distFilter, rank, world, device, start_time, new_pipeline)
    call_trans_pairs(f, args, res, run, distFilter, device)
    if results is not None:
        # one gather of (chromosome index, x, y, fdr, sigma) records; rank 0 writes the chromosomes in their order
        from .sharding import gather_chromosome_rows
        per_chromosome = gather_chromosome_rows(results, len(run.cis), 4)
        for i, rows in enumerate(per_chromosome or []):
            o = [[np.int64(a), np.int64(b), np.float64(q), np.float64(sg)] for a, b, q, sg in rows]
            if i == 0 or o:
                write_loops(args.outdir, run.cis[i][0], run.cis[i][1], res, o, first=(i == 0))



if __name__ == '__main__':
    main()
