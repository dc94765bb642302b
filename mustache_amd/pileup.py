"""Aggregate peak analysis (APA) of a loop list on the GPU: the map piled up around every loop of a Mustache TSV, with
Juicer APA's names and defaults (w = 10, q = 6, n = 30).  `python -m mustache_amd.pileup`, `pileup()` / `pileup_band()` in
Python.  tests/pileup_reference.py restates the arithmetic in NumPy.

Rules:
  * Loop list: any TSV Mustache writes (`.tsv`, `.loop1`, `.diffloop1`, ...); columns 1-6 are read, later ones are kept as
    they are.  An anchor's bin is ((start + end) // 2) // res, so a list from another resolution piles up on this map; the
    two anchors are taken as (x, y) = (min, max).  Chromosome names match with or without a `chr` prefix.
  * Status of every row: `trans` (two chromosomes), `no_chrom` (not selected, or not in the map), `short` (y - x < n_min),
    `long` (-x given and y - x > x_max), `off_map` (an anchor >= n), `used` otherwise.
  * Per chromosome: D = max(y - x) + 2w over its kept loops; the map is read with the distance limit D * res (not the
    caller's -d clamp ladder) into the RAW band (not normalised) with D + 1 used rows; n is the band width as the caller has it.
  * Valid bins: touched by a non-zero pixel (i, j), |i - j| <= D.  E[d] = sum band[d, i] / #{i : i and i + d valid,
    i + d < n} over i with both ends valid; 0 when the count is 0.
  * Windows: cell [a + w, b + w] = pixel (x + a, y + b), a, b in [-w, w], read at (min, max) below the diagonal; NaN off the
    chromosome (index < 0 or >= n), excluded from every sum and count.  obs = band value, oe = obs / E[distance] (NaN where
    E is 0).
  * Aggregate: the loops sorted by (x, y), per cell the sum and the non-NaN count of obs and oe (chunks of 512 loops added in
    chunk order); the genome-wide aggregate adds the chromosome partials in the order the chromosomes ran.  Bit-identical
    under any permutation of the input rows and from run to run.
  * Metrics on M = sum / count: corners q x q, rows = a index, columns = b index; LL = rows 2w-q+1 .. 2w, columns 0 .. q-1
    (nearest the diagonal), UL, UR, LR alike; c = M[w, w]; P2X = c / mean(X); ZscoreLL = (c - mean LL) / std LL (population);
    P2M = c / mean(M without the centre).  Per loop: P2LL = centre / mean of its own non-NaN LL cells (NaN when there is none
    or the mean is 0).
Not claimed: agreement with Juicer's own output.

Device work (mustache_amd/csrc/mst_pileup.hip): valid flags and E (two reads of the band), the windows with each loop's
centre and P2LL, and the reduce; one host wait per chromosome, when the aggregates come back.

Inter-chromosomal lists (`--trans`, `pileup(..., trans=True)`, `pileup_trans_records()`; tests/pileup_trans_reference.py
restates the rules).  Without the switch nothing changes: rows with two chromosomes keep the status `trans`.
  * Rows: a row with one chromosome gets the status `cis`.  A row with two belongs to the unordered pair {chr1, chr2}; the
    pair's orientation (A, B) is that of its first row in the file, and a row written (B, A) has its anchors swapped.  Bins:
    a = ((start + end) // 2) // res on A, b likewise on B -- no min / max across chromosomes.  -ch keeps the pairs whose two
    chromosomes are both in the list; the other rows get `no_pair`.  Pairs run in order of first appearance.  -n / -x are
    refused: there is no distance.
  * Map: trans.read_trans_contacts(f, norm, A, B, res) -- what the trans caller has before its z-score (trans.py rule 1: v > 0
    and finite, divided by the file's vectors); n1 = max x + 1, n2 = max y + 1; no z-score.  A pair without a record, or not in
    the file, gives its rows `no_pair`; a row with a >= n1 or b >= n2 is `off_map`; every other row is `used`.  Text input,
    --balance, -b and `.hic` files of version 6 are refused as the trans caller refuses them.
  * A pixel that occurs more than once among the records takes the largest of its values (an order-free rule).
  * Row i of A is valid when some record has x = i, column j of B when some record has y = j.  E = (sum of v over ALL records,
    a repeated pixel's every record counted) / (#valid rows * #valid columns): one scalar per pair, 0 when the product is 0.
    The sum is exact (csrc/mst_exact_sum.h: one rounding, equal to math.fsum of the records in any order).
  * Windows: cell [da + w][db + w] = pixel (a + da, b + db); NaN when an index is < 0, or >= n1 on the A axis or >= n2 on the B
    axis; 0.0 where the map has no record.  oe = obs / E, NaN where E is 0 or obs is NaN.  Per loop: the obs centre, the oe
    centre and P2LL with the cis definition (the same row and column index ranges).  In a trans window no corner is nearer a
    diagonal than another: the four corners are equivalent by symmetry, and "LL" names an index range only.
  * Aggregate: the loops sorted by (a, b), the same reduce with the same chunks of 512; genome-wide = the pair partials added
    in run order; the same metrics().  Bit-identical under any permutation of the records and of the rows.
Device work (mustache_amd/csrc/mst_pileup_trans.hip): one pass over the pair's records finds the valid rows and columns, the
exact total and the window cells together; one host wait per pair.

Genome mode (`--trans --balance-genome ICE|NEWTON [--balance-pixels all|inter] [--pairs-trans]`, `pileup(..., trans=True,
balance_genome=...)`, `pileup_trans_batch()`): the lists the callers write from a raw `.hic` file or a pairs file, piled up on
the map they were called from.  The rows, the windows, E, the aggregate and the files are the trans rules above; what differs:
  * Map of a pair (A, B): the genome-balanced records the trans caller has before its z-score -- GenomeBias.records(A, B)
    through mst_balance_apply_pairs, the records with v' > 0.  The genome is read and balanced ONCE for the run
    (balance_genome.read_genome, solve_genome: one `... balancing of the genome (... pixels)` line), on every chromosome of the
    file whichever pairs the list names; its memory refusal is balance_genome's.
  * Dimensions: n1 = n_A, n2 = n_B of the genome layout (length // res + 1, GenomeBias.bins), known on the host before anything
    runs -- NOT max x + 1 as above: under --balance-genome the chromosome's extent is known, so NaN means "off the
    chromosome".  E does not depend on the choice.
  * Statuses: `off_map` when a >= n_A or b >= n_B, decided on the host before the launch; `no_pair` when a chromosome of the
    pair is not in the file, when the pair has no raw record, or when none of its records counts after the balancing (its
    `kept` comes back 0: the pair's device result is discarded and its partial is the empty one).
  * Pairs run in order of first appearance; the genome-wide aggregate adds the pair partials in that order on the host.
  * Batches: consecutive pairs until their raw records reach balance_genome.APPLY_BATCH_RECORDS (balanced_segments), cut
    earlier where the windows of their loops (16 (2w+1)^2 bytes per loop) would exceed WINDOW_SHARE of the device's free
    memory; a single pair whose windows do not fit is refused with both numbers.  One host wait per batch: one concatenated
    copy carries every pair's aggregate, loop statistics, E and kept.
  * Refused: --balance-genome without --trans, with --balance, -b or -norm other than NONE, on `.cool` / `.mcool` / text input;
    --balance-pixels without --balance-genome; a pairs file without --pairs-trans; --pairs-trans without --balance-genome or
    on another input; --pairs-zero-based without --pairs-trans (no other pile-up bins a pairs file with it).  Each is one `Error:` line before anything is read.
Device work (mustache_amd/csrc/mst_pileup_trans_batch.hip): mst_pileup_trans_batch is mst_pileup_trans_windows for P pairs in
five launches -- a record whose v' is not > 0 is skipped in the pass, so the balanced records go in without a compaction --
and mst_pileup_reduce_segmented the reduce for P pairs in two; every pair's values have the bits the single-pair entry points
give on that pair alone.

Enrichment (`--enrich [--peak P] [--min-enrichment T]`, `peak=P` on pileup() / pileup_band() / pileup_trans_records() /
pileup_trans_batch(); tests/pileup_enrich_reference.py restates the rules).  Every used loop against its own local background,
HiCCUPS's four neighbourhoods, in all three modes above.  Without the switch (`peak=None`) nothing is launched and nothing changes.
  * Parameters: w, the window half-width above, and the peak half-width p, 0 <= p < w (default 2).
  * Cell (a, b), |a|, |b| <= w, is the pixel (x + a, y + b) as above.  The peak box is |a| <= p and |b| <= p.  The
    neighbourhoods, in the fixed order DONUT, LL, H, V:
      DONUT  outside the peak box, a != 0 and b != 0;
      LL     1 <= a <= w and -w <= b <= -1, outside the peak box (the side nearer the diagonal, as the LL corner);
      H      |a| <= 1 and p < |b| <= w;
      V      |b| <= 1 and p < |a| <= w.
  * A cell counts when its obs is not NaN and its expected value e is not 0.  cis: e = E[|(y + b) - (x + a)|], and that distance
    must be <= D.  trans: e is the pair's scalar E.
  * Per loop and neighbourhood N, over the counted cells: S_o = sum obs, S_e = sum e, cnt = their number.
    EXP_N = E_centre * S_o / S_e (E_centre = E[y - x], or the pair's E), NaN when cnt = 0, S_e = 0 or the obs centre is NaN.
    FE_N = obs centre / EXP_N, NaN when EXP_N is 0 or NaN.  FE_MIN = the smallest of the four, NaN when any of them is NaN.
  * The aggregate, on the host, per neighbourhood: apa_oe[w, w] / mean of apa_oe over the neighbourhood's non-NaN cells (NaN when
    there is none or the mean is 0), for every chromosome or pair and for the genome-wide pile-up.
  * Files: PREFIX.enrich.tsv (each row as read, then STATUS OBS_CENTER E_CENTER EXP_* FE_* FE_MIN; NaN for a row that is not
    `used`), PREFIX.enrich.stats.tsv (one line per chromosome or pair and `all`: the aggregate's four ratios), and with
    --min-enrichment T PREFIX.enriched.tsv: the input's header and the unchanged lines of the `used` rows with FE_MIN >= T (NaN
    fails), a loop list the tools read.  The four files above stay byte for byte what they are without --enrich.
  * Refused, one `Error:` line before anything is read: --peak or --min-enrichment without --enrich; P >= w (or P < 0).
  * Not done: a Poisson p-value (the band holds balanced values, not counts); widening w where a neighbourhood is sparse.
Device work (mustache_amd/csrc/mst_pileup_enrich.hip): mst_pileup_enrich, one wave per loop over the window of obs that is already
resident, the twelve sums per loop; they come back in the one concatenated copy each mode waits for.  The ratios are NumPy's.
"""
import argparse
import math
import os
import sys

import numpy as np

MAX_W = 64
CORNERS = ("LL", "UL", "UR", "LR")
METRICS = ("P2LL", "P2UL", "P2UR", "P2LR", "ZscoreLL", "P2M")
STATS_HEADER = "CHR\tROWS_IN\tLOOPS_USED\t" + "\t".join(METRICS) + "\tOE_P2LL\n"
LOOP_COLUMNS = ("STATUS", "OBS_CENTER", "OE_CENTER", "P2LL")
DEFAULT_HEADER = "BIN1_CHR\tBIN1_START\tBIN1_END\tBIN2_CHROMOSOME\tBIN2_START\tBIN2_END\tFDR\tDETECTION_SCALE"
NEIGHBOURHOODS = ("DONUT", "LL", "H", "V")
DEFAULT_PEAK = 2
ENRICH_COLUMNS = ("STATUS", "OBS_CENTER", "E_CENTER") + tuple("EXP_" + n for n in NEIGHBOURHOODS) \
    + tuple("FE_" + n for n in NEIGHBOURHOODS) + ("FE_MIN",)
ENRICH_STATS_HEADER = "CHR\tLOOPS_USED\t" + "\t".join("OE_P2" + n for n in NEIGHBOURHOODS) + "\n"


class PileupError(ValueError):
    """A pile-up request that cannot be honoured."""


def check_window(w, q):
    if not 0 <= int(w) <= MAX_W:
        raise PileupError("window half-width w = %d is outside 0 .. %d (a window holds at most %d cells)"
                          % (w, MAX_W, (2 * MAX_W + 1) ** 2))
    if not 1 <= int(q) <= 2 * int(w) + 1:
        raise PileupError("corner size q = %d is outside 1 .. 2w + 1 = %d" % (q, 2 * int(w) + 1))


def check_peak(w, p):
    if not 0 <= int(p) < int(w):
        raise PileupError("peak half-width p = %d is outside 0 .. w - 1 = %d: the neighbourhoods lie between the peak box and "
                          "the window's edge" % (p, int(w) - 1))


# ----------------------------------------------------------------------------------------------------------------------
# metrics (host, on the (2w+1)^2 mean map)
# ----------------------------------------------------------------------------------------------------------------------
def corner_slices(w, q):
    near, far = slice(0, q), slice(2 * w - q + 1, 2 * w + 1)
    return {"LL": (far, near), "UL": (near, near), "UR": (near, far), "LR": (far, far)}


def mean_map(s, c):
    """sum / count per cell, NaN where the count is 0."""
    s, c = np.asarray(s, np.float64), np.asarray(c, np.float64)
    out = np.full(s.shape, np.nan)
    np.divide(s, c, out=out, where=c > 0)
    return out


def metrics(M, w, q):
    M = np.asarray(M, np.float64)
    c = M[w, w]
    sl = corner_slices(w, q)
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        for name in CORNERS:
            out["P2" + name] = float(c / M[sl[name]].mean())
        ll = M[sl["LL"]]
        out["ZscoreLL"] = float((c - ll.mean()) / ll.std())
        rest = np.delete(M.reshape(-1), w * (2 * w + 1) + w)
        out["P2M"] = float(c / rest.mean()) if rest.size else math.nan
    return out


# ----------------------------------------------------------------------------------------------------------------------
# enrichment of every loop over its local background (host; the sums are the device's, mst_pileup_enrich)
# ----------------------------------------------------------------------------------------------------------------------
def enrichment_masks(w, p):
    """bool [4, 2w+1, 2w+1]: the cells of DONUT, LL, H, V (rows = a index, columns = b index)."""
    w, p = int(w), int(p)
    check_peak(w, p)
    off = np.arange(-w, w + 1)
    a, b = off[:, None], off[None, :]
    outside = (np.abs(a) > p) | (np.abs(b) > p)
    return np.stack([outside & (a != 0) & (b != 0), outside & (a >= 1) & (b <= -1),
                     (np.abs(a) <= 1) & (np.abs(b) > p), (np.abs(b) <= 1) & (np.abs(a) > p)])


def enrich_windows(obs, w, p, E=None, xs=None, ys=None, e_loop=None):
    """sums, a device float64 [L, 4, 3] tensor (S_o, S_e, cnt per neighbourhood), of the windows `obs` (device float64
    [L, 2w+1, 2w+1]).  cis: E (device float64 [D + 1]) with xs, ys (device int64 [L]); trans: e_loop (device float64 [L]).
    L = 0 launches nothing."""
    import torch
    from . import _lib
    from ._lib import ptr as _ptr, stream as _stream, require_gpu
    lib = require_gpu()
    L = int(obs.shape[0])
    cis = E is not None
    with torch.cuda.device(obs.device):
        sums = torch.empty((L, 4, 3), dtype=torch.float64, device=obs.device)
        _lib.check(lib.mst_pileup_enrich(_ptr(obs) if L else None, L, int(w), int(p), _ptr(E) if cis else None,
                                         int(E.numel()) - 1 if cis else 0, _ptr(xs) if cis and L else None,
                                         _ptr(ys) if cis and L else None, None if cis else (_ptr(e_loop) if L else None),
                                         _ptr(sums) if L else None, _stream()))
    return sums


def enrichment(sums, centre_obs, centre_e):
    """(EXP [L, 4], FE [L, 4], FE_MIN [L]) of the sums [L, 4, 3] mst_pileup_enrich wrote, each loop's obs centre and its E_centre."""
    sums = np.asarray(sums, np.float64).reshape(-1, 4, 3)
    so, se, cnt = np.ascontiguousarray(sums.transpose(2, 1, 0))          # each [4, L] with unit stride: a third of the time
    c = np.asarray(centre_obs, np.float64).reshape(1, -1)
    e = np.asarray(centre_e, np.float64).reshape(1, -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        exp = e * so / se
        exp[(cnt == 0) | (se == 0) | np.isnan(c)] = np.nan
        fe = c / exp                                     # a NaN EXP hands itself on
        fe[exp == 0] = np.nan
    fe_min = np.minimum(np.minimum(fe[0], fe[1]), np.minimum(fe[2], fe[3]))          # np.minimum hands a NaN on
    return exp.T, fe.T, fe_min


def aggregate_enrichment(apa_oe, w, p):
    """float64 [4]: apa_oe[w, w] / mean of apa_oe over each neighbourhood's non-NaN cells; NaN when there is none or the mean is 0."""
    M = np.asarray(apa_oe, np.float64)
    out = np.full(4, np.nan)
    for k, mask in enumerate(enrichment_masks(w, p)):
        cells = M[mask]
        cells = cells[~np.isnan(cells)]
        if cells.size and cells.mean() != 0:
            out[k] = M[int(w), int(w)] / cells.mean()
    return out


def _peak_kw(peak):
    """the keyword a driver hands on: a run without a peak makes the call it has always made"""
    return {} if peak is None else {"peak": peak}


def _enrich_result(sums, centre_obs, centre_e, apa_oe, w, p):
    """the keys a pile-up dict gains under `peak`"""
    exp, fe, fe_min = enrichment(sums, centre_obs, centre_e)
    return {"center_e": np.asarray(centre_e, np.float64), "enrich_sums": np.asarray(sums, np.float64).reshape(-1, 4, 3),
            "enrich_exp": exp, "enrich_fe": fe, "fe_min": fe_min, "enrich_agg": aggregate_enrichment(apa_oe, w, p)}


# ----------------------------------------------------------------------------------------------------------------------
# the device pile-up of one chromosome
# ----------------------------------------------------------------------------------------------------------------------
def _workspace(lib, n, D, L, w, device):
    import torch
    return torch.empty(max(int(lib.mst_pileup_workspace_bytes(int(n), int(D), int(L), int(w))), 256), dtype=torch.uint8,
                       device=device)


def expected(band, n, D, ws=None):
    """(valid uint8 [n], E float64 [D + 1]) device tensors of a raw band (device, [rows >= D + 1, n])."""
    import torch
    from . import _lib
    from ._lib import ptr as _ptr, stream as _stream, require_gpu
    lib = require_gpu()
    n, D = int(n), int(D)
    if band.dim() != 2 or band.shape[1] != n or band.shape[0] < D + 1 or band.dtype != torch.float64 or not band.is_contiguous():
        raise PileupError("band must be a contiguous float64 [rows >= D + 1, n] tensor (got %s, n %d, D %d)"
                          % (tuple(band.shape), n, D))
    with torch.cuda.device(band.device):
        if ws is None:
            ws = _workspace(lib, n, D, 0, 0, band.device)
        valid = torch.empty(n, dtype=torch.uint8, device=band.device)
        E = torch.empty(D + 1, dtype=torch.float64, device=band.device)
        _lib.check(lib.mst_pileup_expected(_ptr(band), n, int(band.shape[0]), D, _ptr(valid), _ptr(E), _ptr(ws), ws.numel(),
                                           _stream()))
    return valid, E


def windows(band, n, D, E, xd, yd, w, q):
    """(obs, oe [L, 2w+1, 2w+1], loop stats [L, 3] = obs centre, oe centre, P2LL) device tensors; xd, yd int64 device [L]."""
    import torch
    from . import _lib
    from ._lib import ptr as _ptr, stream as _stream, require_gpu
    lib = require_gpu()
    L, S = int(xd.numel()), 2 * int(w) + 1
    with torch.cuda.device(band.device):
        obs = torch.empty((L, S, S), dtype=torch.float64, device=band.device)
        oe = torch.empty_like(obs)
        st = torch.empty((L, 3), dtype=torch.float64, device=band.device)
        _lib.check(lib.mst_pileup_windows(_ptr(band), int(n), int(band.shape[0]), int(D), _ptr(E), _ptr(xd), _ptr(yd), L, int(w),
                                          int(q), _ptr(obs), _ptr(oe), _ptr(st), _stream()))
    return obs, oe, st


def reduce(obs, oe, order, w, ws):
    """agg [4, (2w+1)^2] device tensor: sum obs, count obs, sum oe, count oe over the windows in `order` (int32 device)."""
    import torch
    from . import _lib
    from ._lib import ptr as _ptr, stream as _stream, require_gpu
    lib = require_gpu()
    S = 2 * int(w) + 1
    with torch.cuda.device(obs.device):
        agg = torch.empty((4, S * S), dtype=torch.float64, device=obs.device)
        _lib.check(lib.mst_pileup_reduce(_ptr(obs), _ptr(oe), _ptr(order), int(order.numel()), int(w), _ptr(agg), _ptr(ws),
                                         ws.numel(), _stream()))
    return agg


def _empty_result(w, q, peak=None):
    S = 2 * w + 1
    z = np.zeros((S, S))
    M = np.full((S, S), np.nan)
    if peak is not None:
        return dict(_empty_result(w, q), **_enrich_result(np.zeros((0, 4, 3)), np.zeros(0), np.zeros(0), M, w, peak))
    return {"valid": None, "expected": None, "obs": None, "oe": None, "sum_obs": z, "count_obs": z.copy(), "sum_oe": z.copy(),
            "count_oe": z.copy(), "apa": M, "apa_oe": M.copy(), "center_obs": np.zeros(0), "center_oe": np.zeros(0),
            "p2ll": np.zeros(0), "metrics": metrics(M, w, q), "metrics_oe": metrics(M, w, q)}


def pileup_band(band, n, D, xs, ys, w=10, q=6, peak=None):
    """The pile-up of one chromosome's raw band (device float64 [rows >= D + 1, n]) around the loops (xs, ys) (bins, host
    arrays or tensors, y - x + 2w <= D).  Returns a dict: "valid", "expected", "obs", "oe" (device tensors), "sum_obs",
    "count_obs", "sum_oe", "count_oe", "apa" (mean obs), "apa_oe" (host [2w+1, 2w+1]), "center_obs", "center_oe", "p2ll"
    (host [L], input order), "metrics" and "metrics_oe" (dicts of METRICS).  L = 0 returns empty aggregates without a launch.
    peak=p adds the enrichment of every loop (the module docstring has the rules): "center_e" (E[y - x], host [L]),
    "enrich_sums" [L, 4, 3], "enrich_exp", "enrich_fe" [L, 4], "fe_min" [L] and "enrich_agg" [4], from one more launch inside the
    same host wait."""
    import torch
    w, q = int(w), int(q)
    check_window(w, q)
    if peak is not None:
        check_peak(w, peak)
    xs = np.asarray(xs.cpu() if isinstance(xs, torch.Tensor) else xs, np.int64).reshape(-1)
    ys = np.asarray(ys.cpu() if isinstance(ys, torch.Tensor) else ys, np.int64).reshape(-1)
    if len(xs) != len(ys):
        raise PileupError("xs and ys differ in length (%d, %d)" % (len(xs), len(ys)))
    L, S = len(xs), 2 * w + 1
    if L == 0:
        return _empty_result(w, q, peak)
    from ._lib import require_gpu
    lib = require_gpu()
    dev = band.device
    with torch.cuda.device(dev):
        ws = _workspace(lib, n, D, L, w, dev)
        valid, E = expected(band, n, D, ws)
        xd = torch.from_numpy(xs).to(dev, non_blocking=True)
        yd = torch.from_numpy(ys).to(dev, non_blocking=True)
        obs, oe, st = windows(band, n, D, E, xd, yd, w, q)
        order = torch.from_numpy(np.lexsort((ys, xs)).astype(np.int32)).to(dev, non_blocking=True)
        agg = reduce(obs, oe, order, w, ws)
        parts = [agg.view(-1), st.view(-1)]
        if peak is not None:
            parts += [enrich_windows(obs, w, peak, E=E, xs=xd, ys=yd).view(-1), E[yd - xd]]
        host = torch.cat(parts).cpu().numpy()                             # the one wait
    agg_h, st_h = host[:4 * S * S].reshape(4, S, S), host[4 * S * S:4 * S * S + 3 * L].reshape(L, 3)
    apa, apa_oe = mean_map(agg_h[0], agg_h[1]), mean_map(agg_h[2], agg_h[3])
    out = {"valid": valid, "expected": E, "obs": obs, "oe": oe, "sum_obs": agg_h[0], "count_obs": agg_h[1],
           "sum_oe": agg_h[2], "count_oe": agg_h[3], "apa": apa, "apa_oe": apa_oe, "center_obs": st_h[:, 0].copy(),
           "center_oe": st_h[:, 1].copy(), "p2ll": st_h[:, 2].copy(), "metrics": metrics(apa, w, q),
           "metrics_oe": metrics(apa_oe, w, q)}
    if peak is not None:
        out.update(_enrich_result(host[-13 * L:-L], out["center_obs"], host[-L:], apa_oe, w, peak))
    return out


def pileup_trans_records(x, y, v, n1, n2, xs, ys, w=10, q=6, peak=None):
    """The pile-up of one inter-chromosomal pair's records (x = bins of A, y = bins of B, v > 0; host arrays or device tensors)
    on the n1 x n2 map around the loops (xs, ys) (bins of A, bins of B).  Returns pileup_band's dict with "expected" the
    scalar E (a float) and "valid" the pair (rows uint8 [n1], columns uint8 [n2]) of device tensors.  L = 0 still finds the
    valid flags and E; N = 0 gives E = 0.  One host wait.  peak=p adds pileup_band's enrichment keys, every cell's e and E_centre
    being the scalar E."""
    import torch
    from . import _lib
    from ._lib import ptr as _ptr, stream as _stream, require_gpu
    w, q, n1, n2 = int(w), int(q), int(n1), int(n2)
    check_window(w, q)
    if peak is not None:
        check_peak(w, peak)
    xs = np.asarray(xs.cpu() if isinstance(xs, torch.Tensor) else xs, np.int64).reshape(-1)
    ys = np.asarray(ys.cpu() if isinstance(ys, torch.Tensor) else ys, np.int64).reshape(-1)
    if len(xs) != len(ys):
        raise PileupError("xs and ys differ in length (%d, %d)" % (len(xs), len(ys)))
    if not (len(x) == len(y) == len(v)):
        raise PileupError("x, y and v differ in length (%d, %d, %d)" % (len(x), len(y), len(v)))
    if n1 < 1 or n2 < 1:
        raise PileupError("a trans map needs n1 >= 1 and n2 >= 1 (got %d x %d)" % (n1, n2))
    lib = require_gpu()
    dev = v.device if isinstance(v, torch.Tensor) and v.is_cuda else torch.device("cuda", torch.cuda.current_device())
    L, S = len(xs), 2 * w + 1
    with torch.cuda.device(dev):
        x = torch.as_tensor(x).to(dev, dtype=torch.int32).contiguous()
        y = torch.as_tensor(y).to(dev, dtype=torch.int32).contiguous()
        v = torch.as_tensor(v).to(dev, dtype=torch.float64).contiguous()
        ws = torch.empty(max(int(lib.mst_pileup_trans_workspace_bytes(n1, n2, L, w)), 256), dtype=torch.uint8, device=dev)
        rows = torch.empty(n1, dtype=torch.uint8, device=dev)
        cols = torch.empty(n2, dtype=torch.uint8, device=dev)
        E = torch.empty(1, dtype=torch.float64, device=dev)
        obs = torch.empty((L, S, S), dtype=torch.float64, device=dev)
        oe = torch.empty_like(obs)
        st = torch.empty((L, 3), dtype=torch.float64, device=dev)
        xd = torch.from_numpy(xs).to(dev, non_blocking=True)
        yd = torch.from_numpy(ys).to(dev, non_blocking=True)
        N = int(v.numel())
        _lib.check(lib.mst_pileup_trans_windows(_ptr(x) if N else None, _ptr(y) if N else None, _ptr(v) if N else None, N, n1, n2,
                                                _ptr(xd) if L else None, _ptr(yd) if L else None, L, w, q, _ptr(rows), _ptr(cols),
                                                _ptr(E), _ptr(obs) if L else None, _ptr(oe) if L else None,
                                                _ptr(st) if L else None, _ptr(ws), ws.numel(), _stream()))
        order = torch.from_numpy(np.lexsort((ys, xs)).astype(np.int32)).to(dev, non_blocking=True)
        agg = reduce(obs, oe, order, w, ws)
        parts = [agg.view(-1), st.view(-1), E]
        if peak is not None:
            parts.insert(2, enrich_windows(obs, w, peak, e_loop=E.expand(L).contiguous()).view(-1))
        host = torch.cat(parts).cpu().numpy()                             # the one wait
    agg_h, st_h = host[:4 * S * S].reshape(4, S, S), host[4 * S * S:4 * S * S + 3 * L].reshape(L, 3)
    apa, apa_oe = mean_map(agg_h[0], agg_h[1]), mean_map(agg_h[2], agg_h[3])
    out = {"valid": (rows, cols), "expected": float(host[-1]), "obs": obs, "oe": oe, "sum_obs": agg_h[0], "count_obs": agg_h[1],
           "sum_oe": agg_h[2], "count_oe": agg_h[3], "apa": apa, "apa_oe": apa_oe, "center_obs": st_h[:, 0].copy(),
           "center_oe": st_h[:, 1].copy(), "p2ll": st_h[:, 2].copy(), "metrics": metrics(apa, w, q),
           "metrics_oe": metrics(apa_oe, w, q)}
    if peak is not None:
        out.update(_enrich_result(host[-1 - 12 * L:-1], out["center_obs"], np.full(L, host[-1]), apa_oe, w, peak))
    return out


def _host_ptr(a):
    """a contiguous host array as the C ABI takes a host table"""
    import ctypes
    return ctypes.c_void_p(a.ctypes.data)


def pileup_trans_batch(x, y, v, seg_off, dims, loops, w=10, q=6, peak=None):
    """pileup_trans_records for P inter-chromosomal pairs in shared launches (csrc/mst_pileup_trans_batch.hip).  x, y, v: the
    pairs' records concatenated (device int32 / int32 / float64, or host arrays; None when there is none), pair p owning
    [seg_off[p], seg_off[p + 1]) -- seg_off a HOST table of P + 1 entries; a record whose v is not > 0 is ignored, so the output of
    mst_balance_apply_pairs goes in unfiltered.  dims: [(n1, n2)] per pair; loops: [(xs, ys)] per pair (host arrays, bins of A
    and of B; either may be empty).  Returns one dict per pair with pileup_trans_records' keys -- "obs", "oe" and "valid" are
    views into the batch's device tensors -- and "kept", the records of the pair that counted.  Every value has the bits
    pileup_trans_records gives on that pair's records with v > 0 alone.  One host wait for the whole batch.  peak=p adds the
    enrichment keys to every pair's dict: one launch over all the windows, each loop's e its own pair's E, gathered on the device."""
    import torch
    from . import _lib
    from ._lib import ptr as _ptr, stream as _stream, require_gpu
    w, q, P = int(w), int(q), len(dims)
    check_window(w, q)
    if peak is not None:
        check_peak(w, peak)
    if len(loops) != P:
        raise PileupError("dims and loops differ in length (%d, %d)" % (P, len(loops)))
    seg = np.ascontiguousarray(seg_off, np.int64).reshape(-1)
    if len(seg) != P + 1:
        raise PileupError("seg_off has %d entries, %d pairs need %d" % (len(seg), P, P + 1))
    n1 = np.ascontiguousarray([d[0] for d in dims], np.int64)
    n2 = np.ascontiguousarray([d[1] for d in dims], np.int64)
    xs = [np.asarray(a, np.int64).reshape(-1) for a, _ in loops]
    ys = [np.asarray(b, np.int64).reshape(-1) for _, b in loops]
    for p in range(P):
        if len(xs[p]) != len(ys[p]):
            raise PileupError("xs and ys of pair %d differ in length (%d, %d)" % (p, len(xs[p]), len(ys[p])))
    loop_off = np.zeros(P + 1, np.int64)
    np.cumsum([len(a) for a in xs], out=loop_off[1:])
    N, L, S = int(seg[-1]) if P else 0, int(loop_off[-1]), 2 * w + 1
    if v is None:
        x = y = np.zeros(0, np.int32)
        v = np.zeros(0, np.float64)
    if not (len(x) == len(y) == len(v) == N):
        raise PileupError("x, y and v hold %d, %d and %d records, seg_off ends at %d" % (len(x), len(y), len(v), N))
    lib = require_gpu()
    dev = v.device if isinstance(v, torch.Tensor) and v.is_cuda else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        x = torch.as_tensor(x).to(dev, dtype=torch.int32).contiguous()
        y = torch.as_tensor(y).to(dev, dtype=torch.int32).contiguous()
        v = torch.as_tensor(v).to(dev, dtype=torch.float64).contiguous()
        lxy = np.concatenate(xs + ys) if L else np.zeros(0, np.int64)
        order = np.concatenate([np.lexsort((ys[p], xs[p])) + loop_off[p] for p in range(P)]).astype(np.int32) if L \
            else np.zeros(0, np.int32)
        lxy_d = torch.from_numpy(lxy).to(dev, non_blocking=True)
        order_d = torch.from_numpy(order).to(dev, non_blocking=True)
        need = max(int(lib.mst_pileup_trans_batch_workspace_bytes(_host_ptr(seg), _host_ptr(n1), _host_ptr(loop_off), P, w)),
                   int(lib.mst_pileup_reduce_segmented_workspace_bytes(_host_ptr(loop_off), P, w)), 256)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        rows = torch.empty(max(int(n1.sum()), 1), dtype=torch.uint8, device=dev)
        cols = torch.empty(max(int(n2.sum()), 1), dtype=torch.uint8, device=dev)
        E = torch.empty(max(P, 1), dtype=torch.float64, device=dev)
        kept = torch.empty(max(P, 1), dtype=torch.int64, device=dev)
        obs = torch.empty((L, S, S), dtype=torch.float64, device=dev)
        oe = torch.empty_like(obs)
        st = torch.empty((L, 3), dtype=torch.float64, device=dev)
        agg = torch.empty((max(P, 1), 4, S * S), dtype=torch.float64, device=dev)
        _lib.check(lib.mst_pileup_trans_batch(
            _ptr(x) if N else None, _ptr(y) if N else None, _ptr(v) if N else None, N, _host_ptr(seg), _host_ptr(n1), _host_ptr(n2),
            _ptr(lxy_d) if L else None, _lib.off(lxy_d, L) if L else None, L, _host_ptr(loop_off), P, w, q, _ptr(rows), _ptr(cols),
            _ptr(E), _ptr(kept), _ptr(obs) if L else None, _ptr(oe) if L else None, _ptr(st) if L else None, _ptr(ws), ws.numel(),
            _stream()))
        _lib.check(lib.mst_pileup_reduce_segmented(_ptr(obs) if L else None, _ptr(oe) if L else None, _ptr(order_d) if L else None,
                                                   L, _host_ptr(loop_off), P, w, _ptr(agg), _ptr(ws), ws.numel(), _stream()))
        parts = [agg.view(-1), st.view(-1), E, kept.view(torch.float64)]
        if peak is not None:                           # e_loop: the E of the pair each loop belongs to
            pair_of = torch.from_numpy(np.repeat(np.arange(P, dtype=np.int64), np.diff(loop_off))).to(dev, non_blocking=True)
            parts.insert(2, enrich_windows(obs, w, peak, e_loop=E[pair_of]).view(-1))
        host = torch.cat(parts).cpu().numpy()                                                         # the one wait
    agg_h = host[:P * 4 * S * S].reshape(P, 4, S, S)
    st_h = host[P * 4 * S * S:P * 4 * S * S + 3 * L].reshape(L, 3)
    E_h, kept_h = host[-2 * P:-P], host[-P:].view(np.int64)
    en_h = host[P * 4 * S * S + 3 * L:P * 4 * S * S + 15 * L].reshape(L, 4, 3) if peak is not None else None
    row_off = np.concatenate([[0], np.cumsum(n1)])
    col_off = np.concatenate([[0], np.cumsum(n2)])
    out = []
    for p in range(P):
        l0, l1 = int(loop_off[p]), int(loop_off[p + 1])
        a = agg_h[p]
        apa, apa_oe = mean_map(a[0], a[1]), mean_map(a[2], a[3])
        out.append({"valid": (rows[int(row_off[p]):int(row_off[p + 1])], cols[int(col_off[p]):int(col_off[p + 1])]),
                    "expected": float(E_h[p]), "kept": int(kept_h[p]), "obs": obs[l0:l1], "oe": oe[l0:l1], "sum_obs": a[0],
                    "count_obs": a[1], "sum_oe": a[2], "count_oe": a[3], "apa": apa, "apa_oe": apa_oe,
                    "center_obs": st_h[l0:l1, 0].copy(), "center_oe": st_h[l0:l1, 1].copy(), "p2ll": st_h[l0:l1, 2].copy(),
                    "metrics": metrics(apa, w, q), "metrics_oe": metrics(apa_oe, w, q)})
        if peak is not None:
            out[-1].update(_enrich_result(en_h[l0:l1], out[-1]["center_obs"], np.full(l1 - l0, E_h[p]), apa_oe, w, peak))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# loop lists
# ----------------------------------------------------------------------------------------------------------------------
def _key(c):
    return str(c).replace("chr", "")


class LoopTable:
    """The rows of a Mustache loop TSV: `header` (without newline), `lines` (each row as read), the six anchor columns."""

    def __init__(self, header, lines, chr1, s1, e1, chr2, s2, e2):
        self.header, self.lines = header, lines
        self.chr1, self.chr2 = chr1, chr2
        self.s1, self.e1 = np.asarray(s1, np.int64), np.asarray(e1, np.int64)
        self.s2, self.e2 = np.asarray(s2, np.int64), np.asarray(e2, np.int64)

    def __len__(self):
        return len(self.lines)

    def bins(self, res):
        """(x, y) = (min, max) of the two anchors' bins, ((start + end) // 2) // res."""
        a = ((self.s1 + self.e1) // 2) // int(res)
        b = ((self.s2 + self.e2) // 2) // int(res)
        return np.minimum(a, b), np.maximum(a, b)


def read_loops(path):
    header, lines, cols = DEFAULT_HEADER, [], [[] for _ in range(6)]
    with open(path) as fh:
        for k, raw in enumerate(fh):
            line = raw.rstrip("\r\n")
            if not line.strip():
                continue
            f = line.split("\t")
            if k == 0 and f[0] == "BIN1_CHR":
                header = line
                continue
            if len(f) < 6:
                raise PileupError("%s: row %d has %d columns, a loop row has at least 6" % (path, k + 1, len(f)))
            lines.append(line)
            for c in range(6):
                cols[c].append(f[c])
    try:
        return LoopTable(header, lines, cols[0], [int(float(v)) for v in cols[1]], [int(float(v)) for v in cols[2]], cols[3],
                         [int(float(v)) for v in cols[4]], [int(float(v)) for v in cols[5]])
    except ValueError as e:
        raise PileupError("%s: an anchor position is not a number (%s)" % (path, e))


def _classify_trans(table, res, chromosomes):
    """classify() in trans mode: (status list, a, b, [(A, B)]) with a = bins on A, b = bins on B in the pair's orientation."""
    a = ((table.s1 + table.e1) // 2) // int(res)
    b = ((table.s2 + table.e2) // 2) // int(res)
    keys = None if not chromosomes else {_key(c) for c in chromosomes}
    pairs, first, status = [], {}, []
    for k in range(len(table)):
        k1, k2 = _key(table.chr1[k]), _key(table.chr2[k])
        if k1 == k2:
            status.append("cis")
        elif keys is not None and not (k1 in keys and k2 in keys):
            status.append("no_pair")
        else:
            if frozenset((k1, k2)) not in first:         # the pair's orientation: that of its first row
                first[frozenset((k1, k2))] = k1
                pairs.append((table.chr1[k], table.chr2[k]))
            if first[frozenset((k1, k2))] != k1:
                a[k], b[k] = b[k], a[k]
            status.append(None)
    return status, a, b, pairs


def classify(table, res, chromosomes=None, n_min=None, x_max=None, trans=False):
    """Statuses before the map is read: (status list, x, y, selected chromosome names).  Rows still eligible have status
    None; `x_max` is in bins; `n_min` = None is the default of 30 bins.  trans=True: (status list, a, b, [(A, B)]), the bins in
    each pair's orientation and the pairs in order of first appearance; `n_min` and `x_max` are refused."""
    if trans:
        if n_min is not None or x_max is not None:
            raise PileupError("-n / -x do not apply to inter-chromosomal loops: there is no distance")
        return _classify_trans(table, res, chromosomes)
    n_min = 30 if n_min is None else int(n_min)
    x, y = table.bins(res)
    cis = [_key(a) == _key(b) for a, b in zip(table.chr1, table.chr2)]
    selected, seen = [], set()
    for c, ok in (((c, True) for c in chromosomes) if chromosomes else zip(table.chr1, cis)):
        if ok and _key(c) not in seen:                   # each chromosome once, in order of first appearance
            seen.add(_key(c))
            selected.append(c)
    keys = {_key(c) for c in selected}
    status = []
    for k in range(len(table)):
        sep = int(y[k] - x[k])
        if not cis[k]:
            status.append("trans")
        elif _key(table.chr1[k]) not in keys:
            status.append("no_chrom")
        elif sep < n_min:
            status.append("short")
        elif x_max is not None and sep > x_max:
            status.append("long")
        else:
            status.append(None)
    return status, x, y, selected


# ----------------------------------------------------------------------------------------------------------------------
# the whole run
# ----------------------------------------------------------------------------------------------------------------------
def _read_band(f, chromosome, res, D, norm=False, bias=False, balance=None, device=None, verbose=False):
    """The chromosome's RAW band with distance limit D (device [D + 2, n]) and n, or (None, 0) when the map has no record of
    it (or no such chromosome)."""
    import torch
    from .hicfile import PackedContacts
    from .mustache import read_contacts
    from .normalize import band_from_host_coo, band_from_packed
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    try:
        r = read_contacts(f, norm, False, res, D * res, bias, chromosome, chromosome, verbose=verbose, packed=True, device=dev,
                          balance=balance)
    except NameError:                                  # a `.hic` file without this chromosome
        return None, 0
    if r is None:
        return None, 0
    if isinstance(r, PackedContacts):
        band = band_from_packed(r, D, dev)
        return band, int(band.shape[1])
    x, y, v, _res = r
    x = np.ascontiguousarray(x, dtype=np.int64)
    y = np.ascontiguousarray(y, dtype=np.int64)
    n = int(max(x.max(), y.max())) + 1
    return band_from_host_coo(x, y, np.ascontiguousarray(v, dtype=np.float64), n, D, dev), n


class PileupResult:
    """What pileup() returns: the table, per row `status`, `obs_center`, `oe_center`, `p2ll`; `chromosomes` = [(name, rows in,
    loops used, pile-up dict)] in run order; `all` = the genome-wide pile-up dict (sums, counts, means, metrics).  Under `peak`
    also per row `e_center`, `enrich_exp`, `enrich_fe` ([rows, 4]: DONUT, LL, H, V) and `fe_min`, NaN for a row that was not
    used, and "enrich_agg" in every pile-up dict; without it they are None."""

    def __init__(self, table, status, w, q, peak=None):
        self.table, self.status, self.w, self.q, self.peak = table, status, w, q, peak
        L = len(table)
        self.obs_center, self.oe_center, self.p2ll = np.full(L, np.nan), np.full(L, np.nan), np.full(L, np.nan)
        self.e_center = self.enrich_exp = self.enrich_fe = self.fe_min = None
        if peak is not None:
            self.e_center, self.fe_min = np.full(L, np.nan), np.full(L, np.nan)
            self.enrich_exp, self.enrich_fe = np.full((L, 4), np.nan), np.full((L, 4), np.nan)
        self.chromosomes = []
        self.all = None

    def take(self, rows, part):
        """the per-loop values of pile-up dict `part` to the table rows `rows` (one per loop of `part`, in its order)"""
        rows = np.asarray(rows, np.int64)
        self.obs_center[rows], self.oe_center[rows], self.p2ll[rows] = part["center_obs"], part["center_oe"], part["p2ll"]
        if self.peak is not None:
            self.e_center[rows], self.fe_min[rows] = part["center_e"], part["fe_min"]
            self.enrich_exp[rows], self.enrich_fe[rows] = part["enrich_exp"], part["enrich_fe"]

    def total(self, tot):
        """`all` from the four genome-wide sums and counts"""
        apa, apa_oe = mean_map(tot[0], tot[1]), mean_map(tot[2], tot[3])
        self.all = {"sum_obs": tot[0], "count_obs": tot[1], "sum_oe": tot[2], "count_oe": tot[3], "apa": apa, "apa_oe": apa_oe,
                    "metrics": metrics(apa, self.w, self.q), "metrics_oe": metrics(apa_oe, self.w, self.q)}
        if self.peak is not None:
            self.all["enrich_agg"] = aggregate_enrichment(apa_oe, self.w, self.peak)


def _read_pair(f, norm, A, B, res, device):
    """read_trans_contacts, or None when the file has no such chromosome or no matrix for the pair."""
    from .hicfile import HicError
    from .trans import read_trans_contacts
    try:
        return read_trans_contacts(f, norm, A, B, res, device=device)
    except NameError:
        return None
    except HicError as e:
        if e.code == -4 and ("is not in the file" in str(e) and "chromosome" in str(e) or "no matrix for the pair" in str(e)):
            return None
        raise


def _pileup_trans(f, table, res, chromosomes, norm, bias, balance, w, q, n_min, x_max, device, verbose, peak=None):
    """pileup() in trans mode: one pile-up per chromosome pair."""
    import torch
    from .request import balance_on_trans, trans_input
    why = trans_input((f,)) or balance_on_trans(balance or None)
    if why is None and bias:
        why = "-b does not apply to inter-chromosomal pairs"
    if why:
        raise PileupError(why)
    status, a, b, pairs = classify(table, res, chromosomes, n_min, x_max, trans=True)
    out = PileupResult(table, status, w, q, peak)
    S = 2 * w + 1
    tot = [np.zeros((S, S)) for _ in range(4)]
    for A, B in pairs:
        pair = frozenset((_key(A), _key(B)))
        rows = [k for k in range(len(table)) if status[k] is None
                and frozenset((_key(table.chr1[k]), _key(table.chr2[k]))) == pair]
        part, used = _empty_result(w, q, peak), []
        got = _read_pair(f, norm, A, B, res, device)
        if got is None:
            for k in rows:
                status[k] = "no_pair"
        else:
            x, y, v, _res = got
            n1 = int(torch.as_tensor(x).max().item()) + 1
            n2 = int(torch.as_tensor(y).max().item()) + 1
            for k in rows:
                status[k] = "off_map" if a[k] >= n1 or b[k] >= n2 else "used"
            used = [k for k in rows if status[k] == "used"]
            part = pileup_trans_records(x, y, v, n1, n2, a[used], b[used], w, q, **_peak_kw(peak))
            del x, y, v, got
            out.take(used, part)
        part = {k_: v_ for k_, v_ in part.items() if k_ not in ("valid", "expected", "obs", "oe")}   # device arrays freed
        out.chromosomes.append(("%s,%s" % (A, B), len(rows), len(used), part))
        for t, name in zip(tot, ("sum_obs", "count_obs", "sum_oe", "count_oe")):
            t += part[name]                              # genome-wide: in the order the pairs ran
        if verbose:
            print("pile-up of the pair %s,%s: %d of %d rows used, P2M %r" % (A, B, len(used), len(rows), part["metrics"]["P2M"]))
    out.total(tot)
    return out


WINDOW_SHARE = 0.25               # genome mode: the windows of a batch's loops may take this share of the device's free memory


def window_bytes(loops, w):
    """device bytes of the obs and oe windows of `loops` loops"""
    return 16 * (2 * int(w) + 1) ** 2 * int(loops)


def window_budget():
    """the bytes the windows of one batch may take: WINDOW_SHARE of the device memory that is free now"""
    import torch
    return int(WINDOW_SHARE * int(torch.cuda.mem_get_info()[0]))


def _window_batches(loops_of, w, budget, names):
    """Consecutive pairs (indices into loops_of, the pairs' used-loop counts) whose windows fit `budget` bytes together.  A
    single pair that does not fit is a PileupError with both numbers, before anything is launched."""
    for p, n in enumerate(loops_of):
        if window_bytes(n, w) > budget:
            raise PileupError("the windows of the pair %s (%d loops, w = %d) need %d bytes of device memory; %d bytes (%d%% of "
                              "what is free) are allowed" % (names[p], n, w, window_bytes(n, w), budget, round(100 * WINDOW_SHARE)))
    batch, held = [], 0
    for p, n in enumerate(loops_of):
        if batch and held + window_bytes(n, w) > budget:
            yield batch
            batch, held = [], 0
        batch.append(p)
        held += window_bytes(n, w)
    if batch:
        yield batch


def _pileup_trans_genome(f, table, res, chromosomes, norm, bias, balance, method, pixels, pairs_zero_based, w, q, n_min, x_max,
                         device, verbose, peak=None):
    """pileup() in trans mode on the genome-balanced map (the module docstring has the rules): the genome read and balanced
    once, every pair's records balanced and piled up in shared launches, one host wait per batch."""
    from . import pairs as pairs_mod
    from .balance import BalanceError, report
    from .balance_genome import APPLY_BATCH_RECORDS, balanced_segments, check_genome_request, read_genome, solve_genome
    from .request import keep_trans_rows
    from_pairs = pairs_mod.is_pairs(f)
    try:
        method, pixels = check_genome_request(method, pixels, [f], bias or None, norm, balance or None, 1, "all",
                                              pairs_trans=from_pairs)
    except BalanceError as e:
        raise PileupError(str(e))
    why = keep_trans_rows([f], pairs_zero_based) if from_pairs else None      # the one parse of a pairs file, host only
    if why:
        raise PileupError(why)
    status, a, b, pairs = classify(table, res, chromosomes, n_min, x_max, trans=True)
    out = PileupResult(table, status, w, q, peak)
    import torch
    try:
        gb = solve_genome(read_genome(f, res, pixels, device, pairs_zero_based, verbose), method)
    except BalanceError as e:
        raise PileupError(str(e))
    if verbose:
        report(gb.info, gb.label)
    at = {frozenset((_key(A), _key(B))): p for p, (A, B) in enumerate(pairs)}
    rows_of, used_of, live = [[] for _ in pairs], [[] for _ in pairs], []
    for k in range(len(table)):                         # one pass: every eligible row to its pair
        if status[k] is None:
            rows_of[at[frozenset((_key(table.chr1[k]), _key(table.chr2[k])))]].append(k)
    for p, (A, B) in enumerate(pairs):
        rows = rows_of[p]
        try:
            have = gb.records(A, B) is not None
        except NameError:                               # a chromosome of the pair is not in the file
            have = False
        if not have:
            for k in rows:
                status[k] = "no_pair"
            continue
        n1, n2 = gb.bins[gb.index(A)], gb.bins[gb.index(B)]
        for k in rows:
            status[k] = "off_map" if a[k] >= n1 or b[k] >= n2 else "used"
        used_of[p] = [k for k in rows if status[k] == "used"]
        live.append(p)
    parts = [_empty_result(w, q, peak) for _ in pairs]
    drop = ("valid", "expected", "obs", "oe", "kept")
    with torch.cuda.device(gb.device):
        budget = window_budget()
        names = ["%s,%s" % pairs[p] for p in live]
        for group in list(_window_batches([len(used_of[p]) for p in live], w, budget, names)):
            mine = [live[i] for i in group]
            for k0, k1, x, y, v, seg in balanced_segments(gb, [pairs[p] for p in mine], release=True,
                                                          max_records=APPLY_BATCH_RECORDS):
                batch = mine[k0:k1]
                dims = [(gb.bins[gb.index(pairs[p][0])], gb.bins[gb.index(pairs[p][1])]) for p in batch]
                got = pileup_trans_batch(x, y, v, seg, dims, [(a[used_of[p]], b[used_of[p]]) for p in batch], w, q,
                                         **_peak_kw(peak))
                del x, y, v
                for p, part in zip(batch, got):
                    if part["kept"] == 0:               # nothing of the pair survives the balancing: its result is discarded
                        for k in rows_of[p]:
                            status[k] = "no_pair"
                        used_of[p] = []
                        continue
                    out.take(used_of[p], part)
                    parts[p] = {k_: v_ for k_, v_ in part.items() if k_ not in drop}
                del got
    S = 2 * w + 1
    tot = [np.zeros((S, S)) for _ in range(4)]
    for p, (A, B) in enumerate(pairs):
        part = {k_: v_ for k_, v_ in parts[p].items() if k_ not in drop}
        out.chromosomes.append(("%s,%s" % (A, B), len(rows_of[p]), len(used_of[p]), part))
        for t, name in zip(tot, ("sum_obs", "count_obs", "sum_oe", "count_oe")):
            t += part[name]                              # genome-wide: in the order of first appearance
        if verbose:
            print("pile-up of the pair %s,%s: %d of %d rows used, P2M %r" % (A, B, len(used_of[p]), len(rows_of[p]),
                                                                            part["metrics"]["P2M"]))
    out.total(tot)
    return out


def pileup(f, loops, res, chromosomes=None, norm=False, bias=False, balance=None, w=10, q=6, n_min=None, x_max=None,
           device=None, verbose=False, trans=False, balance_genome=None, balance_pixels="all", pairs_zero_based=False, peak=None):
    """Pile up map `f` around the loops of `loops` (a TSV path or a LoopTable) at resolution `res` (bp).  The reader
    arguments (`norm`, `bias`, `balance`) mean what they mean for the caller; `n_min` is in bins (None: 30), `x_max` in bp.
    trans=True piles up the inter-chromosomal rows instead, pair by pair (the module docstring has the rules); in that mode
    `chromosomes` of the result holds ("A,B", rows in, loops used, pile-up dict).  balance_genome="NEWTON" | "ICE" (with
    trans=True; balance_pixels "all" | "inter"; pairs_zero_based for a pairs file) piles the rows up on the genome-balanced map
    of a raw `.hic` file or a `.pairs` / `.pairs.gz` file, every pair in shared launches.  peak=p (0 <= p < w) scores every
    used loop against its local background in any of the three modes ("Enrichment" in the module docstring).  Returns a
    PileupResult."""
    w, q, res = int(w), int(q), int(res)
    check_window(w, q)
    if peak is not None:
        peak = int(peak)
        check_peak(w, peak)
    table = read_loops(loops) if isinstance(loops, (str, os.PathLike)) else loops
    if balance_genome is not None:
        if not trans:
            raise PileupError("--balance-genome is for inter-chromosomal pile-ups: give --trans (--balance balances one "
                              "chromosome's own map)")
        return _pileup_trans_genome(f, table, res, chromosomes, norm, bias, balance, balance_genome, balance_pixels,
                                    pairs_zero_based, w, q, n_min, x_max, device, verbose, peak)
    if trans:
        return _pileup_trans(f, table, res, chromosomes, norm, bias, balance, w, q, n_min, x_max, device, verbose, peak)
    status, x, y, selected = classify(table, res, chromosomes, n_min, None if x_max is None else int(x_max) // res)
    out = PileupResult(table, status, w, q, peak)
    S = 2 * w + 1
    tot = [np.zeros((S, S)) for _ in range(4)]
    for chrom in selected:
        rows = [k for k in range(len(table)) if _key(table.chr1[k]) == _key(chrom) and status[k] != "trans"]
        cand = [k for k in rows if status[k] is None]
        part = _empty_result(w, q, peak)
        used = []
        if cand:
            D = int(max(y[k] - x[k] for k in cand)) + 2 * w
            band, n = _read_band(f, chrom, res, D, norm, bias, balance, device, verbose)
            if band is None:
                for k in cand:
                    status[k] = "no_chrom"
            else:
                for k in cand:
                    status[k] = "off_map" if y[k] >= n else "used"
                used = [k for k in cand if status[k] == "used"]
                part = pileup_band(band, n, D, x[used], y[used], w, q, **_peak_kw(peak))
                del band
            out.take(used, part)
        part = {k_: v for k_, v in part.items() if k_ not in ("valid", "expected", "obs", "oe")}   # device arrays freed
        out.chromosomes.append((chrom, len(rows), len(used), part))
        for t, name in zip(tot, ("sum_obs", "count_obs", "sum_oe", "count_oe")):
            t += part[name]                              # genome-wide: in the order the chromosomes ran
        if verbose:
            print("pile-up of chromosome %s: %d of %d rows used, P2LL %r" % (chrom, len(used), len(rows),
                                                                           part["metrics"]["P2LL"]))
    out.total(tot)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# output files
# ----------------------------------------------------------------------------------------------------------------------
def _r(v):
    return repr(float(v))


def write_matrix(path, M):
    with open(path, "w") as fh:
        fh.write("".join("\t".join(_r(v) for v in row) + "\n" for row in np.asarray(M)))


def write_outputs(prefix, res):
    """PREFIX.apa.tsv, PREFIX.oe.tsv, PREFIX.stats.tsv, PREFIX.loops.tsv of a PileupResult."""
    write_matrix(prefix + ".apa.tsv", res.all["apa"])
    write_matrix(prefix + ".oe.tsv", res.all["apa_oe"])

    def stats_row(name, rows_in, used, p):
        return "%s\t%d\t%d\t%s\t%s\n" % (name, rows_in, used, "\t".join(_r(p["metrics"][m]) for m in METRICS),
                                        _r(p["metrics_oe"]["P2LL"]))
    with open(prefix + ".stats.tsv", "w") as fh:
        fh.write(STATS_HEADER)
        for name, rows_in, used, p in res.chromosomes:
            fh.write(stats_row(name, rows_in, used, p))
        fh.write(stats_row("all", len(res.table), sum(u for _, _, u, _ in res.chromosomes), res.all))
    with open(prefix + ".loops.tsv", "w") as fh:
        fh.write(res.table.header + "\t" + "\t".join(LOOP_COLUMNS) + "\n")
        fh.write("".join("%s\t%s\t%s\t%s\t%s\n" % (line, s, _r(a), _r(b), _r(c)) for line, s, a, b, c in
                         zip(res.table.lines, res.status, res.obs_center, res.oe_center, res.p2ll)))


def write_enrichment(prefix, res, min_enrichment=None):
    """PREFIX.enrich.tsv and PREFIX.enrich.stats.tsv of a PileupResult made with `peak`; with min_enrichment = T also
    PREFIX.enriched.tsv, the `used` rows with FE_MIN >= T as a loop list (NaN fails).  Returns how many rows that list holds
    (None without T)."""
    if res.peak is None:
        raise PileupError("this pile-up ran without a peak half-width: there is no enrichment to write")
    with open(prefix + ".enrich.tsv", "w") as fh:
        fh.write(res.table.header + "\t" + "\t".join(ENRICH_COLUMNS) + "\n")
        for k, line in enumerate(res.table.lines):
            vals = [res.obs_center[k], res.e_center[k]] + list(res.enrich_exp[k]) + list(res.enrich_fe[k]) + [res.fe_min[k]]
            fh.write("%s\t%s\t%s\n" % (line, res.status[k], "\t".join(_r(v) for v in vals)))
    with open(prefix + ".enrich.stats.tsv", "w") as fh:
        fh.write(ENRICH_STATS_HEADER)
        for name, _rows_in, used, part in res.chromosomes:
            fh.write("%s\t%d\t%s\n" % (name, used, "\t".join(_r(v) for v in part["enrich_agg"])))
        fh.write("all\t%d\t%s\n" % (sum(u for _, _, u, _ in res.chromosomes), "\t".join(_r(v) for v in res.all["enrich_agg"])))
    if min_enrichment is None:
        return None
    with np.errstate(invalid="ignore"):
        keep = [k for k in range(len(res.table)) if res.status[k] == "used" and res.fe_min[k] >= min_enrichment]
    with open(prefix + ".enriched.tsv", "w") as fh:
        fh.write(res.table.header + "\n")
        fh.write("".join(res.table.lines[k] + "\n" for k in keep))
    return len(keep)


# ----------------------------------------------------------------------------------------------------------------------
# command line
# ----------------------------------------------------------------------------------------------------------------------
def parse_args(args):
    p = argparse.ArgumentParser(description="Aggregate peak analysis (APA) of a Mustache loop list on the GPU")
    p.add_argument("-f", "--file", dest="f_path", required=True, help="contact map (text + -b, .hic, .cool, .mcool)")
    p.add_argument("-l", "--loops", dest="loops", required=True, help="loop list: a TSV written by Mustache")
    p.add_argument("-r", "--resolution", dest="resolution", required=True, help="resolution of the map")
    p.add_argument("-o", "--outfile", dest="prefix", required=True, help="output prefix")
    p.add_argument("-ch", "--chromosome", dest="chromosome", nargs="+", default=None,
                   help="chromosomes to use (default: those of the cis rows, in order of first appearance)")
    p.add_argument("-b", "--biases", dest="biasfile", default=None, help="bias vector of a text map")
    p.add_argument("-norm", "--normalization", dest="norm_method", default=False, help=".hic normalisation (KR, VC, NONE)")
    p.add_argument("--balance", dest="balance", default=None, metavar="ICE|NEWTON",
                   help="balance the raw map on the GPU (ICE or NEWTON)")
    p.add_argument("-w", "--window", dest="w", type=int, default=10, help="window half-width in bins (default 10, at most 64)")
    p.add_argument("-q", "--corner", dest="q", type=int, default=6, help="corner size in bins (default 6)")
    p.add_argument("-n", "--min-distance", dest="n_min", type=int, default=None,
                   help="smallest loop size y - x in bins (default 30)")
    p.add_argument("-x", "--max-distance", dest="x_max", default=None, help="largest loop size in bp (default: none)")
    p.add_argument("--trans", dest="trans", action="store_true",
                   help="pile up the inter-chromosomal rows, pair by pair (.hic / .cool; -ch keeps the pairs inside the list)")
    from .balance_genome import add_arguments
    add_arguments(p)                 # --balance-genome, --balance-pixels, --pairs-trans: with --trans, the genome-balanced map
    p.add_argument("--pairs-zero-based", dest="pairs_zero_based", action="store_true",
                   help="OPTIONAL: .pairs / .pairs.gz input only: positions are 0-based (bin = pos // res)")
    p.add_argument("--enrich", dest="enrich", action="store_true",
                   help="score every used loop against its donut, lower-left, horizontal and vertical neighbourhoods: "
                        "PREFIX.enrich.tsv and PREFIX.enrich.stats.tsv")
    p.add_argument("--peak", dest="peak", type=int, default=None, metavar="P",
                   help="with --enrich: half-width of the peak box the neighbourhoods leave out (default %d, below -w)" % DEFAULT_PEAK)
    p.add_argument("--min-enrichment", dest="min_enrichment", type=float, default=None, metavar="T",
                   help="with --enrich: also write PREFIX.enriched.tsv, the used rows with FE_MIN >= T as a loop list")
    return p.parse_args(args)


def enrich_request(args):
    """What --enrich / --peak / --min-enrichment ask: the peak half-width, None for a run without them; PileupError with the
    text of the `Error:` line for a combination that cannot be honoured.  Reads nothing and touches no GPU."""
    if not args.enrich:
        for flag, given in (("--peak", args.peak), ("--min-enrichment", args.min_enrichment)):
            if given is not None:
                raise PileupError("%s without --enrich: it belongs to the enrichment of every loop; give --enrich" % flag)
        return None
    peak = DEFAULT_PEAK if args.peak is None else args.peak
    if not 0 <= peak < args.w:
        raise PileupError("--peak %d with -w %d: the peak half-width P must be in 0 .. w - 1 (P >= w leaves no neighbourhood)"
                          % (peak, args.w))
    return peak


def genome_request(args, f, world):
    """What --balance-genome / --balance-pixels / --pairs-trans / --pairs-zero-based ask of a pile-up: (method, pixels) of a
    genome-mode run, None for a run without them; PileupError with the text of the `Error:` line for a combination that cannot
    be honoured.  Reads nothing and touches no GPU."""
    from .balance import BalanceError
    from .balance_genome import check_genome_request
    from .pairs import is_pairs
    pairs_file = is_pairs(f)
    if args.pairs_trans and not pairs_file:
        raise PileupError("--pairs-trans is for .pairs / .pairs.gz input (%s is none)" % f)
    if args.pairs_zero_based and not pairs_file:
        raise PileupError("--pairs-zero-based is for .pairs / .pairs.gz input (%s is none)" % f)
    if args.pairs_zero_based and not args.pairs_trans:
        raise PileupError("--pairs-zero-based without --pairs-trans: only the genome-balanced pile-up (--trans --pairs-trans "
                          "--balance-genome ICE|NEWTON) bins a pairs file with it")
    asked = args.balance_genome is not None or args.balance_pixels_given
    if pairs_file and (args.trans or asked) and not args.pairs_trans:
        raise PileupError("%s without --pairs-trans: only intra-chromosomal loops are piled up from a pairs file without it; give "
                          "--trans --pairs-trans --balance-genome ICE|NEWTON" % f)
    if args.pairs_trans and args.balance_genome is None:
        raise PileupError("--pairs-trans without --balance-genome: %s holds raw read pairs; give --balance-genome ICE|NEWTON" % f)
    if not asked:
        return None
    if args.balance_genome is not None and not args.trans:
        raise PileupError("--balance-genome without --trans: it balances the whole genome's map for inter-chromosomal "
                          "pile-ups; use --balance for one chromosome's own map")
    try:
        return check_genome_request(args.balance_genome, args.balance_pixels, [f], args.biasfile, args.norm_method, args.balance,
                                    world, "all" if args.trans else "none", pairs_trans=args.pairs_trans)
    except BalanceError as e:
        raise PileupError(str(e))


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    from .mustache import parseBP
    from .sharding import init_from_env
    _rank, world = init_from_env()
    if world > 1:
        print("Error: pile-ups run on one GPU only (this run has %d ranks); start a single process" % world)
        return
    f = args.f_path
    if not f or not os.path.exists(f):
        print("Error: Couldn't find the specified contact files")
        return
    if not os.path.exists(args.loops):
        print("Error: Couldn't find the loop list %s" % args.loops)
        return
    res = parseBP(args.resolution)
    if not res:
        print("Error: Invalid resolution")
        return
    if args.biasfile and not os.path.exists(args.biasfile):
        print("Error: Couldn't find specified bias file")
        return
    try:
        genome = genome_request(args, f, world)
        peak = enrich_request(args)
    except PileupError as e:
        print("Error: %s" % e)
        return
    balance = None
    if args.balance is not None:
        from .balance import BalanceError, check_request
        try:
            balance = check_request(args.balance, f, args.biasfile, args.norm_method, world)
        except BalanceError as e:
            print("Error: %s" % e)
            return
    x_max = None
    if args.x_max is not None:
        x_max = parseBP(str(args.x_max))
        if not x_max:
            print("Error: Invalid -x distance %s" % args.x_max)
            return
    from .hicfile import HicError
    from .trans import TransError
    try:
        check_window(args.w, args.q)
        res_ = pileup(f, args.loops, res, chromosomes=args.chromosome, norm=args.norm_method, bias=args.biasfile or False,
                      balance=balance, w=args.w, q=args.q, n_min=args.n_min, x_max=x_max, verbose=True, trans=args.trans,
                      balance_genome=genome[0] if genome else None, balance_pixels=genome[1] if genome else "all",
                      pairs_zero_based=args.pairs_zero_based, peak=peak)
    except (PileupError, TransError) as e:
        print("Error: %s" % e)
        return
    except HicError as e:
        if not args.trans:
            raise
        print("Error: %s" % e)                           # a `.hic` file of version 6: the trans reader's own refusal
        return
    write_outputs(args.prefix, res_)
    a = res_.all["metrics"]
    print("%d of %d loops piled up: P2LL %r, ZscoreLL %r, P2M %r -> %s.{apa,oe,stats,loops}.tsv"
          % (sum(u for _, _, u, _ in res_.chromosomes), len(res_.table), a["P2LL"], a["ZscoreLL"], a["P2M"], args.prefix))
    if peak is not None:
        kept = write_enrichment(args.prefix, res_, args.min_enrichment)
        print("enrichment with peak half-width %d: aggregate over DONUT, LL, H, V %s -> %s.enrich.tsv, %s.enrich.stats.tsv%s"
              % (peak, ", ".join(_r(v) for v in res_.all["enrich_agg"]), args.prefix, args.prefix,
                 "" if kept is None else "; %d loops with FE_MIN >= %r -> %s.enriched.tsv" % (kept, args.min_enrichment, args.prefix)))


if __name__ == "__main__":
    main()
