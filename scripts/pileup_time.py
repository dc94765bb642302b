"""Pile-up (APA) timing on a synthetic chr1 @ 1 kb raw band built on the device (248 957 bins, D = 2 020) with 20 000
loops, w = 10 (GPU box): device events around the three stages (valid + expected, windows, reduce), the enrichment of every loop
(mst_pileup_enrich, peak half-width --peak) and the whole pileup_band call without and with `peak`, median of --steps after
--warmup; bytes moved from shapes, the expected pass's share of 6.3 TB/s and the enrichment against its byte model (8 L (2w+1)^2
bytes read).  The two-map leg (two_map_leg) piles the same list up on a second band: pileup_band_pair as a whole, and
mst_pileup_compare and mst_pileup_reduce_pair alone against their byte model at the copy bandwidth measured in the same run.
The significance leg (poisson_leg) takes the band's non-zero pixels, rounded, as the chromosome's raw record set (float32 counts, a
bias of ones): mst_pileup_centre_counts alone against its byte model (12 bytes per record at 6.3 TB/s), mst_pileup_poisson alone,
and the whole pileup_band call with `peak` and with `peak` and `poisson`, the two alternating.
Prints one JSON line.  python scripts/pileup_time.py [--steps 20] [--warmup 3] [--peak 2]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mustache_amd import pileup as pl                      # noqa: E402
from mustache_amd.synth import band_counts                 # noqa: E402

HBM_TBS = 6.3


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), float(min(out)), float(max(out))


def two_map_leg(a, band, n, D, xs, ys, w, q, p, oe, order, ws, dev):
    """The same list on two maps: a second band from another seed, pileup_band_pair as a whole, and mst_pileup_compare and
    mst_pileup_reduce_pair alone on the two resident stacks of oe windows, each against its byte model (16 L (2w+1)^2 bytes read)
    at the bandwidth a device-to-device copy of 1 GiB reaches on this card in this run."""
    L, S = len(xs), 2 * w + 1
    band2 = torch.empty_like(band)
    for i0 in range(0, n, 16384):
        i1 = min(n, i0 + 16384)
        band2[:, i0:i1] = band_counts(n, D, 300.0, 8000, 2, i0=i0, i1=i1, device=dev)
    xd, yd = torch.from_numpy(xs).to(dev), torch.from_numpy(ys).to(dev)
    _valid2, E2 = pl.expected(band2, n, D, ws)
    _obs2, oe2, _st2 = pl.windows(band2, n, D, E2, xd, yd, w, q)
    del _obs2
    src = torch.empty(1 << 27, dtype=torch.float64, device=dev).normal_()
    dst = torch.empty_like(src)
    torch.cuda.synchronize()
    t_copy = timed(lambda: dst.copy_(src), a.steps, a.warmup)
    copy_tbs = 2 * src.numel() * 8 / (t_copy[0] * 1e-3) / 1e12       # read + write
    del src, dst
    t_cmp = timed(lambda: pl.compare_windows(oe, oe2, w, p), a.steps, a.warmup)
    t_red = timed(lambda: pl.reduce_pair(oe, oe2, order, w, ws), a.steps, a.warmup)
    t_old = timed(lambda: pl.reduce(oe, oe2, order, w, ws), a.steps, a.warmup)     # the four-sum reduce on the same bytes
    t_pair = timed(lambda: pl.pileup_band_pair(band, n, band2, n, D, xs, ys, w, q, p), a.steps, a.warmup)
    _r1, _r2, c = pl.pileup_band_pair(band, n, band2, n, D, xs, ys, w, q, p)
    kernel_bytes = 16 * L * S * S
    model = kernel_bytes / (copy_tbs * 1e12) * 1e3
    rnd = lambda t: [round(t[0], 4), round(t[1], 4), round(t[2], 4)]     # noqa: E731
    return {"copy_1GiB_TBs": round(copy_tbs, 3), "copy_ms_med_min_max": rnd(t_copy), "two_map_kernel_bytes": kernel_bytes,
            "two_map_model_ms": round(model, 4),
            "compare_ms_med_min_max": rnd(t_cmp), "compare_over_model": round(t_cmp[0] / model, 2),
            "reduce_pair_ms_med_min_max": rnd(t_red), "reduce_pair_over_model": round(t_red[0] / model, 2),
            "reduce_on_the_same_windows_ms_med_min_max": rnd(t_old),
            "pileup_band_pair_ms_med_min_max": rnd(t_pair), "two_map_lfc_p2ll": c["lfc_p2ll"],
            "two_map_loops_scored": int((~np.isnan(c["lfc"])).sum())}


def poisson_leg(a, band, n, D, xs, ys, w, q, p, obs, E, dev):
    """The raw record set: every band pixel whose rounded value is >= 1, as (x, dist, float32 count), slab by slab; the bias is 1
    everywhere, so the balanced band is the raw map and raw_center must equal rint(center_obs)."""
    xr, dr, cr = [], [], []
    for i0 in range(0, n, 16384):
        i1 = min(n, i0 + 16384)
        c = torch.round(band[:D + 1, i0:i1])
        d, x = torch.nonzero(c >= 1.0, as_tuple=True)
        xr.append((x + i0).to(torch.int32))
        dr.append(d.to(torch.int32))
        cr.append(c[d, x].to(torch.float32))
    raw = pl.PoissonInput(torch.cat(xr), torch.cat(dr), torch.cat(cr), torch.ones(n, dtype=torch.float64, device=dev))
    del xr, dr, cr
    R, L = int(raw.count.numel()), len(xs)
    sep = ys - xs
    keys, inverse = np.unique((xs << 32) | sep, return_inverse=True)
    kd = torch.from_numpy(keys).to(dev)
    xd, yd = torch.from_numpy(xs).to(dev), torch.from_numpy(ys).to(dev)
    lo, hi = int(sep.min()), int(sep.max())
    in_range = int(((raw.dist >= lo) & (raw.dist <= hi)).sum().item())
    sums = pl.enrich_windows(obs, w, p, E=E, xs=xd, ys=yd)
    per_key, flag = pl.centre_counts(raw.x, raw.dist, raw.count, kd, lo, hi)
    counts = per_key[torch.from_numpy(inverse.reshape(-1).astype(np.int64)).to(dev)]
    centre, e_centre = obs[:, w, w].contiguous(), E[yd - xd]
    torch.cuda.synchronize()
    t_cnt = timed(lambda: pl.centre_counts(raw.x, raw.dist, raw.count, kd, lo, hi), a.steps, a.warmup)
    t_tail = timed(lambda: pl.poisson_windows(sums, centre, e_centre, counts, raw.bias, xd, yd), a.steps, a.warmup)
    t_peak, t_both = [], []
    for _ in range(a.warmup):
        pl.pileup_band(band, n, D, xs, ys, w, q, peak=p)
        pl.pileup_band(band, n, D, xs, ys, w, q, peak=p, poisson=raw)
    for _ in range(a.steps):                                      # alternating: both see the same machine
        t_peak.append(timed(lambda: pl.pileup_band(band, n, D, xs, ys, w, q, peak=p), 1, 0)[0])
        t_both.append(timed(lambda: pl.pileup_band(band, n, D, xs, ys, w, q, peak=p, poisson=raw), 1, 0)[0])
    r = pl.pileup_band(band, n, D, xs, ys, w, q, peak=p, poisson=raw)
    plain = pl.pileup_band(band, n, D, xs, ys, w, q, peak=p)
    same = all(np.array_equal(r[k], plain[k], equal_nan=True) for k in ("enrich_exp", "enrich_fe", "fe_min", "enrich_sums"))
    rec_bytes = 8 * R + 4 * in_range                              # x and dist of every record, the count of those inside the range
    model = 12 * R / (HBM_TBS * 1e12) * 1e3
    rnd = lambda t: [round(float(np.median(t)), 4), round(float(min(t)), 4), round(float(max(t)), 4)]     # noqa: E731
    return {"poisson_records": R, "poisson_records_in_range": in_range, "poisson_keys": int(len(keys)),
            "centre_counts_ms_med_min_max": [round(v, 4) for v in t_cnt], "centre_counts_model_ms": round(model, 4),
            "centre_counts_over_model": round(t_cnt[0] / model, 2), "centre_counts_bytes_read": rec_bytes,
            "centre_counts_TBs": round(rec_bytes / (t_cnt[0] * 1e-3) / 1e12, 3),
            "poisson_kernel_ms_med_min_max": [round(v, 4) for v in t_tail],
            "pileup_band_peak_alternating_ms_med_min_max": rnd(t_peak), "pileup_band_poisson_ms_med_min_max": rnd(t_both),
            "poisson_fractional_flag": int(flag.item()), "poisson_unconverged": int(r["poisson_unconverged"]),
            "poisson_raw_equals_rint_obs": bool((r["raw_center"] == np.rint(r["center_obs"])).all()),
            "poisson_ratios_equal_host": bool(same), "poisson_p_max_defined": int((~np.isnan(r["p_max"])).sum()),
            "poisson_p_max_below_0p05": int((r["p_max"] < 0.05).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loops", type=int, default=20000)
    ap.add_argument("--peak", type=int, default=2)
    a = ap.parse_args()
    n, D, w, q, L, p = 248957, 2020, 10, 6, a.loops, a.peak
    dev = torch.device("cuda", 0)
    band = torch.empty((D + 2, n), dtype=torch.float64, device=dev)
    for i0 in range(0, n, 16384):
        i1 = min(n, i0 + 16384)
        band[:, i0:i1] = band_counts(n, D, 400.0, 8000, 1, i0=i0, i1=i1, device=dev)
    rng = np.random.default_rng(0)
    sep = rng.integers(30, D - 2 * w + 1, L)
    sep[0] = D - 2 * w
    xs = rng.integers(0, n - sep).astype(np.int64)
    ys = (xs + sep).astype(np.int64)
    S = 2 * w + 1
    from mustache_amd.engine import require_gpu
    lib = require_gpu()
    ws = pl._workspace(lib, n, D, L, w, dev)
    xd, yd = torch.from_numpy(xs).to(dev), torch.from_numpy(ys).to(dev)
    order = torch.from_numpy(np.lexsort((ys, xs)).astype(np.int32)).to(dev)
    valid, E = pl.expected(band, n, D, ws)
    obs, oe, _st = pl.windows(band, n, D, E, xd, yd, w, q)
    torch.cuda.synchronize()
    t_exp = timed(lambda: pl.expected(band, n, D, ws), a.steps, a.warmup)
    t_win = timed(lambda: pl.windows(band, n, D, E, xd, yd, w, q), a.steps, a.warmup)
    t_red = timed(lambda: pl.reduce(obs, oe, order, w, ws), a.steps, a.warmup)
    t_enr = timed(lambda: pl.enrich_windows(obs, w, p, E=E, xs=xd, ys=yd), a.steps, a.warmup)
    t_all = timed(lambda: pl.pileup_band(band, n, D, xs, ys, w, q), a.steps, a.warmup)
    t_peak = timed(lambda: pl.pileup_band(band, n, D, xs, ys, w, q, peak=p), a.steps, a.warmup)
    t_all2 = timed(lambda: pl.pileup_band(band, n, D, xs, ys, w, q), a.steps, a.warmup)       # again: the run-to-run spread
    r = pl.pileup_band(band, n, D, xs, ys, w, q, peak=p)
    two = two_map_leg(a, band, n, D, xs, ys, w, q, p, oe, order, ws, dev)
    two.update(poisson_leg(a, band, n, D, xs, ys, w, q, p, obs, E, dev))
    band_bytes = (D + 1) * n * 8
    exp_bytes = 2 * band_bytes                                    # the valid pass and the expected pass each read the band once
    win_bytes = L * S * S * 8 * 3                                 # band reads + obs and oe writes
    red_bytes = L * S * S * 8 * 2                                 # obs and oe read once
    enr_bytes = L * S * S * 8                                     # obs read once (the 96 L bytes written are 0.03 of it)
    ms = lambda t: round(t[0], 4)                                 # noqa: E731
    print(json.dumps({
        **two,
        "metric": "pileup_chr1_1kb_ms", "n": n, "D": D, "loops": L, "w": w, "steps": a.steps, "warmup": a.warmup,
        "expected_ms": ms(t_exp), "windows_ms": ms(t_win), "reduce_ms": ms(t_red), "pileup_band_ms": ms(t_all),
        "expected_min_max_ms": [round(t_exp[1], 4), round(t_exp[2], 4)],
        "pileup_band_min_max_ms": [round(t_all[1], 4), round(t_all[2], 4)],
        "expected_bytes": exp_bytes, "windows_bytes": win_bytes, "reduce_bytes": red_bytes,
        "expected_model_ms": round(exp_bytes / (HBM_TBS * 1e12) * 1e3, 4),
        "expected_share_of_6p3_TBs": round(exp_bytes / (t_exp[0] * 1e-3) / (HBM_TBS * 1e12), 4),
        "windows_TBs": round(win_bytes / (t_win[0] * 1e-3) / 1e12, 3), "reduce_TBs": round(red_bytes / (t_red[0] * 1e-3) / 1e12, 3),
        "peak": p, "enrich_ms": ms(t_enr), "enrich_min_max_ms": [round(t_enr[1], 4), round(t_enr[2], 4)], "enrich_bytes": enr_bytes,
        "enrich_model_ms": round(enr_bytes / (HBM_TBS * 1e12) * 1e3, 4), "enrich_TBs": round(enr_bytes / (t_enr[0] * 1e-3) / 1e12, 3),
        "pileup_band_peak_ms": ms(t_peak), "pileup_band_peak_min_max_ms": [round(t_peak[1], 4), round(t_peak[2], 4)],
        "pileup_band_again_ms": ms(t_all2), "pileup_band_again_min_max_ms": [round(t_all2[1], 4), round(t_all2[2], 4)],
        "P2LL": r["metrics"]["P2LL"], "valid_bins": int(valid.sum().item()),
        "loops_scored": int((~np.isnan(r["fe_min"])).sum()), "enrich_agg": [float(v) for v in r["enrich_agg"]],
    }))


if __name__ == "__main__":
    main()
