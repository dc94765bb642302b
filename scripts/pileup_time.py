"""Pile-up (APA) timing on a synthetic chr1 @ 1 kb raw band built on the device (248 957 bins, D = 2 020) with 20 000
loops, w = 10 (GPU box): device events around the three stages (valid + expected, windows, reduce) and the whole
pileup_band call, median of --steps after --warmup; bytes moved from shapes and the expected pass's share of 6.3 TB/s.
Prints one JSON line.  python scripts/pileup_time.py [--steps 20] [--warmup 3]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loops", type=int, default=20000)
    a = ap.parse_args()
    n, D, w, q, L = 248957, 2020, 10, 6, a.loops
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
    t_all = timed(lambda: pl.pileup_band(band, n, D, xs, ys, w, q), a.steps, a.warmup)
    r = pl.pileup_band(band, n, D, xs, ys, w, q)
    band_bytes = (D + 1) * n * 8
    exp_bytes = 2 * band_bytes                                    # the valid pass and the expected pass each read the band once
    win_bytes = L * S * S * 8 * 3                                 # band reads + obs and oe writes
    red_bytes = L * S * S * 8 * 2                                 # obs and oe read once
    ms = lambda t: round(t[0], 4)                                 # noqa: E731
    print(json.dumps({
        "metric": "pileup_chr1_1kb_ms", "n": n, "D": D, "loops": L, "w": w, "steps": a.steps, "warmup": a.warmup,
        "expected_ms": ms(t_exp), "windows_ms": ms(t_win), "reduce_ms": ms(t_red), "pileup_band_ms": ms(t_all),
        "expected_min_max_ms": [round(t_exp[1], 4), round(t_exp[2], 4)],
        "pileup_band_min_max_ms": [round(t_all[1], 4), round(t_all[2], 4)],
        "expected_bytes": exp_bytes, "windows_bytes": win_bytes, "reduce_bytes": red_bytes,
        "expected_model_ms": round(exp_bytes / (HBM_TBS * 1e12) * 1e3, 4),
        "expected_share_of_6p3_TBs": round(exp_bytes / (t_exp[0] * 1e-3) / (HBM_TBS * 1e12), 4),
        "windows_TBs": round(win_bytes / (t_win[0] * 1e-3) / 1e12, 3), "reduce_TBs": round(red_bytes / (t_red[0] * 1e-3) / 1e12, 3),
        "P2LL": r["metrics"]["P2LL"], "valid_bins": int(valid.sum().item()),
    }))


if __name__ == "__main__":
    main()
