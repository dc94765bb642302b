#!/usr/bin/env python3
"""Differential trans loops of a synthetic genome, two ways on the same device-resident records of two samples:

  genome  call_diff_trans_genome: one batch -- a segmented z-score and a tile count per sample, the kept tile pairs in shared
          launches
  pairs   a loop of call_diff_trans_coo over the same pairs: 12 batches of one pair, each with its own two segmented z-scores,
          statistics copies, tile counts and launches (the same kernels and the same skip rule; what is compared is the
          batching)

The genome: 6 chromosomes of 6000, 5200, 4400, 3600, 3000 and 2400 bins, the first 12 of their pairs in pair order, drawn on the
device: sample 1 holds a log-normal background on a share of the pixels that falls geometrically from 0.2 (6000 x 5200:
6 * 10^6 records) to 0.002 along the pairs, plus 12 Gaussian blobs per pair; sample 2 is an independent draw at 0.7 of that share
with a third of the blobs left out and four new ones.  The sparse pairs at the end are what a real trans map at a fine
resolution looks like: their windows hold fewer than 10 000 records in one sample or in both.

Both forms run in this process after `--warmup` passes of each, alternating, host wall time around a device synchronise; the
median, minimum and maximum of `--reps` passes, the baseline's spread (max - min), the launch and tile-pair counts, the skipped
share and whether both forms gave the same rows go to one JSON line on stdout and into `--out`.  Needs the GPU.
python scripts/diff_trans_genome_time.py [--reps 7] [--warmup 2] [--out profiles/diff_trans_genome_time.json]"""
import argparse
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BINS = [6000, 5200, 4400, 3600, 3000, 2400]
PAIRS = 12
OCT, ST, PT, PT2 = [1.6, 3.2], 0.88, 0.2, 0.1


def draw(torch, dev, g, n1, n2, density, blobs):
    """(x int32, y int32, v float64) on the device: distinct pixels, the corner record included"""
    mask = torch.rand((n1, n2), generator=g, device=dev) < density
    mask[n1 - 1, n2 - 1] = True
    for cx, cy, s in blobs:                                       # a blob's pixels all hold a record, as in synth_trans
        r = int(2.8 * s) + 1
        mask[max(0, cx - r):cx + r + 1, max(0, cy - r):cy + r + 1] = True
    idx = mask.nonzero()
    del mask
    x, y = idx[:, 0].to(torch.int32).contiguous(), idx[:, 1].to(torch.int32).contiguous()
    v = torch.exp(0.5 * torch.randn(x.numel(), generator=g, device=dev, dtype=torch.float64))
    for cx, cy, s in blobs:
        d2 = ((x - cx).to(torch.float64)) ** 2 + ((y - cy).to(torch.float64)) ** 2
        v += torch.where(d2 < (2.8 * s) ** 2, 25.0 * torch.exp(-d2 / (2 * s * s)), torch.zeros_like(d2))
    return x, y, v


def _rows(rows):
    return [[int(r[0]), int(r[1]), float(r[2]), float(r[3]), int(r[4])] for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diff_trans_genome_time.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from mustache_amd.diff_trans import call_diff_trans_coo
    from mustache_amd.diff_trans_genome import call_diff_trans_genome
    if not torch.cuda.is_available():
        raise SystemExit("diff_trans_genome_time.py needs the GPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev).manual_seed(1)
    rng = np.random.default_rng(0)
    combos = list(itertools.combinations(range(len(BINS)), 2))[:PAIRS]
    densities = np.geomspace(0.2, 0.002, len(combos))
    pairs = []
    for k, (a, b) in enumerate(combos):
        n1, n2 = BINS[a], BINS[b]
        spots = [(int(rng.integers(8, n1 - 8)), int(rng.integers(8, n2 - 8)), float(rng.uniform(1.2, 3.0))) for _ in range(16)]
        pairs.append((draw(torch, dev, g, n1, n2, float(densities[k]), spots[:12]),
                      draw(torch, dev, g, n1, n2, 0.7 * float(densities[k]), spots[4:])))
    records = [sum(int(p[s][2].numel()) for p in pairs) for s in (0, 1)]

    stats = {}

    def genome():
        return call_diff_trans_genome(pairs, OCT, ST, PT, PT2, stats=stats)

    def one_by_one():
        return [call_diff_trans_coo(r1, r2, OCT, ST, PT, PT2) for r1, r2 in pairs]

    forms = (("genome", genome), ("pairs", one_by_one))
    times = {name: [] for name, _ in forms}
    rows = {}
    for i in range(args.warmup + args.reps):
        for name, fn in forms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = fn()
            torch.cuda.synchronize()
            if i >= args.warmup:
                times[name].append(time.perf_counter() - t0)
            rows[name] = [_rows(r) for r in got]
    med = {k: float(np.median(v)) for k, v in times.items()}
    by_tag = [sum(1 for r in rows["genome"] for row in r if row[4] == t) for t in (1, 2, 3, 4)]
    result = {
        "metric": "diff_trans_genome_s", "pairs": len(pairs), "records_sample1": records[0], "records_sample2": records[1],
        "largest_pair_records": max(int(p[0][2].numel()) for p in pairs), "reps": args.reps, "warmup": args.warmup,
        "genome_s": med["genome"], "genome_s_min_max": [min(times["genome"]), max(times["genome"])],
        "pairs_s": med["pairs"], "pairs_s_min_max": [min(times["pairs"]), max(times["pairs"])],
        "pairs_s_spread": max(times["pairs"]) - min(times["pairs"]), "pairs_over_genome": med["pairs"] / med["genome"],
        "genome_slower_by_s": med["genome"] - med["pairs"],
        "genome_within_baseline_spread": med["genome"] - med["pairs"] <= max(times["pairs"]) - min(times["pairs"]),
        "genome_s_all": times["genome"], "pairs_s_all": times["pairs"],
        "tile_pairs_total": stats["tiles_total"], "tile_pairs_skipped": stats["tiles_skipped"], "launches": stats["launches"],
        "batches": stats["batches"], "skipped_share": stats["tiles_skipped"] / max(1, stats["tiles_total"]),
        "rows_equal": rows["genome"] == rows["pairs"], "rows_per_tag": by_tag,
    }
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
