#!/usr/bin/env python3
"""All trans pairs of a synthetic genome, two ways on the same device-resident records:

  genome  call_trans_genome: one batch -- a segmented z-score, the tile counts, the kept tiles in shared launches
  pairs   a loop of call_trans_coo over the same pairs: 28 batches of one pair, each with its own segmented z-score, statistics
          copy, tile count and launches (the same kernels and the same skip rule; what is compared is the batching)

The genome: 8 chromosomes of 5200, 4100, 3300, 2600, 2100, 1500, 900 and 600 bins, 28 pairs from tests/trans_reference.py's
synth_trans with densities from 0.0005 to 0.05 (geometric steps in pair order), so most tiles hold fewer than 10 000 records,
as in a real trans map at a fine resolution.

Both forms run in this process after a warm-up pass of each, alternating, wall time around a device synchronise; the medians
of `--reps` passes (at least 7), the spread (max - min) of the baseline's passes, the tile counts and whether both gave the
same rows are printed as one JSON line.  Needs the GPU: there is no other path.
"""
import argparse
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BINS = [5200, 4100, 3300, 2600, 2100, 1500, 900, 600]
OCT, ST, PT = [1.6, 3.2], 0.88, 0.2


def _rows(loops):
    return [[int(a), int(b), float(q), float(s)] for a, b, q, s in loops]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    reps = max(7, args.reps)

    import numpy as np
    import torch
    import trans_reference as tr
    from mustache_amd.trans import call_trans_coo
    from mustache_amd.trans_genome import call_trans_genome
    if not torch.cuda.is_available():
        raise SystemExit("trans_genome_time.py needs the GPU")
    combos = list(itertools.combinations(range(len(BINS)), 2))
    densities = np.geomspace(0.0005, 0.05, len(combos))
    pairs = []
    for k, (a, b) in enumerate(combos):
        x, y, v = tr.synth_trans(BINS[a], BINS[b], density=float(densities[k]), nloops=10, seed=100 + k)
        pairs.append((torch.as_tensor(x.astype(np.int32)).cuda(), torch.as_tensor(y.astype(np.int32)).cuda(),
                      torch.as_tensor(v).cuda()))
    records = sum(int(p[2].numel()) for p in pairs)

    stats = {}

    def genome():
        return call_trans_genome(pairs, OCT, ST, PT, stats=stats)

    def one_by_one():
        return [call_trans_coo(x, y, v, OCT, ST, PT) for x, y, v in pairs]

    forms = (("genome", genome), ("pairs", one_by_one))
    times = {name: [] for name, _ in forms}
    rows = {}
    for i in range(args.warmup + reps):
        for name, fn in forms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = fn()
            torch.cuda.synchronize()
            if i >= args.warmup:
                times[name].append(time.perf_counter() - t0)
            rows[name] = [_rows(r) for r in got]
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    print(json.dumps({
        "pairs": len(pairs), "records": records, "reps": reps,
        "genome_s": med["genome"], "pairs_s": med["pairs"], "pairs_over_genome": med["pairs"] / med["genome"],
        "pairs_s_spread": max(times["pairs"]) - min(times["pairs"]), "genome_s_spread": max(times["genome"]) - min(times["genome"]),
        "genome_s_all": times["genome"], "pairs_s_all": times["pairs"],
        "tiles_total": stats["tiles_total"], "tiles_skipped": stats["tiles_skipped"], "launches": stats["launches"],
        "skipped_share": stats["tiles_skipped"] / max(1, stats["tiles_total"]),
        "rows_equal": rows["genome"] == rows["pairs"], "loops": sum(len(r) for r in rows["genome"]),
    }))


if __name__ == "__main__":
    main()
