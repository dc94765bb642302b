"""Segmented inter-chromosomal pile-up timing on one MI355X: the batched call (pileup.pileup_trans_batch: mst_pileup_trans_batch +
mst_pileup_reduce_segmented, one host wait) beside the loop of per-pair pileup.pileup_trans_records calls on the same records and
loops -- the per-pair path: a loop of batches of one pair each through the same kernels, one host wait per pair.  Device events
around each, the host wait included; median of --steps after --warmup.  The per-pair loop gets the records already filtered by
v > 0 and cut per pair (the batch takes them concatenated and unfiltered), so its own boolean indexing is not charged to it.
  case "genome"  276 pairs (24 chromosomes of 80 .. 1 250 bins, as a human genome at 200 kb), 20 records per 1 000 cells, 40 loops
                 per pair, w = 10: many small pairs.
  case "pair"    the single pair of scripts/pileup_trans_time.py (24 900 x 24 300 bins, --records records, default 5e7, 2 000
                 loops) as a batch of one, beside pileup_trans_records on the filtered records; the per-pair path is timed twice,
                 for its run-to-run spread.
profiles/pileup_trans_batch_time_parent.json holds three runs (two plain, one with --records 1000000) from the commit that still
had single-pair kernels behind pileup_trans_records; profiles/pileup_trans_batch_time.json the same three runs of this code.
Prints one JSON line.
python scripts/pileup_trans_batch_time.py [--steps 20] [--warmup 3] > profiles/pileup_trans_batch_time.json"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mustache_amd import pileup as pl                      # noqa: E402


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
    return {"median_ms": round(float(np.median(out)), 4), "min_ms": round(float(min(out)), 4), "max_ms": round(float(max(out)), 4)}


def case(dims, records, loops_per_pair, w, q, steps, warmup, dev, seed):
    """records / loops of every pair drawn on the device / host; a twentieth of the values are 0.0 (what the balancing leaves of a
    masked bin).  -> the timings of the batch and of the per-pair loop (twice), and whether their aggregates have the same bytes."""
    g = torch.Generator(device=dev).manual_seed(seed)
    rng = np.random.default_rng(seed)
    recs, loops = [], []
    for (n1, n2), n in zip(dims, records):
        x = torch.randint(0, n1, (n,), generator=g, device=dev, dtype=torch.int32)
        y = torch.randint(0, n2, (n,), generator=g, device=dev, dtype=torch.int32)
        v = torch.exp(0.5 * torch.randn(n, generator=g, device=dev, dtype=torch.float64))
        v[torch.rand(n, generator=g, device=dev) < 0.05] = 0.0
        recs.append((x, y, v))
        loops.append((rng.integers(0, n1, loops_per_pair).astype(np.int64), rng.integers(0, n2, loops_per_pair).astype(np.int64)))
    seg = np.concatenate([[0], np.cumsum(records)]).astype(np.int64)
    cx, cy, cv = (torch.cat([r[k] for r in recs]) for k in range(3))
    kept = [tuple(t[r[2] > 0] for t in r) for r in recs]     # the per-pair path's input: filtered, one tensor triple per pair
    torch.cuda.synchronize()

    def batch():
        return pl.pileup_trans_batch(cx, cy, cv, seg, dims, loops, w, q)

    def per_pair():
        return [pl.pileup_trans_records(x, y, v, n1, n2, xs, ys, w, q) for (x, y, v), (n1, n2), (xs, ys) in zip(kept, dims, loops)]
    a, b = batch(), per_pair()
    same = all(p["sum_oe"].tobytes() == s["sum_oe"].tobytes() and p["p2ll"].tobytes() == s["p2ll"].tobytes() for p, s in zip(a, b))
    del a, b
    out = {"pairs": len(dims), "records": int(seg[-1]), "loops": loops_per_pair * len(dims), "w": w, "same_bytes": bool(same),
           "batch": timed(batch, steps, warmup), "per_pair": timed(per_pair, steps, warmup),
           "per_pair_again": timed(per_pair, steps, warmup)}
    out["per_pair_over_batch"] = round(out["per_pair"]["median_ms"] / out["batch"]["median_ms"], 3)
    out["per_pair_spread_ms"] = round(abs(out["per_pair"]["median_ms"] - out["per_pair_again"]["median_ms"]), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--records", type=int, default=50_000_000, help="records of the single large pair")
    ap.add_argument("--loops", type=int, default=2000, help="loops of the single large pair")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    w, q = 10, 6
    bins = np.linspace(1250, 80, 24).astype(int)             # 24 chromosomes at 200 kb: 250 Mb down to 16 Mb
    dims = [(int(bins[i]), int(bins[j])) for i in range(24) for j in range(i + 1, 24)]
    genome = case(dims, [n1 * n2 // 50 for n1, n2 in dims], 40, w, q, a.steps, a.warmup, dev, 1)
    pair = case([(24900, 24300)], [a.records], a.loops, w, q, a.steps, a.warmup, dev, 2)
    print(json.dumps({"metric": "pileup_trans_batch_ms", "steps": a.steps, "warmup": a.warmup, "genome": genome, "pair": pair}))


if __name__ == "__main__":
    main()
