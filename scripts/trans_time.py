"""Time one inter-chromosomal pair at the size of chr1 x chr2 at 10 kb (mustache_amd/trans.py): n1 x n2 bins, a random
`density` share of the pixels holding a log-normal value, already on the device.  Prints one JSON line: the single-pair z-score
on its own (trans.zscore_device) and the whole call (trans.call_trans_coo), wall-clock seconds after one warm-up call.

    python scripts/trans_time.py [--n1 24896] [--n2 24220] [--density 0.05] [--reps 2]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n1", type=int, default=24896)          # chr1 at 10 kb (hg38: 248 956 422 bp)
    ap.add_argument("--n2", type=int, default=24220)          # chr2 at 10 kb (242 193 529 bp)
    ap.add_argument("--density", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import torch
    from mustache_amd.trans import call_trans_coo, trans_tiling, zscore_device
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(a.seed)
    k = int(a.n1 * a.n2 * a.density)
    flat = torch.unique(torch.randint(0, a.n1 * a.n2, (k,), device=dev, generator=g))
    x = (flat // a.n2).to(torch.int32)
    y = (flat % a.n2).to(torch.int32)
    v = torch.exp(torch.randn(flat.numel(), device=dev, dtype=torch.float64, generator=g) * 0.5)
    C, (rs, _), (cs, _) = trans_tiling(int(x.max()) + 1, int(y.max()) + 1)
    times = []
    loops = None
    for r in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.time()
        zscore_device(v, dev)
        torch.cuda.synchronize()
        t1 = time.time()
        loops = call_trans_coo(x, y, v, [1.6, 3.2], 0.88, 0.2)
        torch.cuda.synchronize()
        t2 = time.time()
        if r:
            times.append((t1 - t0, t2 - t1))
    best = min(times, key=lambda t: t[1])
    print(json.dumps({"n1": a.n1, "n2": a.n2, "records": int(flat.numel()), "tiles": len(rs) * len(cs), "tile": C,
                      "zscore_s": round(best[0], 4), "pair_s": round(best[1], 4),
                      "gpix_per_s": round(len(rs) * len(cs) * C * C / best[1] / 1e9, 2), "loops": len(loops),
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
