"""ICE balancing timing: mustache_amd.balance on a synthetic chr1 at 1 kb, full intra-chromosomal map.

    python scripts/balance_time.py [--kept 105000000] [--ref-iters 3]      (GPU box; ~20 GB of device memory)

The map: n = 248 956 bins, distinct pixels (i, i + d), d >= 2 drawn from a 1/d law over the whole chromosome, i drawn in
proportion to a log-normal bin coverage (sigma 0.8), so row lengths are skewed (many rows longer than one 1024-entry chunk,
some far shorter) and the iteration has work to do; records are drawn until `--kept` distinct pixels exist.  Printed:
  - prepare: de-duplication, the sort into the full symmetric CSR and the chunk offsets (torch), timed around BalanceCSR, cold
    (the first call of the process: torch's sort kernels and the allocator warm up) and warm (a second call);
  - the row-length spread of the CSR;
  - the ICE run (ice() as the command line calls it): prepare + filter stage, iterations + bias, the iteration count;
  - ms per iteration from HIP events around 20 iterations that cannot converge (tol < 0), and the achieved bytes per second of
    the iteration against the 6.29 TB/s copy rate, with the traffic model 12 B per CSR entry (int32 column + float64 value;
    each kept off-diagonal pixel is two entries) -- the gathers of w come from L2 and are not counted;
  - the NumPy restatement (tests/balance_reference.py) on the same map: filter stage + `--ref-iters` iterations.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from mustache_amd.balance import BalanceCSR, ice  # noqa: E402

COPY_TBS = 6.29


def synth(n, kept, seed, dev):
    """`kept` distinct pixels (x, y, v), x < y, as device tensors (see the module docstring)."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    cov = torch.exp(0.8 * torch.randn(n, generator=g, device=dev, dtype=torch.float64))
    cdf = torch.cumsum(cov, 0)
    cdf = cdf / cdf[-1]
    keys = torch.zeros(0, dtype=torch.int64, device=dev)
    step = 1 << 24
    while keys.numel() < kept:
        u = torch.rand(step, generator=g, device=dev, dtype=torch.float64)
        d = torch.floor(torch.exp(u * np.log(n / 2.0)) * 2.0).to(torch.int64)        # 2 <= d < n, density ~ 1/d
        x = torch.searchsorted(cdf, torch.rand(step, generator=g, device=dev, dtype=torch.float64)).clamp_(max=n - 1)
        y = x + d
        y = torch.where(y < n, y, x - d)                   # reflected at the chromosome's end
        ok = y >= 0
        lo, hi = torch.minimum(x, y)[ok], torch.maximum(x, y)[ok]
        keys = torch.unique(torch.cat([keys, lo * n + hi]))
    keys = keys[torch.randperm(keys.numel(), generator=g, device=dev)[:kept]]
    v = 1.0 + torch.floor(-torch.log(torch.rand(kept, generator=g, device=dev, dtype=torch.float64)) * 3.0)
    return keys // n, keys % n, v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kept", type=int, default=105_000_000)
    ap.add_argument("--ref-iters", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = 248_956
    x, y, v = synth(n, args.kept, 1, dev)
    torch.cuda.synchronize()

    prep = []
    for _ in range(2):                           # cold, then warm
        t0 = time.perf_counter()
        csr = BalanceCSR(x, y, v, n, ignore_diags=2, device=dev)
        torch.cuda.synchronize()
        prep.append(time.perf_counter() - t0)
        if len(prep) == 1:
            del csr
    kept, entries = csr.kept, csr.nnz
    rl = (csr.row_ptr[1:] - csr.row_ptr[:-1]).cpu().numpy()

    w = torch.ones(n, dtype=torch.float64, device=dev)
    csr.iterate(w, 2, -1.0)                      # warm-up
    w = torch.ones(n, dtype=torch.float64, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    its, _, _ = csr.iterate(w, 20, -1.0)
    e1.record()
    torch.cuda.synchronize()
    ms_it = e0.elapsed_time(e1) / its
    del csr, w
    torch.cuda.empty_cache()

    tm = {}
    t0 = time.perf_counter()
    bias, info = ice(x, y, v, n, timings=tm)
    ice_s = time.perf_counter() - t0

    import balance_reference as br
    xh, yh, vh = x.cpu().numpy(), y.cpu().numpy(), v.cpu().numpy()
    t0 = time.perf_counter()
    br.ice(xh, yh, vh, n, max_iter=args.ref_iters)
    ref_s = time.perf_counter() - t0

    bytes_it = 12.0 * entries
    out = {
        "bins": n, "kept_pixels": kept, "csr_entries": entries,
        "prepare_cold_s": round(prep[0], 4), "prepare_warm_s": round(prep[1], 4),
        "row_entries_median": int(np.median(rl)), "row_entries_p99": int(np.percentile(rl, 99)), "row_entries_max": int(rl.max()),
        "row_entries_min": int(rl.min()), "rows_over_one_chunk": int((rl > 1024).sum()),
        "ice_total_s": round(ice_s, 4), "ice_prepare_and_filter_s": round(tm["prepare_s"], 4),
        "ice_iterate_and_bias_s": round(tm["iterate_s"], 4),
        "iterations": info["iterations"], "converged": info["converged"], "variance": info["variance"],
        "masked": int(info["masked"].sum()),
        "ms_per_iteration": round(ms_it, 4),
        "iteration_TBps_at_12B_per_entry": round(bytes_it / (ms_it * 1e-3) / 1e12, 3),
        "fraction_of_copy_rate": round(bytes_it / (ms_it * 1e-3) / 1e12 / COPY_TBS, 3),
        "restatement_s_filter_plus_%d_iterations" % args.ref_iters: round(ref_s, 2),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
