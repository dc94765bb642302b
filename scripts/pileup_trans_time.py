"""Inter-chromosomal pile-up timing on one synthetic pair built on the device (24 900 x 24 300 bins, 5e7 records, 2 000 loops,
w = 10; GPU box): device events around the record pass with everything behind it (mst_pileup_trans_windows, the kernels of
mst_pileup_trans_batch with P = 1: the table upload, loop ordering, window initialisation, records, E, finish), the reduce, and
the whole pileup_trans_records call (a batch of one pair, with the segmented reduce), median of --steps after --warmup; the
record pass's traffic model (16 B per record) and its share of 6.3 TB/s.  Prints one JSON line.
python scripts/pileup_trans_time.py [--steps 20] [--warmup 3] > profiles/pileup_trans_time.json"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mustache_amd import _lib                              # noqa: E402
from mustache_amd import pileup as pl                      # noqa: E402
from mustache_amd._lib import ptr, stream                  # noqa: E402

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
    ap.add_argument("--records", type=int, default=50_000_000)
    ap.add_argument("--loops", type=int, default=2000)
    a = ap.parse_args()
    n1, n2, w, q, N, L = 24900, 24300, 10, 6, a.records, a.loops
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randint(0, n1, (N,), generator=g, device=dev, dtype=torch.int32)
    y = torch.randint(0, n2, (N,), generator=g, device=dev, dtype=torch.int32)
    v = torch.exp(0.5 * torch.randn(N, generator=g, device=dev, dtype=torch.float64))
    rng = np.random.default_rng(0)
    xs, ys = rng.integers(0, n1, L).astype(np.int64), rng.integers(0, n2, L).astype(np.int64)
    S = 2 * w + 1
    lib = _lib.require_gpu()
    ws = torch.empty(int(lib.mst_pileup_trans_workspace_bytes(n1, n2, L, w)), dtype=torch.uint8, device=dev)
    rows, cols = torch.empty(n1, dtype=torch.uint8, device=dev), torch.empty(n2, dtype=torch.uint8, device=dev)
    E = torch.empty(1, dtype=torch.float64, device=dev)
    obs = torch.empty((L, S, S), dtype=torch.float64, device=dev)
    oe, st = torch.empty_like(obs), torch.empty((L, 3), dtype=torch.float64, device=dev)
    xd, yd = torch.from_numpy(xs).to(dev), torch.from_numpy(ys).to(dev)
    order = torch.from_numpy(np.lexsort((ys, xs)).astype(np.int32)).to(dev)

    def windows(n_records, n_loops):
        _lib.check(lib.mst_pileup_trans_windows(ptr(x), ptr(y), ptr(v), n_records, n1, n2, ptr(xd), ptr(yd), n_loops, w, q, ptr(rows),
                                                ptr(cols), ptr(E), ptr(obs), ptr(oe), ptr(st), ptr(ws), ws.numel(), stream()))
    t_win = timed(lambda: windows(N, L), a.steps, a.warmup)
    t_rest = timed(lambda: windows(0, L), a.steps, a.warmup)           # the same call without a record: everything but the pass
    t_noloop = timed(lambda: windows(N, 0), a.steps, a.warmup)         # the pass with no window to fill: flags and the exact sum
    windows(N, L)
    t_red = timed(lambda: pl.reduce(obs, oe, order, w, ws), a.steps, a.warmup)
    t_all = timed(lambda: pl.pileup_trans_records(x, y, v, n1, n2, xs, ys, w, q), a.steps, a.warmup)
    r = pl.pileup_trans_records(x, y, v, n1, n2, xs, ys, w, q)
    rec_bytes = 16 * N
    pass_ms = t_win[0] - t_rest[0]
    ms = lambda t: round(t[0], 4)                                 # noqa: E731
    print(json.dumps({
        "metric": "pileup_trans_pair_ms", "n1": n1, "n2": n2, "records": N, "loops": L, "w": w, "steps": a.steps, "warmup": a.warmup,
        "windows_call_ms": ms(t_win), "windows_call_min_max_ms": [round(t_win[1], 4), round(t_win[2], 4)],
        "windows_call_without_records_ms": ms(t_rest), "windows_call_without_loops_ms": ms(t_noloop),
        "record_pass_ms": round(pass_ms, 4), "record_bytes": rec_bytes,
        "record_pass_model_ms": round(rec_bytes / (HBM_TBS * 1e12) * 1e3, 4),
        "record_pass_TBs": round(rec_bytes / (pass_ms * 1e-3) / 1e12, 3),
        "record_pass_share_of_6p3_TBs": round(rec_bytes / (pass_ms * 1e-3) / (HBM_TBS * 1e12), 4),
        "reduce_ms": ms(t_red), "pileup_trans_records_ms": ms(t_all),
        "pileup_trans_records_min_max_ms": [round(t_all[1], 4), round(t_all[2], 4)],
        "expected": r["expected"], "P2M": r["metrics"]["P2M"], "valid_rows": int(r["valid"][0].sum().item()),
        "valid_cols": int(r["valid"][1].sum().item()),
    }))


if __name__ == "__main__":
    main()
