#!/usr/bin/env python3
"""Trans read pairs -> per-pair pixels (mustache_amd/pairs.py, csrc/mst_pairs_trans.hip) stage by stage, on device-resident
synthetic rows.

No file is read.  An hg19-shaped table (chr1 .. chr22, chrX, chrY: 276 pairs); --rows trans rows (default 50 M) dealt to the
pairs in proportion to len_a * len_b, both positions uniform over their chromosome (a trans map has no distance decay), laid
pair-major as the reader lays them -- once sorted by (posA, posB) within each pair, as a sorted pairs file gives them, and once in
random order within each pair.  Two resolutions: 100 kb, where the counter array of every cell (4 bytes each) fits
pairs.dense_budget() and everything is dense, and 10 kb, where it does not and everything goes through the far list; at 100 kb
the far path is timed as well (dense_cells = 0), which is what decides bin_trans_device's default.  For each input:

  zero      clearing the counter array [dense_cells]
  bin       mst_pairs_bin_trans
  compact   mst_pairs_trans_compact
  far       the far list: one torch sort of the keys and the sums of equal keys (pairs.sum_far_list)
  decode    mst_pairs_trans_decode on the unique keys
  torch     the plain torch form on the same tensors: the rows' pair from seg_off, keys, sort,
            unique_consecutive(return_counts=True)

Each stage: HIP events around it, 3 warm-ups, the median of 20.  `ratio` = torch / (zero + bin + compact + far): above 1 the
kernels win (decode is left out of both sides: the torch form stops at keys and counts too).  One JSON line is printed and
written to profiles/pairs_trans_time.json.  Needs the GPU: there is no other path.  Not measured here: the host parse with
keep_trans, and a real file.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HG19 = [249250621, 243199373, 198022430, 191154276, 180915260, 171115067, 159138663, 146364022, 141213431, 135534747, 135006516,
        133851895, 115169878, 107349540, 102531392, 90354753, 81195210, 78077248, 59128983, 63025520, 48129895, 51304566, 155270560,
        59373566]
WARMUP, REPS = 3, 20


def timed(fn):
    """(median ms of REPS runs after WARMUP, the last result)"""
    import torch
    ms, out = [], None
    for i in range(WARMUP + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        if i >= WARMUP:
            ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2], out


def rows_of(rows, seed, device):
    """(posA, posB int32 pair-major in random order within each pair, seg_off int64 host array, the rows' pair int64)"""
    import numpy as np
    import torch
    from mustache_amd.pairs import pair_list
    pairs = pair_list(len(HG19))
    weight = np.array([HG19[a] * HG19[b] for a, b in pairs], np.float64)
    counts = np.floor(weight / weight.sum() * rows).astype(np.int64)
    counts[0] += rows - int(counts.sum())
    seg_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    pair = torch.repeat_interleave(torch.arange(len(pairs), device=device), torch.from_numpy(counts).to(device))
    len_a = torch.tensor([HG19[a] for a, _ in pairs], dtype=torch.float64, device=device)[pair]
    len_b = torch.tensor([HG19[b] for _, b in pairs], dtype=torch.float64, device=device)[pair]
    pa = (torch.rand(rows, generator=g, device=device, dtype=torch.float64) * len_a).to(torch.int64) + 1      # 1-based, <= length
    pb = (torch.rand(rows, generator=g, device=device, dtype=torch.float64) * len_b).to(torch.int64) + 1
    return pa.to(torch.int32), pb.to(torch.int32), seg_off, pair


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs_trans_time.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from mustache_amd import _lib, pairs
    from mustache_amd._lib import ptr, stream
    if not torch.cuda.is_available():
        raise SystemExit("pairs_trans_time.py needs the GPU")
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = args.rows
    ra, rb, seg_off, pair = rows_of(rows, 11, dev)
    # by (pair, posA, posB): a stable sort by posB first, then a stable one by (pair, posA)
    by_b = torch.argsort(rb.to(torch.int64), stable=True)
    order = by_b[torch.argsort((pair[by_b] << 31) | ra[by_b].to(torch.int64), stable=True)]
    inputs = {"sorted": (ra[order].contiguous(), rb[order].contiguous()), "shuffled": (ra, rb)}
    del order, by_b
    P = len(seg_off) - 1
    seg_d = torch.from_numpy(seg_off).to(dev)
    result = {"device": torch.cuda.get_device_name(dev), "rows": rows, "pairs": P, "warmup": WARMUP, "reps": REPS, "cases": []}
    for res in (100000, 10000):
        bins = [length // res + 1 for length in HG19]
        tables, cells = pairs.trans_tables(HG19, bins)
        fits = 4 * cells <= pairs.dense_budget(dev)
        t = torch.from_numpy(tables).to(dev)
        lim_a, lim_b, n_a, n_b, cell_off = (t[k] for k in range(5))
        for mode in (("dense", "far") if fits else ("far",)):
            dense_cells = cells if mode == "dense" else 0
            for name, (pa, pb) in inputs.items():
                dense = torch.zeros(dense_cells, dtype=torch.int32, device=dev)
                far_key = torch.empty(rows, dtype=torch.int64, device=dev)
                far_mult = torch.empty(rows, dtype=torch.int32, device=dev)
                counters = torch.zeros(P + 1, dtype=torch.int64, device=dev)
                room = min(rows, dense_cells)
                ok, oc = torch.empty(room, dtype=torch.int64, device=dev), torch.empty(room, dtype=torch.int32, device=dev)
                found = torch.zeros(1, dtype=torch.int64, device=dev)
                ws = torch.empty(int(lib.mst_pairs_trans_compact_workspace_bytes(dense_cells)), dtype=torch.uint8, device=dev)

                def clear():
                    dense.zero_()
                    counters.zero_()

                def bin_rows():
                    counters.zero_()                 # the far list's slots start at 0 in every run
                    _lib.check(lib.mst_pairs_bin_trans(ptr(pa), ptr(pb), rows, ptr(seg_d), P, ptr(lim_a), ptr(lim_b), ptr(n_a), ptr(n_b),
                                                       ptr(cell_off), res, 0, dense_cells, ptr(dense) if dense_cells else None,
                                                       ptr(far_key), ptr(far_mult), rows, ptr(counters[P:]), ptr(counters), stream()))

                def compact():
                    _lib.check(lib.mst_pairs_trans_compact(ptr(dense) if dense_cells else None, dense_cells, ptr(ok), ptr(oc), room,
                                                           ptr(found), ptr(ws), ws.numel(), stream()))

                def plain_torch():
                    p = torch.searchsorted(seg_d, torch.arange(rows, device=dev), right=True) - 1
                    x, y = (pa.to(torch.int64) - 1) // res, (pb.to(torch.int64) - 1) // res
                    key, _ = torch.sort(cell_off[p] + x * n_b[p] + y)
                    return torch.unique_consecutive(key, return_counts=True)

                zero_ms, _ = timed(clear)
                # the counter array adds up over the repeated runs (its time does not depend on what it holds); the run that is
                # read below starts from a cleared array
                bin_ms, _ = timed(bin_rows)
                clear()
                bin_rows()
                counted = counters.cpu().tolist()
                far_entries, dropped = int(counted[P]), int(sum(counted[:P]))
                compact_ms, _ = timed(compact)
                dense_pixels = int(found.item())
                far_ms, (uk, uc) = timed(lambda: pairs.sum_far_list(far_key[:far_entries], far_mult[:far_entries]))
                keys = torch.cat([ok[:dense_pixels], uk])
                counts = torch.cat([oc[:dense_pixels].to(torch.int64) & 0xFFFFFFFF, uc])
                x, y, v = (torch.empty(keys.numel(), dtype=d, device=dev) for d in (torch.int32, torch.int32, torch.float64))
                decode_ms, _ = timed(lambda: _lib.check(lib.mst_pairs_trans_decode(ptr(keys), ptr(counts), keys.numel(), ptr(cell_off),
                                                                                  ptr(n_b), P, ptr(x), ptr(y), ptr(v), stream())))
                torch_ms, (tk, tc) = timed(plain_torch)
                assert torch.equal(tk, keys) and torch.equal(tc, counts) and dropped == 0 and int(v.sum().item()) == rows
                ours = zero_ms + bin_ms + compact_ms + far_ms
                result["cases"].append({
                    "res": res, "mode": mode, "order": name, "cells": cells, "dense_cells": dense_cells, "pixels": int(tk.numel()),
                    "dense_pixels": dense_pixels, "far_entries": far_entries,
                    "zero_ms": round(zero_ms, 3), "bin_ms": round(bin_ms, 3), "compact_ms": round(compact_ms, 3),
                    "far_ms": round(far_ms, 3), "decode_ms": round(decode_ms, 3), "kernels_ms": round(ours, 3),
                    "total_ms": round(ours + decode_ms, 3), "torch_ms": round(torch_ms, 3), "ratio": round(torch_ms / ours, 3),
                    "bin_rows_per_s": round(rows / (bin_ms * 1e-3)),
                })
                print(json.dumps(result["cases"][-1]), file=sys.stderr, flush=True)
                del dense, far_key, far_mult, ok, oc, ws, uk, uc, keys, counts, x, y, v, tk, tc
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
