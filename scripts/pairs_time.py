#!/usr/bin/env python3
"""Read pairs -> pixels (mustache_amd/pairs.py, csrc/mst_pairs.hip) stage by stage, on device-resident synthetic positions.

No file is read.  One chr1-shaped chromosome (248 956 422 bp) at 5 kb and at 1 kb; --rows read pairs (default 50 M) whose
first position is uniform over the chromosome and whose separation is log-uniform between 1 bp and the chromosome's length (the
1 / s decay of real maps), once sorted by (pos1, pos2) as a pairs file is and once shuffled.  For each of the four inputs:

  zero      clearing the counter array [K][n] (K = min(D + 1, n, budget // (4 n)), D = 2 Mb / res)
  bin       mst_pairs_bin
  compact   mst_pairs_compact
  far       the far list: one torch sort of the keys and the sums of equal keys (pairs.sum_far_list)
  torch     the plain torch form on the same tensors: keys, sort, unique_consecutive(return_counts=True)

Each stage: HIP events around it, 3 warm-ups, the median of 20.  `ratio` = torch / (zero + bin + compact + far): above 1 the
kernels win.  `dense_adds` = the integer atomic adds mst_pairs_bin issued into the counter array (one per run of equal pixels
within a wave), `dense_add_bytes_per_s` = 4 bytes each over the kernel's whole time -- a rate observed inside this kernel, which
also loads, bins and writes the far list in that time; it is not a ceiling of the integer atomic unit.
One JSON line is printed and written to profiles/pairs_time.json.  Needs the GPU: there is no other path.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LENGTH = 248956422
DISTANCE_BP = 2000000
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


def positions(rows, seed, device):
    """(pos1, pos2) int32, 1-based, pos1 <= pos2, sorted by (pos1, pos2)"""
    import math
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    p1 = torch.randint(1, LENGTH + 1, (rows,), generator=g, device=device, dtype=torch.int64)
    s = torch.exp(torch.rand(rows, generator=g, device=device, dtype=torch.float64) * math.log(LENGTH)).to(torch.int64)
    p2 = torch.clamp(p1 + s, max=LENGTH)
    order = torch.argsort(p1 * (LENGTH + 1) + p2)
    return p1[order].to(torch.int32), p2[order].to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs_time.json"))
    args = ap.parse_args()

    import torch
    from mustache_amd import _lib, pairs
    from mustache_amd._lib import ptr, stream
    if not torch.cuda.is_available():
        raise SystemExit("pairs_time.py needs the GPU")
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = args.rows
    s1, s2 = positions(rows, 11, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(12)
    perm = torch.randperm(rows, generator=g, device=dev)
    inputs = {"sorted": (s1, s2), "shuffled": (s1[perm], s2[perm])}
    del perm
    result = {"device": torch.cuda.get_device_name(dev), "rows": rows, "length_bp": LENGTH, "warmup": WARMUP, "reps": REPS, "cases": []}
    for res in (5000, 1000):
        n = (LENGTH - 1) // res + 1
        D = DISTANCE_BP // res
        K = pairs.dense_diagonals(n, D, pairs.dense_budget(dev))
        for order, (p1, p2) in inputs.items():
            dense = torch.zeros(K * n, dtype=torch.int32, device=dev)
            far_key = torch.empty(rows, dtype=torch.int64, device=dev)
            far_mult = torch.empty(rows, dtype=torch.int32, device=dev)
            counters = torch.zeros(2, dtype=torch.int64, device=dev)
            room = min(rows, K * n)
            ox, od, oc = (torch.empty(room, dtype=torch.int32, device=dev) for _ in range(3))
            found = torch.zeros(1, dtype=torch.int64, device=dev)
            ws = torch.empty(int(lib.mst_pairs_compact_workspace_bytes(K, n)), dtype=torch.uint8, device=dev)

            def clear():
                dense.zero_()
                counters.zero_()

            def bin_rows():
                counters.zero_()                     # 16 bytes: the far list's slots start at 0 in every run
                _lib.check(lib.mst_pairs_bin(ptr(p1), ptr(p2), rows, res, 0, LENGTH, n, K, ptr(dense), ptr(far_key), ptr(far_mult), rows,
                                             ptr(counters), stream()))

            def compact():
                _lib.check(lib.mst_pairs_compact(ptr(dense), K, n, ptr(ox), ptr(od), ptr(oc), room, ptr(found), ptr(ws), ws.numel(),
                                                 stream()))

            def plain_torch():
                b1, b2 = (p1.to(torch.int64) - 1) // res, (p2.to(torch.int64) - 1) // res
                key = torch.minimum(b1, b2) * n + torch.maximum(b1, b2)
                key, _ = torch.sort(key)
                return torch.unique_consecutive(key, return_counts=True)

            zero_ms, _ = timed(clear)
            # the counter array adds up over the repeated runs (its time does not depend on what it holds); the run that is
            # read below starts from a cleared array
            bin_ms, _ = timed(bin_rows)
            clear()
            bin_rows()
            far_entries, dropped = (int(v) for v in counters.cpu().tolist())
            compact_ms, _ = timed(compact)
            dense_pixels = int(found.item())
            far_ms, (uk, _) = timed(lambda: pairs.sum_far_list(far_key[:far_entries], far_mult[:far_entries]))
            torch_ms, (tk, tc) = timed(plain_torch)
            pixels = int(tk.numel())
            assert dense_pixels + int(uk.numel()) == pixels and dropped == 0 and int(tc.sum()) == rows
            # the runs of equal pixels within a wave: what mst_pairs_bin turns into one write each
            b1, b2 = (p1.to(torch.int64) - 1) // res, (p2.to(torch.int64) - 1) // res
            key = torch.minimum(b1, b2) * n + torch.maximum(b1, b2)
            head = torch.ones(rows, dtype=torch.bool, device=dev)
            head[1:] = key[1:] != key[:-1]
            head[::64] = True
            runs = int(head.sum().item())
            del b1, b2, key, head, uk, tk, tc
            ours = zero_ms + bin_ms + compact_ms + far_ms
            dense_adds = runs - far_entries
            result["cases"].append({
                "res": res, "order": order, "n": n, "dense_diags": K, "pixels": pixels, "dense_pixels": dense_pixels,
                "far_entries": far_entries, "runs": runs, "dense_adds": dense_adds,
                "zero_ms": round(zero_ms, 3), "bin_ms": round(bin_ms, 3), "compact_ms": round(compact_ms, 3), "far_ms": round(far_ms, 3),
                "kernels_ms": round(ours, 3), "torch_ms": round(torch_ms, 3), "ratio": round(torch_ms / ours, 3),
                "bin_rows_per_s": round(rows / (bin_ms * 1e-3)), "dense_add_bytes_per_s": round(4 * dense_adds / (bin_ms * 1e-3)),
            })
            print(json.dumps(result["cases"][-1]), file=sys.stderr, flush=True)
            del dense, far_key, far_mult, ox, od, oc, ws
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
