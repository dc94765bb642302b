#!/usr/bin/env python3
"""Whole-genome balancing (mustache_amd/balance_genome.py) stage by stage, on device-resident records.

The genome is scripts/trans_genome_time.py's: 8 chromosomes of 5200 .. 600 bins, 28 trans pairs from tests/trans_reference.py's
synth_trans with densities from 0.0005 to 0.05 -- plus cis bands (the diagonals 2 .. 200 of every chromosome, Poisson(200 /
(1 + d)) counts).  No file is read: the stages timed are what follows the read.

  assemble   the records -> (lo, hi, v) genome coordinates (torch)
  csr        balance.BalanceCSR on the assembled set (the sort, both triangles, the chunk table)
  iterate    the filter stage, the NEWTON iteration, kappa and the bias on that CSR
  apply      mst_balance_apply_pairs over all 28 pairs in one launch
  apply_big  the same launch over the batch repeated until it holds >= 32 M records (the kernel at a size where its traffic,
             not its launch, sets the time)

Each stage: HIP events around it, 3 warm-ups, the median of 20.  The apply kernel is set against its traffic model: 16 bytes
read and 8 written per record, the bias vector once (its gathers stay in cache), at the 6.3 TB/s the project measures against.
One JSON line is printed and written to profiles/balance_genome_time.json.  Needs the GPU: there is no other path.
"""
import argparse
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BINS = [5200, 4100, 3300, 2600, 2100, 1500, 900, 600]
PEAK_BYTES_PER_S = 6.3e12
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "balance_genome_time.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import trans_reference as tr
    from mustache_amd import balance
    from mustache_amd.balance_genome import apply_pairs, genome_layout
    if not torch.cuda.is_available():
        raise SystemExit("balance_genome_time.py needs the GPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    _, offsets, n = genome_layout([b * 10000 - 1 for b in BINS], 10000)
    rng = np.random.default_rng(3)
    cis = []
    for c, nc in enumerate(BINS):
        i = np.repeat(np.arange(nc), 199)
        d = np.tile(np.arange(2, 201), nc)
        keep = i + d < nc
        i, d = i[keep], d[keep]
        cnt = rng.poisson(200.0 / (1 + d)).astype(np.float64)
        keep = cnt > 0
        cis.append(tuple(torch.from_numpy(a).to(dev) for a in (i[keep], (i + d)[keep], cnt[keep])))
    combos = list(itertools.combinations(range(len(BINS)), 2))
    densities = np.geomspace(0.0005, 0.05, len(combos))
    pairs = []
    for k, (a, b) in enumerate(combos):
        x, y, v = tr.synth_trans(BINS[a], BINS[b], density=float(densities[k]), nloops=10, seed=100 + k)
        pairs.append(tuple(torch.from_numpy(t).to(dev) for t in (x.astype(np.int32), y.astype(np.int32), v)))

    def assemble():
        los = [x + offsets[c] for c, (x, _, _) in enumerate(cis)] + [p[0].to(torch.int64) + offsets[a] for p, (a, _) in zip(pairs, combos)]
        his = [y + offsets[c] for c, (_, y, _) in enumerate(cis)] + [p[1].to(torch.int64) + offsets[b] for p, (_, b) in zip(pairs, combos)]
        return torch.cat(los), torch.cat(his), torch.cat([c[2] for c in cis] + [p[2] for p in pairs])

    assemble_ms, (lo, hi, v) = timed(assemble)
    csr_ms, csr = timed(lambda: balance.BalanceCSR(lo, hi, v, n, ignore_diags=0, device=dev))
    info_box = {}

    def iterate():
        w = torch.ones(n, dtype=torch.float64, device=dev)
        _, nnz = csr.marginals(w, with_nnz=True)
        w = (nnz >= 10).to(torch.float64)
        m, _ = csr.marginals(w)
        masked = balance.mad_mask(m.cpu().numpy(), 5.0)
        w = torch.from_numpy((~masked).astype(np.float64)).to(dev)
        st, _ = csr.newton(w, 2000, 1e-6)
        b, kappa = csr.bias(w)
        info_box.update(matvecs=int(st.matvecs), iterations=int(st.iterations), converged=bool(st.converged),
                        masked=int(masked.sum()), kappa=kappa)
        return b

    iterate_ms, bias = timed(iterate)

    lens = [int(p[2].numel()) for p in pairs]
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    x, y, vv = (torch.cat([p[k] for p in pairs]) for k in range(3))
    seg_d = torch.from_numpy(seg).to(dev)
    row = torch.tensor([offsets[a] for a, _ in combos], dtype=torch.int64, device=dev)
    col = torch.tensor([offsets[b] for _, b in combos], dtype=torch.int64, device=dev)
    out = torch.empty_like(vv)
    apply_ms, _ = timed(lambda: apply_pairs(x, y, vv, seg_d, row, col, bias, out=out))
    N = int(vv.numel())
    kept = int((out > 0).sum().item())

    K = -(-(32 << 20) // N)                                   # repeat the batch: K * 28 segments, K * N records
    xb, yb, vb = x.repeat(K), y.repeat(K), vv.repeat(K)
    segb = torch.from_numpy(np.concatenate([[0], np.cumsum(np.tile(lens, K))]).astype(np.int64)).to(dev)
    outb = torch.empty_like(vb)
    big_ms, _ = timed(lambda: apply_pairs(xb, yb, vb, segb, row.repeat(K), col.repeat(K), bias, out=outb))
    same = bool(torch.equal(outb[:N], out))

    def model_ms(records):
        return (records * 24 + n * 8) / PEAK_BYTES_PER_S * 1e3

    result = {
        "device": torch.cuda.get_device_name(dev), "bins": n, "chromosomes": len(BINS), "pairs": len(pairs),
        "cis_pixels": sum(int(c[2].numel()) for c in cis), "trans_records": N, "csr_nnz": int(csr.nnz),
        "warmup": WARMUP, "reps": REPS,
        "assemble_ms": assemble_ms, "csr_ms": csr_ms, "iterate_ms": iterate_ms, "newton": info_box,
        "apply_ms": apply_ms, "apply_model_ms": model_ms(N), "apply_over_model": apply_ms / model_ms(N), "apply_kept": kept,
        "apply_big_records": K * N, "apply_big_segments": K * len(pairs), "apply_big_ms": big_ms,
        "apply_big_model_ms": model_ms(K * N), "apply_big_over_model": big_ms / model_ms(K * N),
        "apply_big_tb_per_s": (K * N * 24 + n * 8) / (big_ms * 1e-3) / 1e12, "apply_big_same_values": same,
    }
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
