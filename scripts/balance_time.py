"""Balancing timing, ICE and NEWTON: mustache_amd.balance on a synthetic chr1 at 1 kb, full intra-chromosomal map.

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
  - the NumPy restatement (tests/balance_reference.py) on the same map: filter stage + `--ref-iters` iterations (0: skipped);
  - "compare": ICE against NEWTON on this map ("whole_chromosome") and on a banded one ("banded": what a real map looks like
    to the iteration -- 200 diagonals of Poisson counts with a 1/(1 + d) decay times a bin coverage, plus sparse long-range
    pixels and some empty bins, n = 248 956; `--no-banded` leaves it out).  For each: ICE iterations and seconds to its own
    stop (ice() defaults), NEWTON mat-vecs and seconds (newton() defaults), both timed around the iteration alone on a
    prepared CSR (warm: each ran once before; the median of 7 runs, with the fastest and slowest), ms per NEWTON step (one
    mat-vec plus its vector stages, the state reads every STEPS_PER_READ steps included) against ms per ICE iteration timed
    the same way, and the largest relative difference of the two bias vectors.
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
from mustache_amd.balance import BalanceCSR, ice, mad_mask, newton  # noqa: E402

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


def synth_banded(n, seed, dev, band=200, depth=40.0, sparse_per_bin=0.7, empty=0.003):
    """The banded map of the module docstring (tests/balance_reference.py synth_full_map at scale) as device tensors."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    cov = 0.5 + torch.rand(n, generator=g, device=dev, dtype=torch.float64)
    cov[torch.randperm(n, generator=g, device=dev)[:int(empty * n)]] = 0.0
    xs, ys, vs = [], [], []
    for d in range(band):
        x = torch.arange(n - d, device=dev)
        c = torch.poisson(depth / (1.0 + d) * cov[:n - d] * cov[d:], generator=g)
        k = c > 0
        xs.append(x[k]); ys.append(x[k] + d); vs.append(c[k])
    m = int(sparse_per_bin * n)
    a = torch.randint(0, n, (m,), generator=g, device=dev)
    b = torch.randint(0, n, (m,), generator=g, device=dev)
    k = (cov[a] > 0) & (cov[b] > 0) & ((a - b).abs() >= band)
    xs.append(torch.minimum(a, b)[k]); ys.append(torch.maximum(a, b)[k])
    vs.append(torch.randint(1, 4, (m,), generator=g, device=dev).to(torch.float64)[k])
    return torch.cat(xs), torch.cat(ys), torch.cat(vs)


REPEATS = 7


def _iteration_alone(csr, w0, run):
    """(median, min, max) seconds of run(csr, w) on a fresh copy of w0 over REPEATS runs, after one untimed run"""
    run(csr, w0.clone())
    ts = []
    for _ in range(REPEATS):
        w = w0.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = run(csr, w)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return (float(np.median(ts)), min(ts), max(ts)), r


def compare(x, y, v, n, dev):
    """ICE against NEWTON on one map (see the module docstring)."""
    b_ice, i_ice = ice(x, y, v, n)
    b_new, i_new = newton(x, y, v, n)
    ok = ~i_ice["masked"]
    csr = BalanceCSR(x, y, v, n, ignore_diags=2, device=dev)
    w = torch.ones(n, dtype=torch.float64, device=dev)
    _, nnz = csr.marginals(w, with_nnz=True)
    m, _ = csr.marginals((nnz >= 10).to(torch.float64))
    w0 = torch.from_numpy((~mad_mask(m.cpu().numpy(), 5.0)).astype(np.float64)).to(dev)
    ice_s, (its, _var, _conv) = _iteration_alone(csr, w0, lambda c, w: c.iterate(w, 200, 1e-5))
    new_s, (st, _trace) = _iteration_alone(csr, w0, lambda c, w: c.newton(w, 2000, 1e-6))
    steps = st.matvecs + 1                        # the start step's mat-vec is not counted
    return {"kept_pixels": csr.kept, "csr_entries": csr.nnz, "masked": int(i_ice["masked"].sum()),
            "ice_iterations": its, "ice_converged": bool(i_ice["converged"]), "ice_variance": i_ice["variance"],
            "ice_iterate_s": round(ice_s[0], 5), "ice_iterate_s_min_max": [round(t, 5) for t in ice_s[1:]],
            "ms_per_ice_iteration": round(1e3 * ice_s[0] / its, 4),
            "newton_matvecs": int(st.matvecs), "newton_outer_iterations": int(st.iterations),
            "newton_converged": bool(st.converged), "newton_residual": float(np.sqrt(st.rout)),
            "newton_capped_steps": int(st.capped_steps), "newton_iterate_s": round(new_s[0], 5),
            "newton_iterate_s_min_max": [round(t, 5) for t in new_s[1:]],
            "ms_per_newton_step": round(1e3 * new_s[0] / steps, 4),
            "masks_equal": bool(np.array_equal(i_ice["masked"], i_new["masked"])),
            "max_rel_bias_difference_ice_vs_newton": float(np.max(np.abs(b_ice[ok] / b_new[ok] - 1.0))) if ok.any() else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-banded", action="store_true")
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

    ref_s = float("nan")
    if args.ref_iters > 0:
        import balance_reference as br
        xh, yh, vh = x.cpu().numpy(), y.cpu().numpy(), v.cpu().numpy()
        t0 = time.perf_counter()
        br.ice(xh, yh, vh, n, max_iter=args.ref_iters)
        ref_s = time.perf_counter() - t0
        del xh, yh, vh

    cmp = {"whole_chromosome": compare(x, y, v, n, dev)}
    del x, y, v
    torch.cuda.empty_cache()
    if not args.no_banded:
        cmp["banded"] = compare(*synth_banded(n, 2, dev), n, dev)

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
        "compare": cmp,
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
