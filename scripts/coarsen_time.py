#!/usr/bin/env python3
"""The coarsening kernel (mustache_amd/multires.py, csrc/mst_coarsen.hip) on the device-resident input of
scripts/downsample_time.py: the read pairs of scripts/pairs_time.py (50 M by default), binned at 5 kb by pairs.bin_pairs_device,
coarsened by the factors 2 and 5.

  coarsen        mst_coarsen_records and mst_coarsen_compact of the product library (adjacent lanes with equal keys combine
                 their counts before the atomic), the zeroing of the counters included
  coarsen_plain  the same file built with -DMST_COARSEN_PLAIN (`make -C mustache_amd/csrc coarsen_plain`): one atomic per
                 record; skipped when that library is not there
  records        multires.coarsen_records end to end: the above with its allocations, the far list's sort and sum and the
                 host's reads of the words
  torch          the obvious alternative: the coarse keys, then pairs.sum_far_list on them (one sort and a cumulative sum);
                 a yardstick only

Each: HIP events around it, 3 warm-ups, the median of 20.  The script asserts that all forms give the same pixel set.  With
`--wall FILE.pairs[.gz]` it also times `-r 5kb --coarser 10kb` on that file against the two plain runs and the host parse
alone (one run each, wall clock).  One JSON line is printed and written to profiles/coarsen_time.json (--append: added to
it, for the three invocations DESIGN records).  Needs the GPU.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

FACTORS = (2, 5)


def wall_times(path, chromosome):
    """one run each of the merged call, the two plain calls and the parse alone: seconds of wall clock"""
    import contextlib
    import io
    import tempfile
    from mustache_amd import pairs
    from mustache_amd.mustache import main as mustache
    out = {}
    with tempfile.TemporaryDirectory() as d:
        jobs = {"warm_up": ["-r", "5kb", "--coarser", "10kb"], "merged_s": ["-r", "5kb", "--coarser", "10kb"],
                "plain_5kb_s": ["-r", "5kb"], "plain_10kb_s": ["-r", "10kb"]}
        for name, extra in jobs.items():                             # the first run pays the process's first launches: not kept
            pairs.close_pairs_handles()                              # every run parses the file, as a process of its own would
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                mustache(["-f", path, "-ch", chromosome, "--balance", "ICE", "-o", os.path.join(d, name + ".tsv")] + extra)
            if name != "warm_up":
                out[name] = round(time.perf_counter() - t0, 3)
                with open(os.path.join(d, name + ".tsv")) as f:
                    out[name.replace("_s", "_loops")] = sum(1 for _ in f) - 1
        pairs.close_pairs_handles()
        t0 = time.perf_counter()
        pairs.pairs_handle(path)
        out["parse_s"] = round(time.perf_counter() - t0, 3)
        pairs.close_pairs_handles()
    out["two_plain_minus_merged_s"] = round(out["plain_5kb_s"] + out["plain_10kb_s"] - out["merged_s"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50000000)
    ap.add_argument("--plain-lib", default=os.path.join(ROOT, "mustache_amd", "libmustache_hip_coarsen_plain.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coarsen_time.json"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--wall", default=None, metavar="FILE.pairs[.gz]")
    ap.add_argument("--wall-chromosome", default="chr1")
    args = ap.parse_args()

    import torch
    from pairs_time import DISTANCE_BP, LENGTH, REPS, WARMUP, positions, timed
    from mustache_amd import _lib, multires, pairs
    from mustache_amd._lib import ptr, stream
    if not torch.cuda.is_available():
        raise SystemExit("coarsen_time.py needs the GPU")
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    res = 5000
    p1, p2 = positions(args.rows, 11, dev)
    px = pairs.bin_pairs_device(p1, p2, res, length=LENGTH, distance_bins=DISTANCE_BP // res, device=dev)
    del p1, p2
    x, dist, count = px.x.contiguous(), px.dist.contiguous(), px.count.contiguous()
    reads, records = int(count.sum().item()), int(count.numel())
    result = {"device": torch.cuda.get_device_name(dev), "rows": args.rows, "res": res, "records": records, "reads": reads,
              "warmup": WARMUP, "reps": REPS, "bytes_read_per_record": 16, "factors": {}}
    plain = None
    if os.path.exists(args.plain_lib):
        plain = ctypes.CDLL(args.plain_lib)
        for name in ("mst_coarsen_records", "mst_coarsen_compact_workspace_bytes", "mst_coarsen_compact"):
            getattr(plain, name).restype, getattr(plain, name).argtypes = _lib._SIGNATURES[name]

    for k in FACTORS:
        n = (px.n_alloc - 1) // k + 1
        K = pairs.dense_diagonals(n, DISTANCE_BP // (res * k), pairs.dense_budget(dev) // 2)
        dense = torch.zeros(K * n, dtype=torch.int64, device=dev)
        far_key = torch.empty(records, dtype=torch.int64, device=dev)
        far_count = torch.empty(records, dtype=torch.int64, device=dev)
        words = torch.zeros(3, dtype=torch.int64, device=dev)
        found = torch.zeros(1, dtype=torch.int64, device=dev)
        room = min(records, K * n)
        ox, od = (torch.empty(room, dtype=torch.int32, device=dev) for _ in range(2))
        oc = torch.empty(room, dtype=torch.int64, device=dev)
        ws = torch.empty(int(lib.mst_coarsen_compact_workspace_bytes(K, n)), dtype=torch.uint8, device=dev)

        def kernels(library):
            def run():
                dense.zero_()
                words.zero_()
                _lib.check(library.mst_coarsen_records(ptr(x), ptr(dist), ptr(count), 0, records, k, n, K, ptr(dense), ptr(far_key),
                                                       ptr(far_count), records, ptr(words), stream()))
                _lib.check(library.mst_coarsen_compact(ptr(dense), K, n, ptr(ox), ptr(od), ptr(oc), room, ptr(found), ptr(ws),
                                                       ws.numel(), stream()))
            return run

        def pixel_set(X, D, C):
            key, order = torch.sort(X.to(torch.int64) * n + X.to(torch.int64) + D.to(torch.int64))
            return key, C[order]

        def collected():
            """the pixel set the last kernels() run left: the compacted counters and the summed far list"""
            far_entries, total, bad = words.cpu().tolist()
            m = int(found.item())
            assert total == reads and bad == 0 and far_entries <= records and m <= room
            keys, sums = pairs.sum_far_list(far_key[:far_entries], far_count[:far_entries])
            fx = torch.div(keys, n, rounding_mode="floor")
            return pixel_set(torch.cat([ox[:m], fx.to(torch.int32)]), torch.cat([od[:m], (keys - fx * n - fx).to(torch.int32)]),
                             torch.cat([oc[:m], sums])), far_entries

        def torch_form():
            X = torch.div(x, k, rounding_mode="floor").to(torch.int64)
            Y = torch.div(x.to(torch.int64) + dist, k, rounding_mode="floor")
            return pairs.sum_far_list(X * n + Y, count)

        coarsen_ms, _ = timed(kernels(lib))
        (want_key, want_count), far_entries = collected()
        row = {"n": n, "dense_diags": K, "pixels": int(want_key.numel()), "far_entries": far_entries,
               "coarsen_ms": round(coarsen_ms, 3), "coarsen_records_per_s": round(records / (coarsen_ms * 1e-3)),
               "coarsen_read_GB_per_s": round(16 * records / (coarsen_ms * 1e-3) / 1e9, 1)}
        if plain is not None:
            plain_ms, _ = timed(kernels(plain))
            (key, cnt), plain_far = collected()
            assert torch.equal(key, want_key) and torch.equal(cnt, want_count)      # both builds: the same pixel set
            row.update(coarsen_plain_ms=round(plain_ms, 3), plain_far_entries=plain_far, plain_over_combined=round(plain_ms / coarsen_ms, 3))
        records_ms, got = timed(lambda: multires.coarsen_records(x, dist, count, k, distance_bins=DISTANCE_BP // (res * k), device=dev))
        key, cnt = pixel_set(*got)
        assert torch.equal(key, want_key) and torch.equal(cnt, want_count)
        torch_ms, (key, cnt) = timed(torch_form)
        assert torch.equal(key, want_key) and torch.equal(cnt, want_count)          # and the sort gives it too
        row.update(records_ms=round(records_ms, 3), torch_ms=round(torch_ms, 3), torch_over_coarsen=round(torch_ms / coarsen_ms, 3),
                   torch_over_records=round(torch_ms / records_ms, 3))
        result["factors"][str(k)] = row
        del dense, far_key, far_count, ox, od, oc, ws
    if args.wall:
        result["wall"] = wall_times(args.wall, args.wall_chromosome)
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
