#!/usr/bin/env python3
"""Time the single-pair trans entry points, trans.call_trans_coo and diff_trans.call_diff_trans_coo, on one tree:

  one sample    short_long_2x2 and dense_2x2 of tests/trans_reference.py (2 x 2 tiles of 2000) and a 180 x 140 single tile
  two samples   production_2x2 of tests/diff_trans_reference.py (2 x 2 tile pairs of 2000) and a 180 x 140 single tile pair

each from device tensors (x, y int32: what the `.hic` reader hands over) and from host arrays (what `.cool` does).  Host clock
around a synchronised call, `--warmup` calls, then `--reps` timed ones per case.  Prints one JSON line: per case the median,
the fastest, the slowest and the number of rows.

Only names every tree since the trans callers has are used, so two trees are compared by running this file once per tree in a
fresh process each: `--root DIR` names the checkout whose mustache_amd is imported (default: this one), `--merge A B OUT`
writes both runs' lines and, per case, whether the second median lies within the first's spread (max - min) of its median.

    python scripts/trans_pair_time.py [--root DIR] [--label NAME] [--reps 7] [--warmup 2] > new.json
    python scripts/trans_pair_time.py --merge parent.json new.json profiles/trans_pair_time.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST, PT, PT2 = 0.88, 0.2, 0.1


def merge(parent_path, new_path, out_path):
    parent, new = (json.loads(open(p).read().strip().splitlines()[-1]) for p in (parent_path, new_path))
    table = {}
    for name, p in parent["cases"].items():
        n = new["cases"][name]
        spread = p["max_s"] - p["min_s"]
        table[name] = {"parent_median_s": p["median_s"], "parent_spread_s": spread, "new_median_s": n["median_s"],
                       "new_minus_parent_s": n["median_s"] - p["median_s"], "inside": n["median_s"] <= p["median_s"] + spread,
                       "rows_equal": p["rows"] == n["rows"]}
    with open(out_path, "w") as fh:
        json.dump({"parent": parent, "new": new, "table": table}, fh, indent=1)
        fh.write("\n")
    print(json.dumps(table))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--label", default="this tree", help="what the JSON line calls the tree")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--merge", nargs=3, metavar=("PARENT", "NEW", "OUT"))
    a = ap.parse_args()
    if a.merge:
        return merge(*a.merge)
    sys.path[:0] = [os.path.abspath(a.root), os.path.join(ROOT, "tests"), ROOT]    # the tests' maps need this tree's oracle/
    import torch
    import diff_trans_reference as dr
    import trans_reference as tr
    from mustache_amd.diff_trans import call_diff_trans_coo
    from mustache_amd.trans import call_trans_coo
    if not torch.cuda.is_available():
        raise SystemExit("trans_pair_time.py needs the GPU")

    def on_device(rec):
        return (torch.as_tensor(rec[0]).to("cuda", dtype=torch.int32), torch.as_tensor(rec[1]).to("cuda", dtype=torch.int32),
                torch.as_tensor(rec[2]).to("cuda"))

    one = {name: (tr.production_records(name), tr.PRODUCTION_CASES[name]["oct"]) for name in ("short_long_2x2", "dense_2x2")}
    one["tile_180x140"] = (tr.synth_trans(180, 140, density=0.6, nloops=6, seed=41), [1.6, 3.2])
    two = {"production_2x2": (dr.case_records("production_2x2"), dr.CASES["production_2x2"]["oct"]),
           "tile_pair_180x140": (dr.synth_pair(180, 140, density=0.6, nloops=8, seed=44, added=3), [1.6, 3.2])}
    calls = {}
    for name, (rec, oct) in one.items():
        for where, r in (("device", on_device(rec)), ("host", rec)):
            calls["one/%s/%s" % (name, where)] = lambda r=r, oct=oct: call_trans_coo(r[0], r[1], r[2], oct, ST, PT)
    for name, ((rec1, rec2), oct) in two.items():
        for where, r1, r2 in (("device", on_device(rec1), on_device(rec2)), ("host", rec1, rec2)):
            calls["two/%s/%s" % (name, where)] = lambda r1=r1, r2=r2, oct=oct: call_diff_trans_coo(r1, r2, oct, ST, PT, PT2)
    cases = {}
    for name, call in calls.items():
        times, rows = [], None
        for i in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = call()
            torch.cuda.synchronize()
            if i >= a.warmup:
                times.append(time.perf_counter() - t0)
        cases[name] = {"median_s": sorted(times)[len(times) // 2], "min_s": min(times), "max_s": max(times), "all_s": times,
                       "rows": len(rows)}
    print(json.dumps({"tree": a.label, "reps": a.reps, "warmup": a.warmup,
                      "device": torch.cuda.get_device_name(0), "cases": cases}))


if __name__ == "__main__":
    main()
