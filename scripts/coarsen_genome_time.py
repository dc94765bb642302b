#!/usr/bin/env python3
"""The many-pairs coarsening kernel (mustache_amd/multires.py, csrc/mst_coarsen_pairs.hip) on the trans records of an
hg19-shaped genome (24 chromosomes, 276 pairs; the layout of scripts/bench_extra.py's thin_pairs_leg): every cell of every trans
matrix at 100 kb a record with probability --density, in cell order as a reader delivers them, counts 1 + Poisson(0.4) as
float64; coarsened to 500 kb (factor 5).

  dense      mst_coarsen_pairs and mst_coarsen_pairs_compact of the product library with every cell a 64-bit counter, the
             zeroing of the counters included
  all_far    dense_cells = 0: every run of a wave is a far entry, then pairs.sum_far_list (one torch sort and a cumulative sum)
  plain      `dense` with the file built with -DMST_COARSEN_PAIRS_PLAIN (`make -C mustache_amd/csrc coarsen_pairs_plain`): one
             atomic per record, no combining of adjacent lanes; skipped when that library is not there
  host       multires.coarsen_pairs end to end for the dense and the all-far form: the above with its allocations, the table
             upload, the host's reads of the words and mst_pairs_trans_decode

Each: HIP events around it, 3 warm-ups, the median of 20 with the least and the most.  The script asserts that all forms give
the same keys and counts.  With `--wall FILE` (a `.pairs[.gz]` file with `#chromsize` lines, or a `.hic` file that stores 100,
200 and 500 kb) it also times `--trans-all --balance-genome NEWTON -r 100kb --coarser-genome 200kb 500kb` on that file (250 kb
is no multiple of 100 kb) against the three plain runs (one run each after a warm-up, wall clock); `--make-pairs FILE --rows N`
writes such a pairs file first.  One JSON line is printed and written to profiles/coarsen_genome_time.json (the kernel times
before the wall runs start, the whole line at the end).  Needs the GPU.
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

RES, FACTOR = 100000, 5
WARMUP, REPS = 3, 20


def timed(fn):
    """((median, least, most) ms of REPS runs after WARMUP, the last result)"""
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
    ms.sort()
    return (round(ms[len(ms) // 2], 4), round(ms[0], 4), round(ms[-1], 4)), out


def make_pairs(path, rows, seed=5):
    """a pairs file of `rows` trans rows on the hg19 table, uniform over the genome"""
    import gzip
    import numpy as np
    from bench_extra import HG19
    names = ["chr%d" % (c + 1) for c in range(22)] + ["chrX", "chrY"]
    rng = np.random.default_rng(seed)
    edges = np.concatenate([[0], np.cumsum(HG19)])
    g1, g2 = rng.integers(0, edges[-1], rows), rng.integers(0, edges[-1], rows)
    c1, c2 = np.searchsorted(edges, g1, side="right") - 1, np.searchsorted(edges, g2, side="right") - 1
    keep = c1 != c2
    c1, c2, p1, p2 = c1[keep], c2[keep], (g1 - edges[c1])[keep] + 1, (g2 - edges[c2])[keep] + 1
    head = "## pairs format v1.0\n" + "".join("#chromsize: %s %d\n" % (n, l) for n, l in zip(names, HG19)) + \
           "#columns: readID chr1 pos1 chr2 pos2 strand1 strand2\n"
    with (gzip.open(path, "wt", compresslevel=1) if path.endswith(".gz") else open(path, "w")) as f:
        f.write(head)
        for s in range(0, len(c1), 1 << 20):
            e = s + (1 << 20)
            f.write("".join("r\t%s\t%d\t%s\t%d\t+\t-\n" % (names[a], p, names[b], q)
                            for a, p, b, q in zip(c1[s:e].tolist(), p1[s:e].tolist(), c2[s:e].tolist(), p2[s:e].tolist())))
    return int(len(c1))


def wall_times(path):
    """one run each of the merged call and the three plain calls, after a warm-up: seconds of wall clock"""
    import contextlib
    import io
    import tempfile
    from mustache_amd import pairs
    from mustache_amd.mustache import main as mustache
    base = ["-f", path, "--trans-all", "--balance-genome", "NEWTON"] + (["--pairs-trans"] if pairs.is_pairs(path) else [])
    jobs = {"warm_up": ["-r", "500kb"], "merged_s": ["-r", "100kb", "--coarser-genome", "200kb", "500kb"],
            "plain_100kb_s": ["-r", "100kb"], "plain_200kb_s": ["-r", "200kb"], "plain_500kb_s": ["-r", "500kb"]}
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name, extra in jobs.items():                             # the first run pays the process's first launches: not kept
            pairs.WANT_TRANS.clear()
            pairs.close_pairs_handles()                              # every run parses the file, as a process of its own would
            t0 = time.perf_counter()
            said = io.StringIO()
            with contextlib.redirect_stdout(said):
                mustache(base + ["-o", os.path.join(d, name + ".tsv")] + extra)
            if not os.path.exists(os.path.join(d, name + ".tsv")):
                raise SystemExit("%s wrote no output:\n%s" % (name, said.getvalue()))
            if name != "warm_up":
                out[name] = round(time.perf_counter() - t0, 3)
                with open(os.path.join(d, name + ".tsv")) as f:
                    out[name.replace("_s", "_loops")] = sum(1 for _ in f) - 1
        pairs.WANT_TRANS.clear()
        pairs.close_pairs_handles()
    out["three_plain_s"] = round(out["plain_100kb_s"] + out["plain_200kb_s"] + out["plain_500kb_s"], 3)
    out["three_plain_minus_merged_s"] = round(out["three_plain_s"] - out["merged_s"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--density", type=float, default=0.05)
    ap.add_argument("--plain-lib", default=os.path.join(ROOT, "mustache_amd", "libmustache_hip_coarsen_pairs_plain.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coarsen_genome_time.json"))
    ap.add_argument("--wall", default=None, metavar="FILE")
    ap.add_argument("--make-pairs", default=None, metavar="FILE.pairs[.gz]")
    ap.add_argument("--rows", type=int, default=5000000)
    args = ap.parse_args()

    import numpy as np
    import torch
    from bench_extra import HG19
    from mustache_amd import _lib, multires, pairs
    from mustache_amd._lib import ptr, stream
    if not torch.cuda.is_available():
        raise SystemExit("coarsen_genome_time.py needs the GPU")
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    fine = [s // RES + 1 for s in HG19]
    bins = [s // (RES * FACTOR) + 1 for s in HG19]
    tables, cells = pairs.trans_tables(HG19, bins)
    P = tables.shape[1]
    gen = torch.Generator(device=dev).manual_seed(1000)
    xs, ys, lens = [], [], []
    for i, j in pairs.pair_list(len(fine)):
        cell = torch.nonzero(torch.rand(fine[i] * fine[j], device=dev, generator=gen) < args.density).flatten()
        xs.append((cell // fine[j]).to(torch.int32))
        ys.append((cell % fine[j]).to(torch.int32))
        lens.append(int(cell.numel()))
    x, y = torch.cat(xs), torch.cat(ys)
    del xs, ys
    N = int(x.numel())
    counts = 1.0 + torch.poisson(torch.full((N,), 0.4, device=dev, dtype=torch.float64), generator=gen)
    reads = int(counts.sum().item())
    seg = np.zeros(P + 1, np.int64)
    np.cumsum(lens, out=seg[1:])
    td = torch.from_numpy(np.concatenate([tables[2], tables[3], tables[4], seg])).to(dev)
    result = {"device": torch.cuda.get_device_name(dev), "res": RES, "factor": FACTOR, "density": args.density, "pairs": P,
              "records": N, "reads": reads, "cells": cells, "warmup": WARMUP, "reps": REPS, "bytes_read_per_record": 16}

    far_key, far_count = (torch.empty(N, dtype=torch.int64, device=dev) for _ in range(2))
    words = torch.zeros(4, dtype=torch.int64, device=dev)
    dense = torch.zeros(cells, dtype=torch.int64, device=dev)
    found = torch.zeros(1, dtype=torch.int64, device=dev)
    room = min(N, cells)
    ok, oc = (torch.empty(room, dtype=torch.int64, device=dev) for _ in range(2))
    ws = torch.empty(int(lib.mst_coarsen_pairs_compact_workspace_bytes(cells)), dtype=torch.uint8, device=dev)

    def launch(library, dense_cells):
        words.zero_()
        _lib.check(library.mst_coarsen_pairs(ptr(x), ptr(y), ptr(counts), 2, N, ptr(td[3 * P:]), ptr(td[:P]), ptr(td[P:2 * P]),
                                             ptr(td[2 * P:3 * P]), P, FACTOR, dense_cells, ptr(dense) if dense_cells else None,
                                             ptr(far_key), ptr(far_count), N, ptr(words), 0, stream()))

    def dense_form(library):
        def run():
            dense.zero_()
            launch(library, cells)
            _lib.check(library.mst_coarsen_pairs_compact(ptr(dense), cells, ptr(ok), ptr(oc), room, ptr(found), ptr(ws), ws.numel(),
                                                         stream()))
        return run

    def dense_result():
        far_entries, total, bad, outside = words.cpu().tolist()
        m = int(found.item())
        assert (far_entries, total, bad, outside) == (0, reads, 0, 0) and m <= room
        return ok[:m].clone(), oc[:m].clone()

    def all_far():
        launch(lib, 0)
        entries = int(words[0].item())                               # the host wait the product pays as well
        return pairs.sum_far_list(far_key[:entries], far_count[:entries]), entries

    t_dense, _ = timed(dense_form(lib))
    want_key, want_count = dense_result()
    result.update(pixels=int(want_key.numel()), dense_ms=t_dense, dense_records_per_s=round(N / (t_dense[0] * 1e-3)),
                  dense_read_GB_per_s=round(16 * N / (t_dense[0] * 1e-3) / 1e9, 1))
    t_far, ((key, cnt), entries) = timed(all_far)
    assert torch.equal(key, want_key) and torch.equal(cnt, want_count)
    result.update(all_far_ms=t_far, far_entries=entries, all_far_over_dense=round(t_far[0] / t_dense[0], 3))
    if os.path.exists(args.plain_lib):
        plain = ctypes.CDLL(args.plain_lib)
        for name in ("mst_coarsen_pairs", "mst_coarsen_pairs_compact_workspace_bytes", "mst_coarsen_pairs_compact"):
            getattr(plain, name).restype, getattr(plain, name).argtypes = _lib._SIGNATURES[name]
        t_plain, _ = timed(dense_form(plain))
        key, cnt = dense_result()
        assert torch.equal(key, want_key) and torch.equal(cnt, want_count)          # both builds: the same pixel set
        result.update(plain_ms=t_plain, plain_over_combined=round(t_plain[0] / t_dense[0], 3))
    for name, dense_cells in (("host_dense_ms", cells), ("host_all_far_ms", 0)):
        t_host, got = timed(lambda: multires.coarsen_pairs(x, y, counts, seg, tables, FACTOR, dense_cells=dense_cells, device=dev))
        assert sum(int(v.numel()) for _, _, v in got.values()) == int(want_key.numel())
        result[name] = t_host
    del dense, far_key, far_count, ok, oc, ws
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result) + "\n")
    if args.make_pairs:
        result["pairs_file_rows"] = make_pairs(args.make_pairs, args.rows)
    if args.wall or args.make_pairs:
        result["wall"] = wall_times(args.wall or args.make_pairs)
    line = json.dumps(result)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
