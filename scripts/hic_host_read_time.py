#!/usr/bin/env python3
"""Host-only timing of the native `.hic` reader (no GPU): two builds of libmustache_io.so side by side.

    python scripts/hic_host_read_time.py PARENT.so NEW.so [--records 70e6] [--passes 7] [--out profiles/hic_host_read_time.json]

Writes a version 8 file with hic_writer.write_hic_bulk from NumPy-made diagonal blocks, then alternates the two libraries, one
fresh process per pass (a process loads one library), a warm-up pass each first.  A pass times, at 16 threads: decode + fetch
of the packed one-shot read, a full drain of HicStream, and a full drain of HicRawStream, every slab released at once.
Verdict per path: the new median may exceed the parent's by at most the parent's own inter-quartile range in this run.
The file must be large enough to time: a path whose parent median is under 0.2 s fails the run (ask for more --records).
`--one LIB FILE` is the single pass the driver starts (prints one JSON line)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                                                     # noqa: E402

RES, BLOCK_BINS, DPX, THREADS, SLABS = 1000, 1000, 400, 16, 40


def write_file(path, records):
    from hic_writer import write_hic_bulk
    per_block = 250000                                                 # of the ~320 000 cells of a block within DPX of the diagonal
    n_blocks = max(1, -(-int(records) // per_block))

    def blocks():
        rng = np.random.default_rng(1)
        for b in range(n_blocks):
            x = rng.integers(0, BLOCK_BINS, 4 * per_block)
            y = np.minimum(x + rng.integers(0, DPX, 4 * per_block), BLOCK_BINS - 1)
            key = np.unique(y * BLOCK_BINS + x)                            # sorted by (y, x); ~300 000 distinct cells
            assert len(key) >= per_block
            key = np.sort(rng.choice(key, per_block, replace=False))
            c = rng.uniform(0.5, 60.0, len(key)).astype(np.float32)
            yield b, b, key % BLOCK_BINS + b * BLOCK_BINS, key // BLOCK_BINS + b * BLOCK_BINS, c
    return write_hic_bulk(path, "chr1", n_blocks * BLOCK_BINS * RES, RES, blocks(), BLOCK_BINS, threads=THREADS)


def one_pass(lib, path):
    os.environ["MUSTACHE_IO_LIB"] = lib
    from mustache_amd.hicfile import HicFile, HicRawStream, HicStream, read_intra_packed
    out = {}
    with HicFile(path) as h:
        t0 = time.perf_counter()
        pc = read_intra_packed(h, "chr1", RES, "KR", DPX, 0, threads=THREADS)
        out["packed_one_shot_s"] = time.perf_counter() - t0
        cap, raw_bytes = 1 << 19, 1 << 22
        mem = np.zeros(SLABS * max(cap * 10, raw_bytes) + 16, np.uint8)
        ptr = mem.ctypes.data + (-mem.ctypes.data) % 16
        for name, st in (("packed_stream_s", lambda: HicStream(h, "chr1", RES, "KR", DPX, 0, ptr, SLABS, cap, 2, threads=THREADS)),
                         ("raw_stream_s", lambda: HicRawStream(h, "chr1", RES, "KR", DPX, ptr, SLABS, raw_bytes, threads=THREADS))):
            t0 = time.perf_counter()
            s = st()
            while True:
                r = s.next(-1)
                if r is False:
                    break
                s.release(r[0])
            s.close()
            out[name] = time.perf_counter() - t0
        out["records"] = len(pc)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--records", type=float, default=70e6)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hic_host_read_time.json"))
    ap.add_argument("--one", nargs=2, metavar=("LIB", "FILE"))
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one_pass(*a.one)))
        return 0
    parent, new = (os.path.abspath(p) for p in a.libs)
    with tempfile.TemporaryDirectory(prefix="mst_hic_time_") as d:
        path = os.path.join(d, "t.hic")
        n = write_file(path, a.records)
        series = {"parent": [], "new": []}
        for i in range(a.passes + 1):                                      # pass 0 of each library is the warm-up
            for name, lib in (("parent", parent), ("new", new)):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", lib, path], capture_output=True, text=True,
                                   check=True)
                if i:
                    series[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    result = {"records_written": int(n), "threads": THREADS, "passes": a.passes, "series": series, "paths": {}}
    ok = True
    for key in ("packed_one_shot_s", "packed_stream_s", "raw_stream_s"):
        p, q = (np.array([s[key] for s in series[k]]) for k in ("parent", "new"))
        iqr = float(np.percentile(p, 75) - np.percentile(p, 25))
        row = {"parent_median_s": float(np.median(p)), "new_median_s": float(np.median(q)), "parent_iqr_s": iqr,
               "within_margin": bool(np.median(q) <= np.median(p) + iqr), "long_enough": bool(np.median(p) >= 0.2)}
        ok = ok and row["within_margin"] and row["long_enough"]
        result["paths"][key] = row
        print("%-18s parent %.4f s  new %.4f s  parent IQR %.4f s  %s" % (key, row["parent_median_s"], row["new_median_s"], iqr,
                                                                        ("ok" if row["within_margin"] else "SLOWER") + ("" if row["long_enough"] else "  TOO SHORT (< 0.2 s)")))
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
