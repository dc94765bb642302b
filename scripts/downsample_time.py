#!/usr/bin/env python3
"""The thinning kernel (mustache_amd/downsample.py, csrc/mst_thin.hip) on device-resident synthetic records shaped like chr1
at 5 kb: the read pairs of scripts/pairs_time.py (50 M by default), binned by pairs.bin_pairs_device, thinned at T = 2^31.

  thin        mst_thin_counts of the product library (two modes: a pixel with MST_THIN_HEAVY reads or more is thinned by its wave)
  thin_plain  the same kernel built with MST_THIN_HEAVY above any count (`make -C mustache_amd/csrc thin_plain`): one lane per
              pixel throughout; skipped when that library is not there
  binomial    torch.binomial on the same counts on the same device: a yardstick, not a parity target (another generator)

Each: HIP events around it, 3 warm-ups, the median of 20.  `heavy_share` = the share of the reads that lie in pixels of
MST_THIN_HEAVY reads or more.  One JSON line is printed and written to profiles/downsample_time.json.  Needs the GPU.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

T = 1 << 31


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50000000)
    ap.add_argument("--plain-lib", default=os.path.join(ROOT, "mustache_amd", "libmustache_hip_thin_plain.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "downsample_time.json"))
    args = ap.parse_args()

    import torch
    from pairs_time import DISTANCE_BP, LENGTH, REPS, WARMUP, positions, timed
    from mustache_amd import _lib, downsample, pairs
    from mustache_amd._lib import ptr, stream
    if not torch.cuda.is_available():
        raise SystemExit("downsample_time.py needs the GPU")
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    res = 5000
    p1, p2 = positions(args.rows, 11, dev)
    px = pairs.bin_pairs_device(p1, p2, res, length=LENGTH, distance_bins=DISTANCE_BP // res, device=dev)
    del p1, p2
    x, dist, count = px.x.contiguous(), px.dist.contiguous(), px.count.contiguous()
    reads, pixels = int(count.sum().item()), int(count.numel())
    heavy = count >= downsample.HEAVY
    tag = downsample.chromosome_tag("chr1")
    k = torch.empty_like(count)
    words = torch.zeros(3, dtype=torch.int64, device=dev)

    def thin_with(library):
        def run():
            words.zero_()
            _lib.check(library.mst_thin_counts(ptr(x), ptr(dist), ptr(count), 0, pixels, tag, 0, 0, T, ptr(k), ptr(words), stream()))
        return run

    thin_ms, _ = timed(thin_with(lib))
    kept = k.clone()
    totals = words.cpu().tolist()
    assert totals[0] == reads and totals[1] == int(kept.sum().item()) and totals[2] == 0
    result = {"device": torch.cuda.get_device_name(dev), "rows": args.rows, "res": res, "pixels": pixels, "reads": reads, "T": T,
              "kept": totals[1], "heavy_threshold": downsample.HEAVY, "heavy_pixels": int(heavy.sum().item()),
              "heavy_share": round(int(count[heavy].sum().item()) / reads, 4), "max_count": int(count.max().item()),
              "warmup": WARMUP, "reps": REPS, "thin_ms": round(thin_ms, 3), "thin_reads_per_s": round(reads / (thin_ms * 1e-3))}
    if os.path.exists(args.plain_lib):
        plain = ctypes.CDLL(args.plain_lib)
        plain.mst_thin_counts.restype, plain.mst_thin_counts.argtypes = _lib._SIGNATURES["mst_thin_counts"]
        plain_ms, _ = timed(thin_with(plain))
        assert torch.equal(k, kept) and words.cpu().tolist() == totals          # both builds keep the same reads
        result.update(thin_plain_ms=round(plain_ms, 3), thin_plain_reads_per_s=round(reads / (plain_ms * 1e-3)),
                      two_modes_over_plain=round(plain_ms / thin_ms, 3))
    cf = count.to(torch.float64)
    half = torch.full_like(cf, 0.5)
    binomial_ms, drawn = timed(lambda: torch.binomial(cf, half))
    result.update(binomial_ms=round(binomial_ms, 3), binomial_reads_per_s=round(reads / (binomial_ms * 1e-3)),
                  binomial_kept=int(drawn.sum().item()), binomial_over_thin=round(binomial_ms / thin_ms, 3))
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
