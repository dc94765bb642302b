"""Normalisation timing below 125 bp: HIP events around mst_normalize_band on synthetic bands.

    python scripts/norm_fine_time.py                 (GPU box; ~50 GB of device memory for the chr1 shape)

Shapes: chr1 at 100 bp (n = 2.49 M, dpx = 2000, window 20 000: the strip form, 40 GB in + 40 GB out), the same band at
125 bp (window 16 000: the LDS-resident <32> form -- the yardstick, measured in the same run) and chr21 at 50 bp (n = 934 k,
window 40 000).  Printed per shape: the median of 5 timed runs after one warm-up, ns per band sample, and the bytes per sample
of each form's traffic model next to the bandwidth that model implies.
  strip form:  8 (block-sum pass reads the band) + 0.625 (writes 20 B per 32 samples) + 8 (strips: every sample once from HBM,
               its second strip and its centre read from cache) + 20 (W + 1024) / 32 / 1024 (the tile's block sums) + 8 (out)
  <32> form:   8 (the memset of the output) + 8 (every sample once from HBM, the W / 1024 re-reads from cache) + 8 (out)
(diag_stats_kernel's read of the band, 8 B per sample, is in both figures and both models.)"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mustache_amd.normalize import normalize_band  # noqa: E402
from mustache_amd.synth import band_counts  # noqa: E402


def make_band(n, dpx, dev):
    raw = torch.empty((dpx + 2, n), dtype=torch.float64, device=dev)
    for i0 in range(0, n, 65536):
        i1 = min(n, i0 + 65536)
        raw[:, i0:i1] = band_counts(n, dpx, 40.0, max(n // 300, 1), 1, i0=i0, i1=i1, device=dev)
    return raw


def time_one(raw, n, dpx, res, kernel=None, reps=5):
    ms = []
    for rep in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out, _, local = normalize_band(raw, n, dpx, res, kernel=kernel)
        e1.record()
        torch.cuda.synchronize()
        assert local
        del out
        if rep:
            ms.append(e0.elapsed_time(e1))
    return sorted(ms)[len(ms) // 2]


def report(tag, ms, samples, model):
    ns = ms * 1e6 / samples
    print("%-34s %8.2f ms  %6.3f ns/sample  model %5.1f B/sample -> %5.2f TB/s" % (tag, ms, ns, model, model / ns / 1e3),
          flush=True)
    return ns


def main():
    dev = torch.device("cuda", 0)
    res_ = {}
    n, dpx = 2488000, 2000
    raw = make_band(n, dpx, dev)
    samples = (dpx + 2) * n
    for res, tag in ((100, "chr1 @ 100 bp, W 20000 (strips)"), (125, "chr1 @ 125 bp, W 16000 (<32>)")):
        W = int(2000000 / res)
        model = 8 + 8 + 0.625 + 8 + 20 * (W + 1024) / 32 / 1024 + 8 if res == 100 else 8 + 8 + 8 + 8
        res_[res] = report(tag, time_one(raw, n, dpx, res), samples, model)
    print("strips (W 20000) / <32> (W 16000) per sample: %.2f" % (res_[100] / res_[125]), flush=True)
    del raw
    torch.cuda.empty_cache()
    n = 934000
    raw = make_band(n, dpx, dev)
    W = 40000
    report("chr21 @ 50 bp, W 40000 (strips)", time_one(raw, n, dpx, 50), (dpx + 2) * n,
           8 + 8 + 0.625 + 8 + 20 * (W + 1024) / 32 / 1024 + 8)


if __name__ == "__main__":
    main()
