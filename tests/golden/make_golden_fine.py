#!/usr/bin/env python3
"""Generate normalize_E.npz by RUNNING THE REFERENCE (dev container only): branch A of normalize_sparse at a resolution
finer than the LDS-resident kernels serve.

    python -B tests/golden/make_golden_fine.py

res = 100 bp -> window int(2e6 / 100) = 20 000 bins, beyond the 16 384 bins the LDS-resident forms hold, so the
fixture pins the strip kernel (mst_band.hip, local == 4) on the reference's own output.  A synthetic chromosome with
n = 21 500 and dpx = 6 ((n - dpx) * res > 2e6: branch A), integer counts, a thinned stretch from bin 9 000 on where window
counts fall below 30, and one empty diagonal.  Layout as normalize_A..D; only data is stored.  The reference's np.convolve
is O(n * window) per diagonal: a few seconds here.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from _refimport import load_reference  # noqa: E402
from mustache_amd.synth import synth_coo  # noqa: E402


def make_normalize_fine(ref):
    name, n, dpx, res, seed = "normalize_E.npz", 21500, 6, 100, 15
    W = int(2000000 / res)
    x, y, v = synth_coo(n, dpx, depth=60.0, seed=seed)
    d = y - x
    v = np.round(v) + 1.0
    keep = np.ones(len(v), bool)
    keep &= ~((x >= 9000) & ((x + 7 * d) % 503 != 0))          # 0.2 % kept from bin 9000 on: windows there hold < 30 samples
    keep &= d != 3                                                                      # one empty diagonal
    x, y, v = x[keep], y[keep], v[keep].copy()
    few = 0
    for dd in range(dpx + 2):
        row = np.zeros(n - dd)
        row[x[d[keep] == dd]] = 1.0
        c = np.convolve(row, np.ones(W), mode="same")
        few += int(np.count_nonzero((c < 30) & (row != 0)))
    assert few > 0
    vin = v.copy()
    w = ref.normalize_sparse(x, y, v, res, dpx)
    assert (n - dpx) * res > 2000000 and len(w) > 0 and W == 20000
    np.savez_compressed(os.path.join(HERE, name), x=x.astype(np.int32), y=y.astype(np.int32), v_in=vin.astype(np.uint16),
                        v_out=v, weights=np.array(w), res=res, dpx=dpx, window=W)
    assert np.array_equal(vin, vin.astype(np.uint16))
    print(name, len(v), "records, window", W, ";", few, "of them in windows of < 30 samples")


if __name__ == "__main__":
    make_normalize_fine(load_reference("mustache"))
