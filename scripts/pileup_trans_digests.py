"""SHA-256 digests of pileup.pileup_trans_records on fixed single-pair cases, one per case and per output.
tests/golden/pileup_trans_pair_digests.json is this script's output from the commit BEFORE the single-pair kernels
(mst_pileup_trans.hip) were removed: the bits of the removed kernels, which tests/test_gpu_pileup_trans_digests.py holds the
batch of one to.  Never regenerate the fixture from later code -- a difference is a finding.

Cases (cases(), drawn with np.random.default_rng): v = exp(normal(0, 0.5)), loops on the four corners of the map, (0, 0) twice
and the middle, plus random ones.  The smallest map at w = 0 and w = 1; repeated pixels; the record chunk of 4 096 plus one
record; 1 100 loops (the reduce's 512-loop chunks); the row bits on both sides of the LDS switch (131 072 rows); the default
window; N = 0; L = 0; one +inf.
Outputs: "valid_rows", "valid_cols", "expected" (float64 bytes), "obs", "oe" and KEYS; a case with w > 2 runs once more with
peak = 2 and adds "enrich_sums".
python scripts/pileup_trans_digests.py > digests.json"""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KEYS = ("sum_obs", "count_obs", "sum_oe", "count_oe", "apa", "apa_oe", "center_obs", "center_oe", "p2ll")
PEAK = 2


def _edge_loops(n1, n2, L, rng, also=()):
    """L loops: the four corners, (0, 0) again, the middle, `also`, the rest random"""
    fixed = [(0, 0), (n1 - 1, n2 - 1), (0, n2 - 1), (n1 - 1, 0), (0, 0), (n1 // 2, n2 // 2)] + list(also)
    extra = L - len(fixed)
    xs = np.concatenate([[f[0] for f in fixed], rng.integers(0, n1, extra)]).astype(np.int64)
    ys = np.concatenate([[f[1] for f in fixed], rng.integers(0, n2, extra)]).astype(np.int64)
    return xs, ys


def _dense(n1, n2, N, rng):
    """N records anywhere on the map, drawn with replacement"""
    x, y = rng.integers(0, n1, N).astype(np.int32), rng.integers(0, n2, N).astype(np.int32)
    return x, y, np.exp(rng.normal(0.0, 0.5, N))


def _sparse(n1, n2, xs, ys, rng):
    """30 records near each loop and 100 anywhere, for a map too large to fill"""
    near = np.repeat(np.arange(len(xs)), 30)
    x = np.clip(xs[near] + rng.integers(-3, 4, near.size), 0, n1 - 1)
    y = np.clip(ys[near] + rng.integers(-3, 4, near.size), 0, n2 - 1)
    x, y = np.concatenate([x, rng.integers(0, n1, 100)]), np.concatenate([y, rng.integers(0, n2, 100)])
    return x.astype(np.int32), y.astype(np.int32), np.exp(rng.normal(0.0, 0.5, x.size))


def cases():
    """[(name, x, y, v, n1, n2, xs, ys, w, q)] in a fixed order"""
    out = []

    def dense(name, seed, n1, n2, N, L, w, q):
        rng = np.random.default_rng(seed)
        xs, ys = _edge_loops(n1, n2, L, rng)
        out.append((name,) + _dense(n1, n2, N, rng) + (n1, n2, xs, ys, w, q))

    def sparse(name, seed, n1, n2, L, w, q, also):
        rng = np.random.default_rng(seed)
        xs, ys = _edge_loops(n1, n2, L, rng, also)
        out.append((name,) + _sparse(n1, n2, xs, ys, rng) + (n1, n2, xs, ys, w, q))
    dense("smallest_w0", 101, 5, 7, 40, 11, 0, 1)
    dense("smallest_w1", 102, 5, 7, 40, 11, 1, 1)
    dense("repeated_pixels", 103, 60, 45, 900, 26, 3, 2)
    dense("record_chunk_plus_one", 104, 60, 45, 4097, 26, 3, 7)
    dense("reduce_chunks", 105, 30, 20, 300, 1100, 1, 2)
    sparse("row_bits_global", 106, 140000, 50, 40, 2, 2, [(131070, 25), (131075, 28)])
    sparse("row_bits_lds", 107, 131072, 50, 40, 2, 2, [(131070, 25), (65536, 20)])
    dense("default_window", 108, 300, 180, 5000, 50, 10, 6)
    none = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    out.append(("no_record",) + none + (50, 40, np.array([0, 49], np.int64), np.array([0, 39], np.int64), 2, 2))
    dense("no_loop", 109, 300, 180, 5000, 6, 10, 6)
    out[-1] = out[-1][:6] + (np.zeros(0, np.int64), np.zeros(0, np.int64)) + out[-1][8:]
    dense("one_infinite", 110, 60, 45, 900, 26, 3, 2)
    out[-1][3][17] = np.inf
    return out


def _sha(a, dtype):
    return hashlib.sha256(np.ascontiguousarray(a, dtype).tobytes()).hexdigest()


def digests(case):
    """{output: SHA-256} of one case through pileup.pileup_trans_records"""
    from mustache_amd.pileup import pileup_trans_records
    _, x, y, v, n1, n2, xs, ys, w, q = case
    r = pileup_trans_records(x, y, v, n1, n2, xs, ys, w, q)
    d = {"valid_rows": _sha(r["valid"][0].cpu().numpy(), np.uint8), "valid_cols": _sha(r["valid"][1].cpu().numpy(), np.uint8),
         "expected": _sha(np.float64(r["expected"]), np.float64), "obs": _sha(r["obs"].cpu().numpy(), np.float64),
         "oe": _sha(r["oe"].cpu().numpy(), np.float64)}
    d.update({k: _sha(r[k], np.float64) for k in KEYS})
    if w > PEAK:
        d["enrich_sums"] = _sha(pileup_trans_records(x, y, v, n1, n2, xs, ys, w, q, peak=PEAK)["enrich_sums"], np.float64)
    return d


def main():
    print(json.dumps({c[0]: digests(c) for c in cases()}, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
