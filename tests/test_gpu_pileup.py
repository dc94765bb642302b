"""The pile-up (APA) on the MI355X (mustache_amd/pileup.py, csrc/mst_pileup.hip) against the NumPy restatement
(tests/pileup_reference.py): valid bins and E, windows, aggregates and metrics, determinism, the reduce's chunk edges, the
window limit, both kinds of command-line input, and planted loops on synthetic maps."""
import math

import numpy as np
import pytest

import pileup_reference as pr

pytestmark = pytest.mark.gpu


def _synth(n, D, seed, masked=()):
    """a raw band [D + 2, n]: decaying counts, a few zeros, every pixel touching a `masked` bin removed"""
    rng = np.random.default_rng(seed)
    B = np.zeros((D + 2, n))
    for d in range(min(D + 2, n)):
        v = rng.poisson(200.0 / (1.0 + d), n - d).astype(np.float64)
        v[rng.random(n - d) < 0.1] = 0.0
        B[d, :n - d] = v
    for m in masked:
        B[:, m] = 0.0
        for d in range(min(D + 2, m + 1)):
            B[d, m - d] = 0.0
    return B


def _dev(B):
    import torch
    return torch.from_numpy(np.ascontiguousarray(B)).cuda()


def _close(a, b, rel=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    ok = both_nan | (np.abs(a - b) <= rel * np.maximum(np.abs(a), np.abs(b)))
    return bool(ok.all())


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


@pytest.mark.parametrize("n,D,seed", [(300, 40, 1), (4000, 120, 2), (9600, 75, 3)])
def test_valid_and_expected(n, D, seed):
    from mustache_amd.pileup import expected
    masked = [0, 7, n // 2, n // 2 + 1, n - 1] + list(range(n - 60, n - 20, 3))
    B = _synth(n, D, seed, masked)
    valid, E = expected(_dev(B), n, D)
    want_v = pr.valid_bins(B, n, D)
    assert not want_v[masked].any() and want_v.sum() > n // 2
    assert np.array_equal(valid.cpu().numpy().astype(bool), want_v)
    want_E = pr.expected(B, n, D, want_v)
    assert _close(E.cpu().numpy(), want_E)


def _loops(n, D_max, w, L, seed):
    """L loops with 0 < y - x <= D_max - 2w, some at both chromosome ends and some with y - x < 2w"""
    rng = np.random.default_rng(seed)
    sep = rng.integers(1, D_max - 2 * w + 1, L)
    sep[: L // 8] = rng.integers(1, 2 * w + 1, L // 8)
    x = rng.integers(0, np.maximum(n - sep, 1))
    if L >= 4:
        x[0], x[1] = 0, n - 1 - sep[1]
        x[2], x[3] = w // 2, n - 1 - sep[3] - w // 2
    return x.astype(np.int64), (x + sep).astype(np.int64)


def _check_against_restatement(B, n, D, xs, ys, w, q, r):
    E = r["expected"].cpu().numpy()
    obs, oe = pr.windows(B, n, D, E, xs, ys, w)          # the device's own E: windows must match bit for bit
    assert np.array_equal(r["obs"].cpu().numpy(), obs, equal_nan=True)
    assert np.array_equal(r["oe"].cpu().numpy(), oe, equal_nan=True)
    so, co, se, ce = pr.aggregate(obs, oe, xs, ys)
    assert np.array_equal(r["count_obs"], co) and np.array_equal(r["count_oe"], ce)
    assert _close(r["sum_obs"], so) and _close(r["sum_oe"], se)
    c, c_oe, p2 = pr.per_loop(obs, oe, w, q)
    assert _same_bits(r["center_obs"], c) and _same_bits(r["center_oe"], c_oe)
    assert _close(r["p2ll"], p2)
    want = pr.metrics(pr.mean_map(so, co), w, q)
    want_oe = pr.metrics(pr.mean_map(se, ce), w, q)
    for k in want:
        assert _close(r["metrics"][k], want[k]), (k, r["metrics"][k], want[k])
        assert _close(r["metrics_oe"][k], want_oe[k]), k


@pytest.mark.parametrize("w,q", [(5, 3), (10, 6), (20, 6)])
def test_windows_aggregates_and_metrics(w, q):
    from mustache_amd.pileup import pileup_band
    n, Dmax = 2500, 160
    xs, ys = _loops(n, Dmax, w, 300, 10 + w)
    D = int((ys - xs).max()) + 2 * w
    B = _synth(n, D, 20 + w, masked=[5, 600, 601])
    r = pileup_band(_dev(B), n, D, xs, ys, w, q)
    assert np.isnan(r["obs"].cpu().numpy()).any()        # the chromosome ends are reached
    _check_against_restatement(B, n, D, xs, ys, w, q, r)
    ref = pr.pileup_band(B, n, D, xs, ys, w, q)          # and E from the restatement itself
    assert _close(r["expected"].cpu().numpy(), ref["expected"])
    for k in ref["metrics"]:
        assert _close(r["metrics"][k], ref["metrics"][k], 1e-11), k


def test_bit_identical_under_permutation_and_repeats():
    from mustache_amd.pileup import pileup_band
    n, w = 3000, 10
    xs, ys = _loops(n, 200, w, 1100, 7)
    D = int((ys - xs).max()) + 2 * w
    band = _dev(_synth(n, D, 8))
    a = pileup_band(band, n, D, xs, ys, w)
    b = pileup_band(band, n, D, xs, ys, w)
    perm = np.random.default_rng(1).permutation(len(xs))
    c = pileup_band(band, n, D, xs[perm], ys[perm], w)
    for k in ("sum_obs", "count_obs", "sum_oe", "count_oe", "apa", "apa_oe"):
        assert _same_bits(a[k], b[k]) and _same_bits(a[k], c[k]), k
    assert _same_bits(a["p2ll"][perm], c["p2ll"])
    assert _same_bits(a["expected"].cpu().numpy(), c["expected"].cpu().numpy())


@pytest.mark.parametrize("L", [0, 1, 511, 512, 513, 1025])
def test_reduce_chunk_edges(L):
    from mustache_amd.pileup import pileup_band
    n, w, q = 1800, 10, 6
    xs, ys = _loops(n, 120, w, L, 100 + L)
    D = int((ys - xs).max()) + 2 * w if L else 2 * w
    B = _synth(n, D, 30)
    r = pileup_band(_dev(B), n, D, xs, ys, w, q)
    if L == 0:
        assert r["obs"] is None and not r["count_obs"].any() and np.isnan(r["apa"]).all()
        return
    _check_against_restatement(B, n, D, xs, ys, w, q, r)


def test_window_limit():
    import torch
    from mustache_amd import _lib
    from mustache_amd.pileup import PileupError, pileup_band, windows
    n, D = 500, 200
    band = _dev(_synth(n, D, 4))
    with pytest.raises(PileupError, match="64"):
        pileup_band(band, n, D, [100], [150], w=65)
    E = torch.ones(D + 1, dtype=torch.float64, device="cuda")
    xd = torch.tensor([100], dtype=torch.int64, device="cuda")
    with pytest.raises(_lib.MstError, match="64"):
        windows(band, n, D, E, xd, xd + 50, 65, 6)
    r = pileup_band(band, n, D, [60], [130], w=64, q=6)      # the limit itself runs
    assert r["obs"].shape == (1, 129, 129) and not np.isnan(r["center_obs"]).any()


# ---- the command line ----------------------------------------------------------------------------------------------------
HEADER = "BIN1_CHR\tBIN1_START\tBIN1_END\tBIN2_CHROMOSOME\tBIN2_START\tBIN2_END\tFDR\tDETECTION_SCALE\n"


def _write_loops(path, chrom, xs, ys, res):
    with open(path, "w") as fh:
        fh.write(HEADER)
        fh.write("".join("%s\t%d\t%d\t%s\t%d\t%d\t0.01\t1.6\n" % (chrom, a * res, (a + 1) * res, chrom, b * res, (b + 1) * res)
                         for a, b in zip(xs, ys)))
    return str(path)


def _band_of(x, y, v, n, D):
    B = np.zeros((D + 2, n))
    d = y - x
    keep = d <= D + 1
    B[d[keep], x[keep]] = v[keep]
    return B


def _read_matrix(path):
    return np.array([[float(v) for v in line.split("\t")] for line in open(path).read().splitlines()])


def _check_cli(out, B, n, xs, ys, w=10, q=6):
    D = int((ys - xs).max()) + 2 * w
    want = pr.pileup_band(B[:D + 1], n, D, xs, ys, w, q)
    assert _close(_read_matrix(out + ".apa.tsv"), want["apa"]) and _close(_read_matrix(out + ".oe.tsv"), want["apa_oe"])
    rows = [r.split("\t") for r in open(out + ".loops.tsv").read().splitlines()[1:]]
    assert [r[8] for r in rows] == ["used"] * len(xs)
    assert _close([float(r[9]) for r in rows], want["center_obs"]) and _close([float(r[11]) for r in rows], want["p2ll"])
    allrow = open(out + ".stats.tsv").read().splitlines()[-1].split("\t")
    assert allrow[:3] == ["all", str(len(xs)), str(len(xs))]
    assert _close(float(allrow[3]), want["metrics"]["P2LL"], 1e-11)


def test_cli_hic(tmp_path):
    from hic_writer import write_hic
    from mustache_amd.pileup import main
    from mustache_amd.synth import synth_coo
    n, dpx, res = 2000, 150, 5000
    x, y, v = synth_coo(n, dpx, depth=300.0, seed=5, nloops=50)
    v = np.maximum(np.round(v), 0.0)
    keep = v > 0
    x, y, v = x[keep].astype(np.int64), y[keep].astype(np.int64), v[keep]
    h = str(tmp_path / "m.hic")
    write_hic(h, [("All", 1000), ("chr1", n * res)], {1: {res: (x, y, v)}}, {}, version=8, block_bin_count=200,
              float_counts=True)
    xs, ys = _loops(n, 140, 10, 200, 3)
    xs, ys = xs[ys - xs >= 30], ys[ys - xs >= 30]
    lp = _write_loops(tmp_path / "l.tsv", "chr1", xs, ys, res)
    out = str(tmp_path / "o")
    main(["-f", h, "-l", lp, "-r", str(res), "-o", out, "-norm", "NONE"])
    _check_cli(out, _band_of(x, y, v, int(y.max()) + 1, int((ys - xs).max()) + 20), int(y.max()) + 1, xs, ys)


def test_cli_text_and_bias(tmp_path):
    from mustache_amd.mustache import read_pd
    from mustache_amd.pileup import main
    from mustache_amd.synth import synth_coo
    n, dpx, res = 1500, 120, 10000
    x, y, v = synth_coo(n, dpx, depth=200.0, seed=9, nloops=40)
    t = str(tmp_path / "m.txt")
    with open(t, "w") as fh:
        fh.write("".join("%d\t%d\t%d\n" % (a * res, b * res, max(1, round(c))) for a, b, c in zip(x, y, v)))
    bf = str(tmp_path / "b.txt")
    with open(bf, "w") as fh:
        fh.write("".join("%r\n" % float(b) for b in np.random.default_rng(2).uniform(0.5, 1.5, n)))
    xs, ys = _loops(n, 110, 10, 150, 4)
    xs, ys = xs[ys - xs >= 30], ys[ys - xs >= 30]
    lp = _write_loops(tmp_path / "l.tsv", "1", xs, ys, res)
    out = str(tmp_path / "o")
    main(["-f", t, "-l", lp, "-r", str(res), "-o", out, "-b", bf])
    D = int((ys - xs).max()) + 20
    rx, ry, rv = read_pd(t, D * res, bf, "1", res)
    rx, ry = np.asarray(rx, np.int64), np.asarray(ry, np.int64)
    nn = int(max(rx.max(), ry.max())) + 1
    _check_cli(out, _band_of(rx, ry, np.asarray(rv), nn, D), nn, xs, ys)


def test_planted_loops_are_enriched():
    import torch
    from mustache_amd.pileup import pileup_band
    from mustache_amd.synth import band_counts, loop_list
    n, dpx, nloops, seed, w = 6000, 200, 150, 17, 10
    band = band_counts(n, dpx, 300.0, nloops, seed, device="cuda").contiguous()
    a, b, _amp, _sig = (t.numpy() for t in loop_list(n, dpx, nloops, seed))
    sel = (b >= 30) & (b + 2 * w <= dpx + 1) & (a + b + 37 + w < n)
    xs, ys = a[sel], a[sel] + b[sel]
    assert len(xs) > 50
    D = int(b[sel].max()) + 2 * w
    planted = pileup_band(band, n, D, xs, ys, w)
    shifted = pileup_band(band, n, D, xs + 37, ys + 37, w)
    assert planted["metrics"]["P2LL"] > shifted["metrics"]["P2LL"]
    assert planted["metrics_oe"]["P2LL"] > max(1.5, shifted["metrics_oe"]["P2LL"])
    assert math.isfinite(shifted["metrics"]["P2LL"])
    torch.cuda.synchronize()


# ---- the reduce, addition by addition ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,L", pr.REDUCE_SINGLE)
def test_reduce_and_reduce_pair_have_the_bytes_of_the_ordered_restatement(w, L):
    """mst_pileup_reduce and mst_pileup_reduce_pair on one segment against pr.ordered_aggregate, byte for byte: values on which
    another order of additions shows (tests/test_pileup_reference.py), independent NaN masks, entries outside 0 .. L-1."""
    from mustache_amd._lib import require_gpu
    from mustache_amd.pileup import _workspace, reduce, reduce_pair
    a, b, order, _off = pr.reduce_case(w, (L,))
    ad, bd, od = _dev(a), _dev(b), _dev(order)
    ws = _workspace(require_gpu(), 1, 0, L, w, ad.device)
    four = reduce(ad, bd, od, w, ws).cpu().numpy()
    three = reduce_pair(ad, bd, od, w, ws).cpu().numpy()
    assert four.tobytes() == pr.ordered_aggregate((a, b), order).tobytes()
    assert three.tobytes() == pr.ordered_aggregate((a, b), order, joint=True).tobytes()


# what the size queries returned before the reduce had one home: (arguments, bytes)
WORKSPACE_CIS = [((1, 0, 0, 0), 768), ((1, 0, 1, 0), 768), ((1, 0, 512, 1), 768), ((1, 0, 513, 10), 28672),
                 ((1, 0, 1025, 64), 1597952), ((300, 40, 512, 1), 1280), ((4097, 3, 20000, 10), 564736),
                 ((248957, 2020, 20000, 10), 1972992), ((0, 0, 1, 1), 0), ((1, 0, 1, 65), 0), ((1, -1, 1, 1), 0), ((1, 0, -1, 1), 0)]
WORKSPACE_TRANS = [((5, 7, 0, 0), 8390656), ((5, 7, 3, 1), 8391680), ((24900, 24300, 2000, 10), 8434432),
                   ((140000, 50, 5, 64), 8409088), ((700, 600, 100000, 64), 104372992), ((0, 1, 1, 1), 0), ((5, 7, 1, 65), 0)]
WORKSPACE_SEGMENTED = [((0, 0), 0, 512), ((0, 3, 3, 603), 1, 1536), ((0, 511, 512, 1024, 1537, 1538), 10, 85248),
                       ((0, 1025), 64, 1598208), ((0, 40, 80, 120), 10, 43008), ((0, 5, 3), 1, 0)]


def test_the_workspace_queries_return_what_they_did():
    from mustache_amd import _lib
    from mustache_amd.pileup import _host_ptr
    lib = _lib.load()
    for args, want in WORKSPACE_CIS:
        assert lib.mst_pileup_workspace_bytes(*args) == want, args
    for args, want in WORKSPACE_TRANS:
        assert lib.mst_pileup_trans_workspace_bytes(*args) == want, args
    for off, w, want in WORKSPACE_SEGMENTED:
        loop_off = np.array(off, np.int64)
        assert lib.mst_pileup_reduce_segmented_workspace_bytes(_host_ptr(loop_off), len(off) - 1, w) == want, (off, w)
