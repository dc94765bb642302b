"""Branch A of normalize_sparse at resolutions finer than ~125 bp: windows (2 Mb / res) of more than 16 384 bins, beyond what
the LDS-resident kernels hold, go through the strip form of mst_band.hip (local == 4 selects it at any window)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-10, atol=1e-11)


def _band(x, y, v, n, dpx):
    import torch
    from mustache_amd.normalize import band_from_coo
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return band_from_coo(t(x.astype(np.int64)), t(y.astype(np.int64)), t(v.astype(np.float64)), n, dpx)


def test_fine_resolution_fixture_vs_reference(golden_dir):
    """normalize_E.npz: the reference's own normalize_sparse at 100 bp (window 20 000 bins), with windows of fewer than 30
    samples and an empty diagonal."""
    from mustache_amd.mustache import normalize_sparse
    g = np.load(os.path.join(golden_dir, "normalize_E.npz"))
    assert int(g["window"]) == 20000
    v = g["v_in"].astype(np.float64)
    w = normalize_sparse(g["x"].astype(np.int64), g["y"].astype(np.int64), v, int(g["res"]), int(g["dpx"]))
    np.testing.assert_allclose(v, g["v_out"], **TOL)
    np.testing.assert_allclose(np.array(w)[:len(g["weights"])], g["weights"], rtol=1e-12)


def test_50bp_window_vs_oracle():
    import oracle
    from mustache_amd.mustache import normalize_sparse
    from mustache_amd.synth import synth_coo
    n, dpx, res = 42000, 6, 50
    assert int(2000000 / res) == 40000 and (n - dpx) * res > 2000000
    x, y, v = synth_coo(n, dpx, depth=25.0, seed=31)
    exp = v.copy()
    oracle.normalize_sparse(x, y, exp, res, dpx)
    got = v.copy()
    normalize_sparse(x, y, got, res, dpx)
    np.testing.assert_allclose(got, exp, **TOL)
    assert np.count_nonzero(got) > 0.9 * len(got)


def _exact_band(raw, n, dpx, W):
    """normalize_sparse branch A on a [dpx+2, n] host band with window sums and every later step in extended precision
    (longdouble prefix sums over the whole diagonal: exact enough as a yardstick, not a formulation for float64)."""
    L = np.longdouble
    out = np.zeros_like(raw)
    left = W // 2
    for d in range(dpx + 2):
        row = raw[d, :n - d]
        nzm = row != 0
        if not nzm.any():
            continue
        vals = np.where(nzm, row + 0.001, 0.0)
        mean, std = float(np.mean(row[nzm])), float(np.std(row[nzm]))
        m = len(row)
        pc = np.concatenate([[0], np.cumsum(nzm.astype(np.int64))])
        p1 = np.concatenate([[L(0)], np.cumsum(vals.astype(L))])
        p2 = np.concatenate([[L(0)], np.cumsum(vals.astype(L) ** 2)])
        lo = np.clip(np.arange(m) - left, 0, m)
        hi = np.clip(np.arange(m) - left + W, 0, m)
        c = (pc[hi] - pc[lo]).astype(L)
        s1, s2 = p1[hi] - p1[lo], p2[hi] - p2[lo]
        with np.errstate(all="ignore"):
            var = (s2 - s1 * s1 / c) / (c - 1)
            var = np.where(np.isfinite(var), var, L(std) ** 2)
            mu = s1 / c
            mu = np.where(c < 30, L(mean), mu)
            var = np.where(c < 30, L(std) ** 2, var)
            mu = np.where(np.isfinite(mu), mu, L(mean))
            z = (vals.astype(L) - mu) / np.sqrt(var)
            z = np.where(np.isfinite(z), z, L(0))
        z = z * (L(1) + np.log(L(1) + L(mean)) / np.log(L(30)))
        out[d, :m] = np.where(nzm, z, 0).astype(np.float64)
    return out


def test_widest_window_vs_extended_precision():
    """res = 16 bp: window 125 000 bins (np.convolve is too slow there; the yardstick is the extended-precision restatement)."""
    from mustache_amd.normalize import normalize_band
    from mustache_amd.synth import synth_coo
    n, dpx, res = 127000, 4, 16
    W = int(2000000 / res)
    assert W == 125000 and (n - dpx) * res > 2000000
    x, y, v = synth_coo(n, dpx, depth=25.0, seed=32)
    band = _band(x, y, v, n, dpx)
    out, _, local = normalize_band(band, n, dpx, res)
    assert local
    got = out.cpu().numpy()
    exp = _exact_band(band.cpu().numpy(), n, dpx, W)
    np.testing.assert_allclose(got, exp, rtol=1e-10, atol=1e-11)
    assert np.count_nonzero(got) > 0.9 * len(v)


@pytest.mark.parametrize("res", [1000, 250, 125])
def test_strip_form_equals_existing_forms(res):
    """local == 4 (the strip form) at windows the walking / LDS-resident forms serve: 2 000, 8 000 and 16 000 bins."""
    import oracle
    from mustache_amd.normalize import band_to_coo, normalize_band
    from mustache_amd.synth import synth_coo
    n, dpx = 17000, 8
    W = int(2000000 / res)
    assert W in (2000, 8000, 16000) and (n - dpx) * res > 2000000
    x, y, v = synth_coo(n, dpx, depth=25.0, seed=33 + W)
    x, y = x.astype(np.int64), y.astype(np.int64)
    band = _band(x, y, v, n, dpx)
    auto, sa, _ = normalize_band(band, n, dpx, res)
    strips, ss, _ = normalize_band(band, n, dpx, res, kernel="strips")
    assert bool((sa == ss).all())
    a, s = auto.cpu().numpy(), strips.cpu().numpy()
    np.testing.assert_allclose(s, a, **TOL)
    diff = np.abs(s - a)
    print("W = %d: strips vs auto max |diff| %.3g, max relative %.3g" %
          (W, diff.max(), (diff / np.maximum(np.abs(a), 1e-300))[a != 0].max()))
    exp = v.copy()
    oracle.normalize_sparse(x, y, exp, res, dpx)
    import torch
    got = torch.from_numpy(v.copy()).cuda()
    band_to_coo(strips, torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), got, n, dpx)
    np.testing.assert_allclose(got.cpu().numpy(), exp, **TOL)


def test_strip_form_independent_of_n():
    """Appending 3 000 empty bins leaves the first n columns of every diagonal bit-identical.  The per-diagonal mean / std
    pivot on 256 samples spread over the diagonal's length; those positions (for both lengths) hold one integer per diagonal,
    so the global statistics -- computed in a position-fixed order -- are bit-identical as well and what is compared is the
    window sums' independence of the segmentation."""
    import torch
    from mustache_amd.normalize import normalize_band
    n, dpx, res, extra = 21500, 6, 100, 3000
    rng = np.random.default_rng(34)
    raw = np.zeros((dpx + 2, n + extra))
    for d in range(dpx + 2):
        L = n - d
        keep = rng.random(L) < (0.02 if d == 5 else 0.6)          # one sparse diagonal: windows below 30 samples
        raw[d, :L] = np.where(keep, np.round(rng.gamma(2.0, 20.0 / (1 + d), L)) + 1.0, 0.0)
        for LL in (L, L + extra):
            pos = np.arange(256) * LL // 256
            raw[d, pos[pos < L]] = 7.0
    short = torch.from_numpy(np.ascontiguousarray(raw[:, :n])).cuda()
    long_ = torch.from_numpy(raw).cuda()
    for kernel in (None, "strips"):
        o1, s1, _ = normalize_band(short, n, dpx, res, kernel=kernel)
        o2, s2, _ = normalize_band(long_, n + extra, dpx, res, kernel=kernel)
        assert torch.equal(s1, s2)
        assert torch.equal(o1, o2[:, :n].contiguous())
        assert torch.count_nonzero(o2[:, n:]) == 0
        assert torch.count_nonzero(o1) > 0.5 * np.count_nonzero(raw)


def _write_text(path, bpath, x, y, v, res, n, seed):
    rng = np.random.default_rng(seed)
    with open(path, "w") as f:
        for a, b, c in zip(x, y, v):
            f.write("%d\t%d\t%r\n" % (a * res, b * res, float(c)))
    with open(bpath, "w") as f:
        for b in rng.uniform(0.8, 1.25, n + 1):
            f.write("%r\n" % float(b))


def test_cli_at_100bp_equals_oracle_normalisation(tmp_path):
    """`-r 100 -d 20000`: dpx 200, blocks of 2 000 bins, window 20 000 bins.  The CLI's TSV equals call_loops_coo fed with
    the oracle's normalisation of the same reader output; then one diff_mustache run on two such maps."""
    import oracle
    from mustache_amd.diff_mustache import SUFFIX, main as diff_main
    from mustache_amd.mustache import call_loops_coo, main, read_pd
    from mustache_amd.synth import synth_coo
    n, dpx, res = 22000, 200, 100
    paths = []
    for s in (0, 1):
        x, y, v = synth_coo(n, dpx, depth=300.0, seed=35 + s, nloops=400)
        fpath, bpath = str(tmp_path / ("s%d.txt" % s)), str(tmp_path / ("s%d.bias" % s))
        _write_text(fpath, bpath, x, y, np.round(v) + 1.0, res, n, 37 + s)
        paths.append((fpath, bpath))
    fpath, bpath = paths[0]
    out = str(tmp_path / "out.tsv")
    main(["-f", fpath, "-b", bpath, "-ch", "S", "-r", "100", "-pt", "0.1", "-st", "0.8", "-o", out, "-d", str(dpx * res)])
    rows = [l.split("\t") for l in open(out).read().strip().split("\n")[1:]]
    got = sorted((int(r[1]) // res, int(r[4]) // res, float(r[6]), float(r[7])) for r in rows)
    rx, ry, rv = (np.asarray(a) for a in read_pd(fpath, dpx * res, bpath, "S", res))
    rv = rv.astype(np.float64).copy()
    oracle.normalize_sparse(rx, ry, rv, res, dpx)
    exp = sorted((int(a), int(b), q, s) for a, b, q, s in call_loops_coo(rx, ry, rv, res, dpx, [1.6, 3.2], 0.8, 0.1,
                                                                         chromosome="S", verbose=False, normalized=True))
    assert len(exp) > 10
    assert [(a, b, s) for a, b, _, s in got] == [(a, b, s) for a, b, _, s in exp]
    np.testing.assert_allclose([q for _, _, q, _ in got], [q for _, _, q, _ in exp], rtol=1e-6)
    prefix = str(tmp_path / "diff")
    diff_main(["-f1", paths[0][0], "-b1", paths[0][1], "-f2", paths[1][0], "-b2", paths[1][1], "-ch", "S", "-r", "100",
               "-pt", "0.1", "-pt2", "0.1", "-st", "0.8", "-d", str(dpx * res), "-o", prefix])
    for k in (1, 3):
        assert len(open(prefix + SUFFIX[k]).read().strip().split("\n")) > 1, SUFFIX[k]
    for suf in SUFFIX.values():
        assert os.path.exists(prefix + suf)
