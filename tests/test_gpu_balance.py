"""ICE balancing on the MI355X (mustache_amd/balance.py, csrc/mst_balance.hip) against the NumPy restatement
(tests/balance_reference.py), its determinism, its edge cases, and `--balance ICE` through both command lines."""
import os

import numpy as np
import pytest

import balance_reference as br

pytestmark = pytest.mark.gpu

CASES = [(300, 11, 0), (1200, 12, 2), (2000, 13, 3), (4000, 14, 2), (9600, 15, 2)]   # 9600 bins: chr21 at 5 kb


def _ice(*a, **k):
    from mustache_amd.balance import ice
    return ice(*a, **k)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


@pytest.mark.parametrize("n,seed,ig", CASES)
def test_device_matches_restatement(n, seed, ig):
    x, y, v = br.synth_full_map(n, seed)
    trace = []
    want, winfo = br.ice(x, y, v, n, ignore_diags=ig, trace=trace)
    # precondition: no decision of the restatement lies within 1e-6 (relative) of its threshold
    _, m, cut = br.filter_mask(*br.kept_pixels(x, y, v, n, ig), n, details=True)
    assert np.min(np.abs(m[m > 0] / cut - 1.0)) > 1e-6
    assert np.min(np.abs(np.array(trace) / 1e-5 - 1.0)) > 1e-6
    got, info = _ice(x, y, v, n, ignore_diags=ig)
    assert np.array_equal(info["masked"], winfo["masked"])
    assert 0 < int(info["masked"].sum()) < n
    assert info["iterations"] == winfo["iterations"] and info["converged"] == winfo["converged"]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.max(np.abs(got[ok] / want[ok] - 1.0)) <= 1e-10
    assert abs(info["variance"] / winfo["variance"] - 1.0) < 1e-6
    assert abs(info["kappa"] / winfo["kappa"] - 1.0) <= 1e-10


HUB_LENGTHS = [1023, 1024, 1025, 2048, 2049, 3000]          # CSR rows of 1, 1, 2, 2, 3 and 3 chunks of 1024 entries


def _check_against_restatement(x, y, v, n, ig):
    trace = []
    want, winfo = br.ice(x, y, v, n, ignore_diags=ig, trace=trace)
    # precondition: no decision of the restatement lies within 1e-6 (relative) of its threshold
    _, m, cut = br.filter_mask(*br.kept_pixels(x, y, v, n, ig), n, details=True)
    assert np.min(np.abs(m[m > 0] / cut - 1.0)) > 1e-6
    assert np.min(np.abs(np.array(trace) / 1e-5 - 1.0)) > 1e-6
    got, info = _ice(x, y, v, n, ignore_diags=ig)
    assert np.array_equal(info["masked"], winfo["masked"])
    assert info["iterations"] == winfo["iterations"] and info["converged"] == winfo["converged"]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.max(np.abs(got[ok] / want[ok] - 1.0)) <= 1e-10
    assert abs(info["kappa"] / winfo["kappa"] - 1.0) <= 1e-10
    return got, info


@pytest.mark.parametrize("ig", [0, 3])
def test_rows_of_several_chunks_match_restatement(ig):
    """Hub rows of 1023 .. 3000 entries: chunk starts past a row's first chunk, and the in-order sum of several chunk
    partials per row, in the iteration (marginals) and in kappa (upper-triangle sums)."""
    import torch
    from mustache_amd.balance import CHUNK, BalanceCSR
    n = 4000
    x, y, v, hubs = br.add_hubs(*br.synth_full_map(n, 51 + ig), n, HUB_LENGTHS, seed=52 + ig)
    csr = BalanceCSR(x, y, v, n, ignore_diags=ig)
    lengths = (csr.row_ptr[1:] - csr.row_ptr[:-1]).cpu().numpy()
    chunks = (csr.chunk_ptr[1:] - csr.chunk_ptr[:-1]).cpu().numpy()
    assert lengths[hubs].tolist() == HUB_LENGTHS
    assert chunks[hubs].tolist() == [1, 1, 2, 2, 3, 3] and CHUNK == 1024
    del csr
    torch.cuda.synchronize()
    got, info = _check_against_restatement(x, y, v, n, ig)
    assert not info["masked"][hubs].any()
    # a hub row's marginal: the device's filter-stage sum against the restatement's, over all chunks of the row
    i, j, vv = br.kept_pixels(x, y, v, n, ig)
    _, m_ref, _ = br.filter_mask(i, j, vv, n, details=True)
    csr = BalanceCSR(x, y, v, n, ignore_diags=ig)
    w = torch.ones(n, dtype=torch.float64, device=csr.device)
    m1, nnz = csr.marginals(w, with_nnz=True)
    assert nnz.cpu().numpy()[hubs].tolist() == HUB_LENGTHS
    w = (nnz >= 10).to(torch.float64)
    m2 = csr.marginals(w)[0].cpu().numpy()
    assert np.max(np.abs(m2[hubs] / m_ref[hubs] - 1.0)) <= 1e-12


def test_rows_of_several_chunks_bit_identical():
    n = 4000
    x, y, v, _ = br.add_hubs(*br.synth_full_map(n, 61), n, HUB_LENGTHS, seed=62)
    b0, i0 = _ice(x, y, v, n)
    assert _same_bits(b0, _ice(x, y, v, n)[0])
    rng = np.random.default_rng(9)
    p = rng.permutation(len(v))
    flip = rng.random(len(v)) < 0.5
    assert _same_bits(b0, _ice(np.where(flip, y, x)[p], np.where(flip, x, y)[p], v[p], n)[0])
    b3, i3 = _ice(x, y, v, n + 1500)
    assert _same_bits(b0, b3[:n]) and np.isnan(b3[n:]).all() and i3["iterations"] == i0["iterations"]


def test_no_nonzero_marginal_stops_with_zero_variance():
    """w non-zero only on an empty row: no s is non-zero, r = 1, the variance is 0 -- the device and the restatement agree."""
    import torch
    from mustache_amd.balance import BalanceCSR
    n = 500
    x, y, v = br.synth_full_map(n, 71)
    i, j, vv = br.kept_pixels(x, y, v, n, 2)
    empty = int(np.setdiff1d(np.arange(n), np.concatenate([i, j]))[0])
    w0 = np.zeros(n)
    w0[empty] = 2.5
    rows, cols, vals = br._sym(i, j, vv)
    w_ref, it, var, conv = br.iterate(rows, cols, vals, w0.copy(), n)
    csr = BalanceCSR(x, y, v, n)
    w = torch.from_numpy(w0.copy()).to(csr.device)
    got = csr.iterate(w, 200, 1e-5)
    assert (it, var, conv) == (1, 0.0, True) and got == (1, 0.0, True)
    assert _same_bits(w.cpu().numpy(), w_ref)


def test_bit_identical_under_repeat_permutation_padding_and_duplicates():
    n = 2500
    x, y, v = br.synth_full_map(n, 21)
    b0, i0 = _ice(x, y, v, n)
    b1, _ = _ice(x, y, v, n)
    assert _same_bits(b0, b1)
    rng = np.random.default_rng(5)
    p = rng.permutation(len(v))
    flip = rng.random(len(v)) < 0.5
    xp, yp = np.where(flip, y, x)[p], np.where(flip, x, y)[p]
    b2, _ = _ice(xp, yp, v[p], n)
    assert _same_bits(b0, b2)
    b3, i3 = _ice(x, y, v, n + 777)                 # appended empty bins
    assert _same_bits(b0, b3[:n]) and np.isnan(b3[n:]).all() and i3["iterations"] == i0["iterations"]
    dup = rng.choice(len(v), 3000, replace=False)   # repeated pixels, the stale entry first: the last entry wins
    xd = np.concatenate([y[dup], x])
    yd = np.concatenate([x[dup], y])
    vd = np.concatenate([v[dup] * 3.0 + 1.0, v])
    b4, _ = _ice(xd, yd, vd, n)
    assert _same_bits(b0, b4)
    # and from device tensors
    import torch
    b5, _ = _ice(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(v).cuda(), n)
    assert _same_bits(b0, b5)


def test_edge_cases(capsys):
    from mustache_amd.balance import report
    n = 600
    x, y, v = br.synth_full_map(n, 31)
    b, info = _ice(x, y, v, n, min_nnz=10 ** 6)    # every bin masked
    assert np.isnan(b).all() and info["masked"].all() and info["iterations"] == 0
    b, info = _ice(x, y, v, n, max_iter=1)
    assert info["iterations"] == 1 and not info["converged"]
    want, winfo = br.ice(x, y, v, n, max_iter=1)
    ok = ~np.isnan(want)
    assert np.max(np.abs(b[ok] / want[ok] - 1.0)) <= 1e-12
    report(info, "chromosome 1")
    assert "did not converge in 1 iterations" in capsys.readouterr().out


def _maps(n, dpx, seed, nloops):
    """a raw text-like map: synthetic counts near the diagonal with loops, plus sparse long-range pixels"""
    from mustache_amd.synth import synth_coo
    x, y, v = synth_coo(n, dpx, depth=300.0, seed=seed, nloops=nloops)
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n, 4000), rng.integers(0, n, 4000)
    far = np.abs(a - b) > dpx + 5
    x = np.concatenate([x, np.minimum(a, b)[far]])
    y = np.concatenate([y, np.maximum(a, b)[far]])
    v = np.concatenate([np.maximum(np.round(v), 1.0), rng.integers(1, 4, int(far.sum())).astype(np.float64)])
    return x, y, v                                  # integer counts: a .hic stores them exactly


def _write_text(path, x, y, v, res):
    with open(path, "w") as f:
        f.write("".join("%d\t%d\t%r\n" % (a * res, b * res, float(c)) for a, b, c in zip(x, y, v)))


@pytest.mark.parametrize("res,n,dpx,dist", [(5000, 3000, 200, "1000000"), (100, 22000, 200, "20000")])
def test_cli_balance_equals_written_bias(tmp_path, res, n, dpx, dist):
    from mustache_amd.balance import balance_text, write_bias
    from mustache_amd.mustache import main
    x, y, v = _maps(n, dpx, 40 + res % 7, n // 40)
    t = str(tmp_path / "map.txt")
    _write_text(t, x, y, v, res)
    o1, o2, bf = str(tmp_path / "bal.tsv"), str(tmp_path / "b.tsv"), str(tmp_path / "bias.tsv")
    main(["-f", t, "-r", str(res), "-d", dist, "-ch", "1", "-o", o1, "--balance", "ICE"])
    bias, info = balance_text(x * float(res), y * float(res), v, res)
    write_bias(bf, "1", res, bias)
    main(["-f", t, "-r", str(res), "-d", dist, "-ch", "1", "-o", o2, "-b", bf])
    a, b = open(o1).read(), open(o2).read()
    assert a == b
    assert a.count("\n") > 5                        # loops were called


def test_no_records_takes_the_no_contact_path(tmp_path, capsys):
    from mustache_amd.mustache import main
    t = str(tmp_path / "m5.txt")
    with open(t, "w") as f:
        f.write("chr1\t0\tchr1\t5000\t3\nchr1\t5000\tchr1\t10000\t4\n")
    out = str(tmp_path / "o.tsv")
    main(["-f", t, "-r", "5000", "-ch", "chr2", "-o", out, "--balance", "ICE"])
    assert "Could't read any interaction" in capsys.readouterr().out
    assert open(out).read().count("\n") == 1        # header only


def _hic(path, x, y, v, n, res):
    from hic_writer import write_hic
    write_hic(path, [("All", 1000), ("chr1", n * res)], {1: {res: (x, y, v)}}, {}, version=8, block_bin_count=200,
              float_counts=True)


def test_hic_route(tmp_path, capsys):
    import torch
    from mustache_amd.balance import balance_text
    from mustache_amd.hicfile import HicFile, read_intra_packed
    from mustache_amd.mustache import call_loops_coo, main, regulator
    n, dpx, res = 3000, 200, 5000
    x, y, v = _maps(n, dpx, 61, 80)
    h = str(tmp_path / "m.hic")
    _hic(h, x, y, v, n, res)
    bt, it = balance_text(x * float(res), y * float(res), v, res)
    with HicFile(h) as hf:
        pc = read_intra_packed(hf, "chr1", res, "NONE", -1, n * res)
    hx, hd, hv = pc.coo()
    assert len(hv) == len(v)
    bh, ih = _ice(hx, hd, hv, int(hd.max()) + 1)
    m = min(len(bt), len(bh))
    assert _same_bits(bt[:m], bh[:m]) and ih["iterations"] == it["iterations"]
    # the records the route hands on: (v / b[x]) / b[y], +inf for NaN / < 0.2, the reader's own distance rule, v' > 0
    os.environ["MUSTACHE_HIC_BACKEND"] = "native"
    try:
        def f(k):
            return bh[k] if (not np.isnan(bh[k]) and bh[k] >= 0.2) else np.inf
        keep = (hd - hx) <= 1000000 // res
        ex, ey, ev = hx[keep], hd[keep], hv[keep]
        ev = (ev / np.array([f(k) for k in ex])) / np.array([f(k) for k in ey])
        pos = ev > 0
        want = call_loops_coo(ex[pos], ey[pos], ev[pos], res, 200, [1.6, 3.2], 0.88, 0.2, verbose=False)
        got = regulator(h, False, False, None, res=res, distance_filter=1000000, chromosome="chr1", balance="ICE",
                        pt=0.2, st=0.88, verbose=False)
        assert len(want) > 5
        os.environ["MUSTACHE_HIC_BACKEND"] = "hicstraw"   # --balance reads raw counts natively whichever backend is set
        again = regulator(h, False, False, None, res=res, distance_filter=1000000, chromosome="chr1", balance="ICE",
                          pt=0.2, st=0.88, verbose=False)
        os.environ["MUSTACHE_HIC_BACKEND"] = "native"
        assert [list(map(float, r)) for r in again] == [list(map(float, r)) for r in got]
        assert [[int(a), int(b)] for a, b, _, _ in got] == [[int(a), int(b)] for a, b, _, _ in want]
        assert all(g[2] == w[2] and g[3] == w[3] for g, w in zip(got, want))
        out = str(tmp_path / "h.tsv")
        main(["-f", h, "-r", str(res), "-d", "1000000", "-ch", "chr1", "-o", out, "--balance", "ICE"])
        assert open(out).read().count("\n") == len(want) + 1
        capsys.readouterr()
        main(["-f", h, "-r", str(res), "-ch", "chr1", "-o", str(tmp_path / "k.tsv"), "-norm", "KR", "--balance", "ICE"])
        assert "-norm KR" in capsys.readouterr().out and not os.path.exists(str(tmp_path / "k.tsv"))
    finally:
        del os.environ["MUSTACHE_HIC_BACKEND"]
    torch.cuda.synchronize()


def test_diff_mustache_balance(tmp_path):
    """`--balance ICE` balances each sample on its own.  The command line applies no -b1 vector (the reference's quirk,
    kept), so the four files are compared with regulator() given both written vectors (bias1=, bias2=)."""
    from mustache_amd.balance import balance_text, write_bias
    from mustache_amd.diff_mustache import HEADER, SUFFIX, main, regulator
    from mustache_amd.mustache import _scalar_text
    n, dpx, res = 3000, 200, 5000
    paths, biases = [], []
    for s in (0, 1):
        x, y, v = _maps(n, dpx, 70 + s, 80)
        t = str(tmp_path / ("s%d.txt" % s))
        _write_text(t, x, y, v, res)
        b, _ = balance_text(x * float(res), y * float(res), v, res)
        bf = str(tmp_path / ("b%d.tsv" % s))
        write_bias(bf, "1", res, b)
        paths.append(t)
        biases.append(bf)
    out = str(tmp_path / "d")
    main(["-f1", paths[0], "-f2", paths[1], "-r", str(res), "-d", "1000000", "-ch", "1", "-o", out, "--balance", "ICE"])
    rows = regulator(paths[0], paths[1], False, False, None, res=res, distance_filter=1000000, bias1=biases[0],
                     bias2=biases[1], chromosome="1", pt=0.2, pt2=0.1, st=0.88, verbose=False)   # the CLI's defaults
    assert len(rows) > 5
    for tag, suf in SUFFIX.items():
        want = HEADER + "".join("1\t%d\t%d\t1\t%d\t%d\t%s\t%s\n" % (int(r[0]) * res, (int(r[0]) + 1) * res, int(r[1]) * res,
                                                                    (int(r[1]) + 1) * res, _scalar_text(r[2]), _scalar_text(r[3]))
                                for r in rows if r[4] == tag)
        assert open(out + suf).read() == want, suf
