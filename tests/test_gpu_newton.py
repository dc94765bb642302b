"""Newton balancing on the MI355X (mustache_amd/balance.py newton(), csrc/mst_balance.hip) against the NumPy restatement
(tests/newton_reference.py), the balancing condition itself, device ICE run to its fixed point, its determinism, its edge
cases, and `--balance NEWTON` through the three command lines."""
import functools

import numpy as np
import pytest

import balance_reference as br
import newton_reference as nr

pytestmark = pytest.mark.gpu

CASES = [(600, 1, 2), (3000, 2, 2), (3000, 3, 0), "hubs"]   # (n, seed, ignore_diags) of synth_full_map, or the hubs map
HUB_LENGTHS = [1500, 2600]                                  # CSR rows of 2 and 3 chunks of 1024 entries


def _newton(*a, **k):
    from mustache_amd.balance import newton
    return newton(*a, **k)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


@functools.lru_cache(maxsize=None)
def _case(case):
    """(x, y, v, n, ignore_diags, hub bins), the restatement's result and the device's, computed once per case"""
    if case == "hubs":
        n, ig = 4000, 2
        x, y, v, hubs = br.add_hubs(*br.synth_full_map(n, 5), n=n, lengths=HUB_LENGTHS, seed=7)
    else:
        n, seed, ig = case
        x, y, v = br.synth_full_map(n, seed)
        hubs = None
    return (x, y, v, n, ig, hubs), nr.newton(x, y, v, n, ignore_diags=ig), _newton(x, y, v, n, ignore_diags=ig)


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) / np.asarray(b) - 1.0)))


@pytest.mark.parametrize("case", CASES)
def test_device_matches_restatement(case):
    (x, y, v, n, ig, hubs), (want, winfo), (got, info) = _case(case)
    assert np.array_equal(info["masked"], winfo["masked"]) and 0 < int(info["masked"].sum()) < n
    assert info["converged"] and winfo["converged"]
    assert abs(info["matvecs"] - winfo["matvecs"]) <= max(2, 0.1 * winfo["matvecs"])
    assert len(info["trace"]) == info["iterations"] >= 3 and abs(info["residual"] / info["trace"][-1] - 1.0) <= 1e-15
    assert _rel(info["trace"][:3], winfo["trace"][:3]) <= 1e-6
    assert np.array_equal(np.isnan(got), info["masked"])
    ok = ~info["masked"]
    assert _rel(got[ok], want[ok]) <= 1e-6
    assert info["isolated"] == winfo["isolated"] == 0
    assert info["capped_steps"] == winfo["capped_steps"] and info["capped_upper"] == winfo["capped_upper"]
    if hubs is not None:                                    # rows of several chunks, and the lower-cap branch
        from mustache_amd.balance import BalanceCSR
        csr = BalanceCSR(x, y, v, n, ignore_diags=ig)
        assert (csr.chunk_ptr[1:] - csr.chunk_ptr[:-1]).cpu().numpy()[hubs].tolist() == [2, 3]
        assert info["capped_steps"] >= 1 and info["capped_upper"] == 0 and not info["masked"][hubs].any()


@pytest.mark.parametrize("case", CASES)
def test_balancing_condition_from_the_output_alone(case):
    """x = kappa / bias satisfies ||1 - x * (A x)||_2 <= tol, in float64 NumPy from the device's bias, kappa and mask."""
    (x, y, v, n, ig, _hubs), _, (got, info) = _case(case)
    res, kappa, act = nr.condition(x, y, v, n, got, info, ig)
    assert act.sum() == n - info["masked"].sum()
    assert np.linalg.norm(res) <= 1.001 * 1e-6
    assert abs(info["residual"] / np.linalg.norm(res) - 1.0) <= 1e-6
    assert abs(info["kappa"] / kappa - 1.0) <= 1e-12
    assert 0.0 <= info["variance"] <= 1e-12 / act.sum()     # var(v) <= mean((v - 1)^2) = residual^2 / |Act|


def test_newton_agrees_with_device_ice_at_its_fixed_point():
    from mustache_amd.balance import ice
    (x, y, v, n, ig, _hubs), _, (got, info) = _case((3000, 2, 2))
    want, winfo = ice(x, y, v, n, ignore_diags=ig, tol=1e-24, max_iter=20000)
    assert winfo["converged"] and np.array_equal(winfo["masked"], info["masked"])
    ok = ~info["masked"]
    assert _rel(got[ok], want[ok]) <= 1e-5
    assert info["matvecs"] * 20 < winfo["iterations"]       # what the method is for


def test_bit_identical_under_repeat_permutation_padding_and_duplicates():
    n = 2500
    x, y, v = br.synth_full_map(n, 21)
    b0, i0 = _newton(x, y, v, n)
    assert i0["converged"]
    b1, i1 = _newton(x, y, v, n)
    assert _same_bits(b0, b1) and i1["trace"] == i0["trace"] and i1["matvecs"] == i0["matvecs"]
    rng = np.random.default_rng(5)
    p = rng.permutation(len(v))
    assert _same_bits(b0, _newton(x[p], y[p], v[p], n)[0])  # record permutation
    flip = rng.random(len(v)) < 0.5
    assert _same_bits(b0, _newton(np.where(flip, y, x), np.where(flip, x, y), v, n)[0])   # flipped orientation
    b3, i3 = _newton(x, y, v, n + 777)                      # appended empty bins
    assert _same_bits(b0, b3[:n]) and np.isnan(b3[n:]).all() and i3["matvecs"] == i0["matvecs"]
    assert i3["trace"] == i0["trace"]
    dup = rng.choice(len(v), 3000, replace=False)           # repeated pixels, the stale entry first: the last entry wins
    xd = np.concatenate([y[dup], x])
    yd = np.concatenate([x[dup], y])
    vd = np.concatenate([v[dup] * 3.0 + 1.0, v])
    assert _same_bits(b0, _newton(xd, yd, vd, n)[0])
    import torch
    b5, _ = _newton(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(v).cuda(), n)
    assert _same_bits(b0, b5)


def test_rows_of_several_chunks_bit_identical():
    (x, y, v, n, ig, _hubs), _, (b0, i0) = _case("hubs")
    rng = np.random.default_rng(9)
    p = rng.permutation(len(v))
    flip = rng.random(len(v)) < 0.5
    assert _same_bits(b0, _newton(np.where(flip, y, x)[p], np.where(flip, x, y)[p], v[p], n, ignore_diags=ig)[0])
    b3, i3 = _newton(x, y, v, n + 1500, ignore_diags=ig)
    assert _same_bits(b0, b3[:n]) and np.isnan(b3[n:]).all() and i3["trace"] == i0["trace"]


@pytest.mark.parametrize("steps", [1, 7])
def test_steps_per_read_does_not_change_a_bit(monkeypatch, steps):
    from mustache_amd import balance
    (x, y, v, n, ig, _hubs), _, (b0, i0) = _case((600, 1, 2))
    assert balance.STEPS_PER_READ == 8
    monkeypatch.setattr(balance, "STEPS_PER_READ", steps)
    b1, i1 = _newton(x, y, v, n, ignore_diags=ig)
    assert _same_bits(b0, b1)
    for k in ("iterations", "matvecs", "residual", "variance", "capped_steps", "trace", "kappa", "converged"):
        assert i1[k] == i0[k], k


def test_isolated_bin_keeps_x_equal_one():
    x, y, v, n = nr.isolated_map()
    want, winfo = nr.newton(x, y, v, n, ignore_diags=0, min_nnz=0)
    got, info = _newton(x, y, v, n, ignore_diags=0, min_nnz=0)
    assert np.array_equal(info["masked"], winfo["masked"]) and info["masked"][61:].all() and not info["masked"][:61].any()
    assert info["converged"] and info["isolated"] == winfo["isolated"] == 1
    assert got[60] == info["kappa"]
    res, kappa, act = nr.condition(x, y, v, n, got, info, 0)
    assert act.sum() == 60 and not act[60] and np.linalg.norm(res) <= 1.001 * 1e-6
    assert abs(info["kappa"] / kappa - 1.0) <= 1e-12
    assert _rel(got[:61], want[:61]) <= 1e-6


def test_upper_cap():
    n = 600
    x, y, v = br.synth_full_map(n, 1)
    want, winfo = nr.newton(x, y, v * 1e-4, n)
    got, info = _newton(x, y, v * 1e-4, n)
    assert winfo["capped_upper"] >= 1 and info["capped_upper"] == winfo["capped_upper"]
    assert info["capped_steps"] == winfo["capped_steps"] and info["converged"] and winfo["converged"]
    assert abs(info["matvecs"] - winfo["matvecs"]) <= 2
    assert _rel(info["trace"][:3], winfo["trace"][:3]) <= 1e-6
    ok = ~info["masked"]
    assert np.array_equal(info["masked"], winfo["masked"]) and _rel(got[ok], want[ok]) <= 1e-6
    assert np.linalg.norm(nr.condition(x, y, v * 1e-4, n, got, info)[0]) <= 1.001 * 1e-6


def test_matvec_limit_and_all_masked(capsys):
    from mustache_amd.balance import balance_text, report
    n = 600
    x, y, v = br.synth_full_map(n, 1)
    want, winfo = nr.newton(x, y, v, n, max_matvecs=3)
    got, info = _newton(x, y, v, n, max_matvecs=3)
    assert not info["converged"] and info["matvecs"] == winfo["matvecs"] and info["iterations"] == winfo["iterations"]
    ok = ~info["masked"]
    assert np.isfinite(got[ok]).all() and _rel(got[ok], want[ok]) <= 1e-10
    assert abs(info["residual"] / winfo["residual"] - 1.0) <= 1e-10
    report(info, "chromosome 1")
    out = capsys.readouterr().out
    assert "Warning" in out and "NEWTON" in out and "did not converge in %d mat-vecs" % info["matvecs"] in out
    b, info = _newton(x, y, v, n, max_matvecs=0)            # nothing but the start: x = 1
    assert not info["converged"] and info["matvecs"] == 0 and info["iterations"] == 0 and info["trace"] == []
    assert np.all(b[~info["masked"]] == info["kappa"])
    b, info = _newton(x, y, v, n, min_nnz=10 ** 6)          # every bin masked
    assert np.isnan(b).all() and info["masked"].all() and info["iterations"] == 0 and info["matvecs"] == 0
    assert info["converged"] and info["trace"] == []
    b, info = balance_text(np.zeros(0), np.zeros(0), np.zeros(0), 5000, method="NEWTON")    # no bin at all
    assert len(b) == 0 and info["matvecs"] == 0 and info["method"] == "NEWTON"


# ---- the command lines ---------------------------------------------------------------------------------------------------
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
def test_cli_balance_equals_written_bias(tmp_path, capsys, res, n, dpx, dist):
    from mustache_amd.balance import balance_text, write_bias
    from mustache_amd.mustache import main
    x, y, v = _maps(n, dpx, 40 + res % 7, n // 40)
    t = str(tmp_path / "map.txt")
    _write_text(t, x, y, v, res)
    o1, o2, bf = str(tmp_path / "bal.tsv"), str(tmp_path / "b.tsv"), str(tmp_path / "bias.tsv")
    main(["-f", t, "-r", str(res), "-d", dist, "-ch", "1", "-o", o1, "--balance", "NEWTON"])
    assert "NEWTON balancing of chromosome 1:" in capsys.readouterr().out
    bias, info = balance_text(x * float(res), y * float(res), v, res, method="NEWTON")
    assert info["converged"] and info["method"] == "NEWTON" and info["matvecs"] <= 60
    write_bias(bf, "1", res, bias)
    main(["-f", t, "-r", str(res), "-d", dist, "-ch", "1", "-o", o2, "-b", bf])
    a, b = open(o1).read(), open(o2).read()
    assert a == b
    assert a.count("\n") > 5                        # loops were called


def test_hic_route(tmp_path, capsys, monkeypatch):
    from hic_writer import write_hic
    from mustache_amd.balance import balance_text
    from mustache_amd.hicfile import HicFile, read_intra_packed
    from mustache_amd.mustache import call_loops_coo, main, regulator
    n, dpx, res = 3000, 200, 5000
    x, y, v = _maps(n, dpx, 61, 80)
    h = str(tmp_path / "m.hic")
    write_hic(h, [("All", 1000), ("chr1", n * res)], {1: {res: (x, y, v)}}, {}, version=8, block_bin_count=200,
              float_counts=True)
    bt, it = balance_text(x * float(res), y * float(res), v, res, method="NEWTON")
    with HicFile(h) as hf:
        pc = read_intra_packed(hf, "chr1", res, "NONE", -1, n * res)
    hx, hd, hv = pc.coo()
    assert len(hv) == len(v)
    bh, ih = _newton(hx, hd, hv, int(hd.max()) + 1)
    m = min(len(bt), len(bh))
    assert ih["converged"] and _same_bits(bt[:m], bh[:m]) and ih["matvecs"] == it["matvecs"]
    # the records the route hands on: (v / b[x]) / b[y], +inf for NaN / < 0.2, the reader's own distance rule, v' > 0
    monkeypatch.setenv("MUSTACHE_HIC_BACKEND", "native")

    def f(k):
        return bh[k] if (not np.isnan(bh[k]) and bh[k] >= 0.2) else np.inf
    keep = (hd - hx) <= 1000000 // res
    ex, ey, ev = hx[keep], hd[keep], hv[keep]
    ev = (ev / np.array([f(k) for k in ex])) / np.array([f(k) for k in ey])
    pos = ev > 0
    want = call_loops_coo(ex[pos], ey[pos], ev[pos], res, 200, [1.6, 3.2], 0.88, 0.2, verbose=False)
    got = regulator(h, False, False, None, res=res, distance_filter=1000000, chromosome="chr1", balance="NEWTON",
                    pt=0.2, st=0.88, verbose=False)
    assert len(want) > 5
    assert [[int(a), int(b)] for a, b, _, _ in got] == [[int(a), int(b)] for a, b, _, _ in want]
    assert all(g[2] == w[2] and g[3] == w[3] for g, w in zip(got, want))
    capsys.readouterr()
    out = str(tmp_path / "h.tsv")
    main(["-f", h, "-r", str(res), "-d", "1000000", "-ch", "chr1", "-o", out, "--balance", "NEWTON"])
    text = capsys.readouterr().out
    assert "raw counts for NEWTON balancing" in text and "NEWTON balancing of chromosome chr1:" in text
    assert open(out).read().count("\n") == len(want) + 1


def test_diff_mustache_balance(tmp_path, capsys):
    """`--balance NEWTON` balances each sample on its own: the four files equal regulator()'s rows with both written vectors
    (bias1=, bias2=), as tests/test_gpu_balance.py checks for ICE."""
    from mustache_amd.balance import balance_text, write_bias
    from mustache_amd.diff_mustache import HEADER, SUFFIX, main, regulator
    from mustache_amd.mustache import _scalar_text
    n, dpx, res = 3000, 200, 5000
    paths, biases = [], []
    for s in (0, 1):
        x, y, v = _maps(n, dpx, 70 + s, 80)
        t = str(tmp_path / ("s%d.txt" % s))
        _write_text(t, x, y, v, res)
        b, _ = balance_text(x * float(res), y * float(res), v, res, method="NEWTON")
        bf = str(tmp_path / ("b%d.tsv" % s))
        write_bias(bf, "1", res, b)
        paths.append(t)
        biases.append(bf)
    out = str(tmp_path / "d")
    main(["-f1", paths[0], "-f2", paths[1], "-r", str(res), "-d", "1000000", "-ch", "1", "-o", out, "--balance", "NEWTON"])
    assert capsys.readouterr().out.count("NEWTON balancing of chromosome 1:") == 2
    rows = regulator(paths[0], paths[1], False, False, None, res=res, distance_filter=1000000, bias1=biases[0],
                     bias2=biases[1], chromosome="1", pt=0.2, pt2=0.1, st=0.88, verbose=False)   # the CLI's defaults
    assert len(rows) > 5
    for tag, suf in SUFFIX.items():
        want = HEADER + "".join("1\t%d\t%d\t1\t%d\t%d\t%s\t%s\n" % (int(r[0]) * res, (int(r[0]) + 1) * res, int(r[1]) * res,
                                                                    (int(r[1]) + 1) * res, _scalar_text(r[2]), _scalar_text(r[3]))
                                for r in rows if r[4] == tag)
        assert open(out + suf).read() == want, suf


def test_pileup_balance(tmp_path, capsys):
    """`pileup --balance NEWTON` writes what `pileup -b` writes with the vector balance_text returns."""
    from mustache_amd.balance import balance_text, write_bias
    from mustache_amd.pileup import main
    n, dpx, res = 1500, 120, 10000
    x, y, v = _maps(n, dpx, 9, 40)
    t = str(tmp_path / "m.txt")
    _write_text(t, x, y, v, res)
    bias, info = balance_text(x * float(res), y * float(res), v, res, method="NEWTON")
    assert info["converged"]
    bf = str(tmp_path / "b.tsv")
    write_bias(bf, "1", res, bias)
    rng = np.random.default_rng(4)
    xs = rng.integers(20, n - 130, 60)
    ys = xs + rng.integers(30, 100, 60)
    lp = str(tmp_path / "l.tsv")
    with open(lp, "w") as fh:
        fh.write("BIN1_CHR\tBIN1_START\tBIN1_END\tBIN2_CHROMOSOME\tBIN2_START\tBIN2_END\tFDR\tDETECTION_SCALE\n")
        fh.write("".join("1\t%d\t%d\t1\t%d\t%d\t0.01\t1.6\n" % (a * res, (a + 1) * res, b * res, (b + 1) * res)
                         for a, b in zip(xs, ys)))
    o1, o2 = str(tmp_path / "o1"), str(tmp_path / "o2")
    main(["-f", t, "-l", lp, "-r", str(res), "-o", o1, "--balance", "NEWTON"])
    assert "NEWTON balancing of chromosome 1:" in capsys.readouterr().out
    main(["-f", t, "-l", lp, "-r", str(res), "-o", o2, "-b", bf])
    for suf in (".apa.tsv", ".oe.tsv", ".stats.tsv", ".loops.tsv"):
        a, b = open(o1 + suf).read(), open(o2 + suf).read()
        assert a == b and len(a) > 0, suf
    assert "used" in open(o1 + ".loops.tsv").read()
