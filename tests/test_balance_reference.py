"""CPU tests of the ICE restatement (tests/balance_reference.py), the bias file form and the --balance refusals.  No GPU."""
import os

import numpy as np
import pytest

import balance_reference as br


def _dense_to_coo(A):
    i, j = np.nonzero(np.triu(A))
    return i, j, A[i, j]


def _newton_balance(A, iters=100):
    """x with x_i * sum_j A_ij x_j = 1 for every i (Newton on F(x) = x * (A x) - 1): bias ∝ 1 / x."""
    x = np.ones(len(A)) / np.sqrt(A.sum(1).mean())
    for _ in range(iters):
        Ax = A @ x
        F = x * Ax - 1.0
        J = np.diag(Ax) + x[:, None] * A
        x = x - np.linalg.solve(J, F)
        if np.max(np.abs(F)) < 1e-15:
            break
    return x


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("n", [6, 13, 24])
def test_restatement_matches_exact_balancing(n, seed):
    rng = np.random.default_rng(seed)
    A = rng.uniform(0.5, 20.0, (n, n))
    A = A + A.T                                         # symmetric, all positive: fully indecomposable
    x, y, v = _dense_to_coo(A)
    # var < tol bounds the spread of r by sqrt(tol); at tol = 1e-14 the bias is only within ~1e-7 of the exact one, so the
    # iteration is run to var < 1e-20 here
    bias, info = br.ice(x, y, v, n, ignore_diags=0, min_nnz=1, mad_max=1e9, tol=1e-20, max_iter=10000)
    assert info["converged"] and not info["masked"].any()
    exact = 1.0 / _newton_balance(A)
    got, want = bias / bias[0], exact / exact[0]
    assert np.max(np.abs(got / want - 1.0)) < 1e-8
    # the balanced matrix has equal row sums, and kappa keeps its total (i <= j) equal to the raw total
    B = A / np.outer(bias, bias)
    rs = B.sum(1)
    assert np.max(np.abs(rs / rs.mean() - 1.0)) < 1e-7
    assert abs(np.triu(B).sum() / np.triu(A).sum() - 1.0) < 1e-12


def test_dkd_returns_d():
    n = 40
    k = np.arange(n)
    dist = np.minimum(np.abs(k[:, None] - k[None, :]), n - np.abs(k[:, None] - k[None, :]))
    K = 1.0 / (1.0 + dist) ** 1.5                       # symmetric circulant: already balanced
    D = np.random.default_rng(4).uniform(0.3, 3.0, n)
    A = D[:, None] * K * D[None, :]
    x, y, v = _dense_to_coo(A)
    bias, info = br.ice(x, y, v, n, ignore_diags=0, min_nnz=1, mad_max=1e9, tol=1e-20, max_iter=5000)
    r = bias / D
    assert np.max(np.abs(r / r.mean() - 1.0)) < 1e-9


def _banded(n, width, seed=3):
    x, y = [], []
    for i in range(n):
        for j in range(i, min(n, i + width)):
            x.append(i)
            y.append(j)
    return np.array(x), np.array(y), np.random.default_rng(seed).uniform(2.0, 8.0, len(x))


def test_filters_mask_the_right_bins():
    n = 60
    x, y, v = _banded(n, 15)
    keep = ~((x == 20) | (y == 20))                     # bin 20: empty
    x, y, v = x[keep], y[keep], v[keep]
    few = (x == 30) | (y == 30)                         # bin 30: only 4 non-zeros left (diagonals 2, 3)
    keep = ~few | (np.abs(y - x) >= 2) & (np.abs(y - x) <= 3)
    x, y, v = x[keep], y[keep], v[keep]
    v = v.copy()
    faint = (x == 40) | (y == 40)                       # bin 40: as many non-zeros as its neighbours, 1e-6 of their weight
    v[faint] = 5e-6
    masked, m, cut = br.filter_mask(*br.kept_pixels(x, y, v, n, 2), n, min_nnz=10, mad_max=5.0, details=True)
    assert masked[20] and masked[30] and masked[40]
    assert m[30] == 0                                   # step 3 removes the masked rows and columns
    assert not masked[[0, 10, 25, 35, 50, 59]].any()
    assert int(masked.sum()) == 3
    # ignore_diags: a bin whose only pixels lie on diagonals 0 and 1 is empty after step 1
    xs, ys, vs = _banded(n, 15)
    only_near = ((xs == 45) | (ys == 45)) & (np.abs(ys - xs) > 1)
    xs, ys, vs = xs[~only_near], ys[~only_near], vs[~only_near]
    assert br.filter_mask(*br.kept_pixels(xs, ys, vs, n, 2), n)[45]
    assert not br.filter_mask(*br.kept_pixels(xs, ys, vs, n, 0), n, min_nnz=2, mad_max=1e9)[45]


def test_repeated_pixels_last_wins_either_orientation():
    i, j, v = br.kept_pixels([3, 9, 3, 1], [9, 3, 9, 7], [1.0, 2.0, 4.0, 8.0], 12, 2)
    assert list(zip(i.tolist(), j.tolist(), v.tolist())) == [(1, 7, 8.0), (3, 9, 4.0)]


def test_write_bias_round_trips_through_read_bias(tmp_path):
    from mustache_amd.balance import bias_lookup, write_bias
    from mustache_amd.mustache import read_bias
    rng = np.random.default_rng(7)
    bias = rng.lognormal(0.0, 0.7, 500)
    bias[[3, 77, 499]] = np.nan
    bias[10] = 0.15                                     # below read_bias' cut-off
    bias[11] = 1.0 / 3.0
    p = tmp_path / "b.tsv"
    write_bias(str(p), "chr7", 5000, bias)
    back = np.array([float(line.split("\t")[2]) for line in open(p)])
    assert np.array_equal(back.view(np.int64)[~np.isnan(back)], bias.view(np.int64)[~np.isnan(bias)])
    assert np.array_equal(np.isnan(back), np.isnan(bias))
    d = read_bias(str(p), "7", 5000)
    want = bias_lookup(bias)
    assert set(d) == set(want) == set(float(i) for i in range(500))
    for k in d:
        assert d[k] == want[k] or (np.isnan(d[k]) and np.isnan(want[k]))
    assert d[3.0] == np.inf and d[10.0] == np.inf and d[11.0] == 1.0 / 3.0


@pytest.fixture
def inputs(tmp_path):
    t = tmp_path / "map.txt"
    t.write_text("0\t5000\t3\n5000\t10000\t4\n")
    b = tmp_path / "bias.txt"
    b.write_text("1.0\n1.0\n1.0\n")
    c = tmp_path / "map.cool"
    c.write_text("")
    return str(t), str(b), str(c), str(tmp_path / "out")


def _refused(capsys, out, needle):
    text = capsys.readouterr().out
    assert "Error:" in text and needle in text, text
    assert not any(os.path.exists(out + s) for s in ("", ".loop1", ".diffloop1", ".loop2", ".diffloop2"))


@pytest.mark.parametrize("extra,needle", [
    (["-b", "{b}"], "-b"),
    (["-norm", "KR"], "-norm KR"),
    ([], "unknown method"),
])
def test_cli_refusals(inputs, capsys, extra, needle):
    from mustache_amd.mustache import main
    t, b, _c, out = inputs
    method = "KR" if needle == "unknown method" else "ICE"
    main(["-f", t, "-r", "5000", "-ch", "1", "-o", out, "--balance", method] + [e.format(b=b) for e in extra])
    _refused(capsys, out, needle)


def test_cli_refuses_cool_and_multirank(inputs, capsys, monkeypatch):
    from mustache_amd import sharding
    from mustache_amd.mustache import main
    t, _b, c, out = inputs
    main(["-f", c, "-r", "5000", "-ch", "1", "-o", out, "--balance", "ICE"])
    _refused(capsys, out, "weight")
    monkeypatch.setattr(sharding, "init_from_env", lambda: (0, 2))
    main(["-f", t, "-r", "5000", "-ch", "1", "-o", out, "--balance", "ICE"])
    _refused(capsys, out, "multi-rank")


def test_diff_cli_refusals(inputs, capsys, monkeypatch):
    from mustache_amd import sharding
    from mustache_amd.diff_mustache import main
    t, b, c, out = inputs
    base = ["-f1", t, "-f2", t, "-r", "5000", "-ch", "1", "-o", out]
    main(base + ["--balance", "ICE", "-b1", b])
    _refused(capsys, out, "-b1/-b2")
    main(base + ["--balance", "ICE", "-b2", b])
    _refused(capsys, out, "-b1/-b2")
    main(base + ["--balance", "ICE", "-norm", "VC"])
    _refused(capsys, out, "-norm VC")
    main(base + ["--balance", "SCALE"])
    _refused(capsys, out, "unknown method")
    main(["-f1", t, "-f2", c, "-r", "5000", "-ch", "1", "-o", out, "--balance", "ICE"])
    _refused(capsys, out, "weight")
    monkeypatch.setattr(sharding, "init_from_env", lambda: (0, 2))
    main(base + ["--balance", "ICE"])
    _refused(capsys, out, "multi-rank")


def test_norm_none_is_accepted():
    from mustache_amd.balance import check_request
    assert check_request("ice", "m.txt", None, "NONE") == "ICE"
    assert check_request("ICE", "m.hic", False, False) == "ICE"
