"""CPU tests of the Newton balancing restatement (tests/newton_reference.py), of report() and of the --balance NEWTON
refusals.  No GPU."""
import os

import numpy as np
import pytest

import balance_reference as br
import newton_reference as nr

CASES = [(600, 1, 2), (3000, 2, 2), (3000, 3, 0)]           # n, seed, ignore_diags


@pytest.fixture(scope="module")
def solved():
    """(map, Newton result, ICE fixed point) of every case, computed once."""
    out = {}
    for n, seed, ig in CASES:
        x, y, v = br.synth_full_map(n, seed)
        out[(n, seed, ig)] = ((x, y, v), nr.newton(x, y, v, n, ignore_diags=ig),
                              br.ice(x, y, v, n, ignore_diags=ig, tol=1e-24, max_iter=20000))
    return out


# measured with this restatement (mat-vecs; max |x (A x) - 1|; largest relative difference from the ICE fixed point):
#   (600, 1, 2): 26, 1.7e-7, 1.9e-7     (3000, 2, 2): 27, 3.6e-8, 4.9e-8     (3000, 3, 0): 25, 1.0e-7, 1.2e-7
@pytest.mark.parametrize("case", CASES)
def test_converges_and_meets_the_condition(solved, case):
    n, _seed, ig = case
    (x, y, v), (bias, info), _ = solved[case]
    assert info["converged"] and info["matvecs"] <= 60
    assert info["iterations"] == len(info["trace"]) and info["residual"] == info["trace"][-1] <= 1e-6
    assert info["isolated"] == 0 and 0 < int(info["masked"].sum()) < n
    res, kappa, act = nr.condition(x, y, v, n, bias, info, ig)
    assert np.array_equal(act, info["active"]) and act.sum() == n - info["masked"].sum()
    assert np.max(np.abs(res)) <= 1e-6
    assert abs(kappa / info["kappa"] - 1.0) <= 1e-12
    assert info["variance"] <= 1e-12 / act.sum()             # var(v) <= mean((v - 1)^2) = residual^2 / |Act|


@pytest.mark.parametrize("case", CASES)
def test_agrees_with_the_ice_fixed_point(solved, case):
    _, (bias, info), (want, winfo) = solved[case]
    assert winfo["converged"]
    assert np.array_equal(info["masked"], winfo["masked"])
    assert np.array_equal(np.isnan(bias), info["masked"]) and np.array_equal(np.isnan(want), info["masked"])
    ok = ~info["masked"]
    assert np.max(np.abs(bias[ok] / want[ok] - 1.0)) <= 1e-5


def test_lower_cap():
    n = 4000
    x, y, v, _hubs = br.add_hubs(*br.synth_full_map(n, 5), n=n, lengths=[1500, 2600], seed=7)
    bias, info = nr.newton(x, y, v, n)
    assert info["converged"] and info["matvecs"] <= 60
    assert info["capped_steps"] >= 1 and info["capped_upper"] == 0
    assert np.max(np.abs(nr.condition(x, y, v, n, bias, info)[0])) <= 1e-6


def test_upper_cap():
    """Counts of 1e-4 of the usual ones: x has to grow a hundredfold, more than Delta = 3 per outer iteration allows."""
    n = 600
    x, y, v = br.synth_full_map(n, 1)
    bias, info = nr.newton(x, y, v * 1e-4, n)
    assert info["converged"] and info["capped_upper"] >= 1 and info["capped_steps"] >= info["capped_upper"]
    assert np.max(np.abs(nr.condition(x, y, v * 1e-4, n, bias, info)[0])) <= 1e-6
    plain, pinfo = nr.newton(x, y, v, n)                    # kappa takes the scale of the counts: the bias is the same
    ok = ~info["masked"]
    assert np.array_equal(info["masked"], pinfo["masked"]) and pinfo["capped_steps"] == 0
    assert abs(info["kappa"] / (pinfo["kappa"] * 1e2) - 1.0) <= 1e-5
    assert np.max(np.abs(bias[ok] / plain[ok] - 1.0)) <= 1e-5


def test_isolated_bin_keeps_x_equal_one():
    x, y, v, n = nr.isolated_map()
    bias, info = nr.newton(x, y, v, n, ignore_diags=0, min_nnz=0)
    assert info["masked"][61:].all() and not info["masked"][:61].any()
    assert info["converged"] and info["isolated"] == 1 and not info["active"][60]
    assert bias[60] == info["kappa"]
    res, _kappa, act = nr.condition(x, y, v, n, bias, info, 0)
    assert act.sum() == 60 and np.max(np.abs(res)) <= 1e-6


def test_matvec_limit(capsys):
    from mustache_amd.balance import report
    n = 600
    x, y, v = br.synth_full_map(n, 1)
    bias, info = nr.newton(x, y, v, n, max_matvecs=3)
    assert not info["converged"] and 3 <= info["matvecs"] <= 4
    assert np.isfinite(bias[~info["masked"]]).all() and (bias[~info["masked"]] > 0).all()
    report(info, "chromosome 1")
    out = capsys.readouterr().out
    assert "Warning" in out and "NEWTON" in out and "did not converge" in out
    report(nr.newton(x, y, v, n)[1], "chromosome 1")
    out = capsys.readouterr().out
    assert "Warning" not in out and "NEWTON balancing of chromosome 1" in out and "mat-vecs" in out


def test_all_masked():
    n = 600
    x, y, v = br.synth_full_map(n, 1)
    bias, info = nr.newton(x, y, v, n, min_nnz=10 ** 6)
    assert np.isnan(bias).all() and info["masked"].all() and info["iterations"] == 0 and info["matvecs"] == 0


# ---- the command lines ---------------------------------------------------------------------------------------------------
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


def test_check_request_accepts_newton():
    from mustache_amd.balance import METHODS, BalanceError, check_request, method_of
    assert METHODS == ("ICE", "NEWTON")
    assert check_request("newton", "m.txt", None, "NONE") == "NEWTON"
    assert check_request("NEWTON", "m.hic", False, False) == "NEWTON"
    assert method_of("newton") == "NEWTON" and method_of("ICE") == "ICE" and method_of(True) == "ICE"
    with pytest.raises(BalanceError, match="unknown method"):
        check_request("KR", "m.txt", None, "NONE")


def test_cli_refusals_hold_for_newton(inputs, capsys, monkeypatch):
    from mustache_amd import sharding
    from mustache_amd.mustache import main
    t, b, c, out = inputs
    base = ["-r", "5000", "-ch", "1", "-o", out, "--balance", "NEWTON"]
    main(["-f", t] + base + ["-b", b])
    _refused(capsys, out, "-b")
    main(["-f", t] + base + ["-norm", "KR"])
    _refused(capsys, out, "-norm KR")
    main(["-f", c] + base)
    _refused(capsys, out, "weight")
    main(["-f", t, "-r", "5000", "-ch", "1", "-ch2", "2", "-o", out, "--balance", "NEWTON"])
    _refused(capsys, out, "inter-chromosomal")
    monkeypatch.setattr(sharding, "init_from_env", lambda: (0, 2))
    main(["-f", t] + base)
    _refused(capsys, out, "multi-rank")


def test_diff_cli_refusals_hold_for_newton(inputs, capsys, monkeypatch):
    from mustache_amd import sharding
    from mustache_amd.diff_mustache import main
    t, b, c, out = inputs
    base = ["-f1", t, "-f2", t, "-r", "5000", "-ch", "1", "-o", out, "--balance", "NEWTON"]
    main(base + ["-b1", b])
    _refused(capsys, out, "-b1/-b2")
    main(base + ["-b2", b])
    _refused(capsys, out, "-b1/-b2")
    main(base + ["-norm", "VC"])
    _refused(capsys, out, "-norm VC")
    main(["-f1", t, "-f2", c, "-r", "5000", "-ch", "1", "-o", out, "--balance", "NEWTON"])
    _refused(capsys, out, "weight")
    monkeypatch.setattr(sharding, "init_from_env", lambda: (0, 2))
    main(base)
    _refused(capsys, out, "multi-rank")


def test_help_names_both_methods(capsys):
    from mustache_amd import diff_mustache, mustache, pileup
    for mod in (mustache, diff_mustache, pileup):
        with pytest.raises(SystemExit):
            mod.parse_args(["-h"])
        assert "ICE|NEWTON" in capsys.readouterr().out, mod.__name__


def test_stale_library_fails_with_the_version_message(monkeypatch):
    """A library older than the binding is refused by its version and revision, before any symbol it lacks is looked up."""
    import ctypes
    from mustache_amd import _lib
    assert {"mst_balance_newton", "mst_balance_newton_workspace_bytes", "mst_abi_revision"} <= set(_lib.exported_symbols())
    assert _lib.load().mst_abi_revision() == _lib.MST_ABI_REVISION >= 1
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "MST_ABI_REVISION", _lib.MST_ABI_REVISION + 1)       # a binding newer than the library
    monkeypatch.setitem(_lib._SIGNATURES, "mst_entry_point_of_a_newer_binding", (ctypes.c_int, []))
    with pytest.raises(ImportError, match=r"ABI version mismatch \(library 3\.1, binding 3\.2\)"):
        _lib.load()
