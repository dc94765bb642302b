"""Whole-genome balancing for inter-chromosomal calling (mustache_amd/balance_genome.py) on the MI355X: genome_bias against the
NumPy restatement (tests/balance_genome_reference.py), the bias to the bit under what must not change it, the entry point
mst_balance_apply_pairs alone, both command lines end to end, and the memory refusal."""
import os

import numpy as np
import pytest

import balance_genome_reference as gr
import newton_reference as nr
import trans_reference as tr
from hic_trans_writer import write_hic_pairs

pytestmark = pytest.mark.gpu

RES = 10000
BINS = (70, 50, 40)
OCT = [1.6, 3.2]
ST, PT, PT2 = 0.88, 0.2, 0.1


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) / np.asarray(b) - 1.0)))


def _write(path, bins, cis, trans, version=8, extra=()):
    chroms, mats = gr.hic_arguments(bins, RES, cis, trans, extra)
    write_hic_pairs(str(path), chroms, mats, version=version)
    return str(path)


# ---- 1. genome_bias against the restatement --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    cis, trans = gr.synth_genome(BINS)
    d = tmp_path_factory.mktemp("balance_genome")
    _, off, n = gr.layout([b * RES - 1 for b in BINS], RES)
    return dict(cis=cis, trans=trans, off=off, n=n, v8=_write(d / "g8.hic", BINS, cis, trans), dir=d, want={})


def _want(genome, method, pixels):
    key = (method, pixels)
    if key not in genome["want"]:
        lo, hi, v = gr.assemble(list(BINS), genome["off"], genome["cis"], genome["trans"], pixels)
        genome["want"][key] = (lo, hi, v) + gr.balance(method, lo, hi, v, genome["n"])
    return genome["want"][key]


@pytest.mark.parametrize("pixels", ["all", "inter"])
@pytest.mark.parametrize("method", ["NEWTON", "ICE"])
def test_genome_bias_matches_the_restatement(genome, method, pixels):
    from mustache_amd.balance_genome import genome_bias
    lo, hi, v, want, winfo = _want(genome, method, pixels)
    gb = genome_bias(genome["v8"], RES, method=method, pixels=pixels)
    assert gb.chromosomes == ["1", "2", "3"] and gb.offsets == genome["off"] and gb.n == genome["n"] == 160
    assert gb.info["pixels"] == pixels and gb.info["method"] == method and gb.info["records"] == len(v)
    assert gb.info["converged"] and winfo["converged"]
    masked = gb.info["masked"]
    assert np.array_equal(masked, winfo["masked"]) and 0 < int(masked.sum()) < gb.n
    assert np.isnan(gb.bias[masked]).all()
    print(method, pixels, len(v), int(masked.sum()), _rel(gb.bias[~masked], want[~masked]))
    assert _rel(gb.bias[~masked], want[~masked]) <= 1e-6
    _, kappa, _ = nr.condition(lo, hi, v, gb.n, gb.bias, gb.info, ignore_diags=0)
    assert abs(gb.info["kappa"] / kappa - 1.0) <= 1e-12
    assert gb.of("2").tobytes() == gb.bias[70:120].tobytes() and gb.of("chr3").tobytes() == gb.bias[120:].tobytes()
    # the resident records are the file's raw ones; a pair asked for the other way round comes transposed
    x, y, c = (t.cpu().numpy() for t in gb.records("1", "3"))
    ex, ey, ec = genome["trans"][(0, 2)]
    o = np.lexsort((y, x))
    assert np.array_equal(x[o], ex) and np.array_equal(y[o], ey) and np.array_equal(c[o], ec)
    tx, ty, tc = (t.cpu().numpy() for t in gb.records("3", "1"))
    assert np.array_equal(tx, y) and np.array_equal(ty, x) and np.array_equal(tc, c)
    assert gb.records("1", "1") is None


# ---- 2. bit identity ---------------------------------------------------------------------------------------------------------
def test_the_bias_keeps_its_bits(genome):
    """Under a repeat run, the file's v9 form, the pair's records entered as (2, 1) and an extra chromosome without a record.
    (A `.hic` file keys a pair by the lower chromosome index first and the reader looks it up so: a file that stores the pair
    the other way round cannot be read at all.  The orientation is therefore exercised where it can occur -- the records of
    the pair enter the device solver as (bin of 2, bin of 1), in another order -- and through a request for (2, 1).)"""
    import torch
    from mustache_amd import balance
    from mustache_amd.balance_genome import balanced_pair, genome_bias
    first = genome_bias(genome["v8"], RES, method="NEWTON", pixels="all")
    bits = first.bias.tobytes()
    assert genome_bias(genome["v8"], RES, method="NEWTON", pixels="all").bias.tobytes() == bits
    v9 = _write(genome["dir"] / "g9.hic", BINS, genome["cis"], genome["trans"], version=9)
    assert genome_bias(v9, RES, method="NEWTON", pixels="all").bias.tobytes() == bits
    # the pair (1, 2) as (2, 1): x = bins of 2, y = bins of 1, the records reversed; the solver's own entry point
    x, y, c = genome["trans"][(0, 1)]
    swapped = dict(genome["trans"])
    del swapped[(0, 1)]
    swapped[(1, 0)] = (y[::-1], x[::-1], c[::-1])
    for tr_set in (genome["trans"], swapped):
        cells = {}
        for (a, b), (px, py, pv) in tr_set.items():
            cells[(a, b)] = (genome["off"][a] + np.asarray(px), genome["off"][b] + np.asarray(py), pv)
        ci = [(genome["off"][k] + i, genome["off"][k] + j, cv) for k, (i, j, cv) in genome["cis"].items()]
        ci = [(i[j - i >= 2], j[j - i >= 2], cv[j - i >= 2]) for i, j, cv in ci]
        parts = ci + list(cells.values())
        ga, gb_, gv = (np.concatenate([p[k] for p in parts]) for k in range(3))
        bias, _ = balance.solve("NEWTON", ga, gb_, gv, genome["n"], ignore_diags=0)
        assert bias.tobytes() == bits
    fwd = [t.cpu().numpy() for t in balanced_pair(first, "1", "2")]
    rev = [t.cpu().numpy() for t in balanced_pair(first, "2", "1")]
    assert np.array_equal(fwd[0], rev[1]) and np.array_equal(fwd[1], rev[0])
    # the rule divides by the first chromosome's bias first: (2, 1) is (v / b_2) / b_1, to the bit, and within two roundings
    # of (v / b_1) / b_2
    raw = [t.cpu().numpy() for t in first.records("2", "1")]
    want_rev = gr.balanced(first.bias, genome["off"][1], genome["off"][0], *raw)
    assert all(np.array_equal(a, b) for a, b in zip(rev[:2], want_rev[:2])) and rev[2].tobytes() == want_rev[2].tobytes()
    assert _rel(fwd[2], rev[2]) <= 4 * np.finfo(np.float64).eps
    # an extra chromosome that holds no record: its bins are NaN, the others keep their bits
    more = _write(genome["dir"] / "g4.hic", BINS, genome["cis"], genome["trans"], extra=("4",))
    gb4 = genome_bias(more, RES, method="NEWTON", pixels="all")
    assert gb4.chromosomes == ["1", "2", "3", "4"] and gb4.n == 161 and gb4.offsets[3] == 160
    assert np.isnan(gb4.of("4")).all() and gb4.bias[:160].tobytes() == bits
    assert gb4.records("1", "4") is None
    torch.cuda.synchronize()


# ---- 3. mst_balance_apply_pairs alone ----------------------------------------------------------------------------------------
def _apply_case():
    rng = np.random.default_rng(5)
    n = 300
    bias = np.exp(rng.normal(0.0, 0.4, n))
    bias[[3, 120, 250]] = np.nan
    bias[[7, 121, 298]] = 0.1
    bias[200] = 0.2                                         # kept: the rule is b < 0.2
    sizes = [0, 1, 4097]                                    # an empty segment, one record, more than a workgroup's 512
    row_off = np.array([10, 100, 0], np.int64)
    col_off = np.array([20, 200, 150], np.int64)
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    x = np.concatenate([[50], rng.integers(0, 150, 4097)]).astype(np.int32)
    y = np.concatenate([[99], rng.integers(0, 150, 4097)]).astype(np.int32)      # 200 + 99 = n - 1
    y[1], y[2], y[3], x[4] = 149, 150, 151, -1              # 150 + 149 = n - 1; one record at n, one past it; a negative bin
    v = rng.integers(1, 500, 4098).astype(np.float64)
    v[10] = np.nan
    pair = np.repeat(np.arange(3), sizes)
    want = gr.apply(bias, row_off[pair], col_off[pair], x, y, v)
    return n, bias, seg, row_off, col_off, x, y, v, want


def _same(got, want):
    """bit-equal, NaN where NaN (whose payload the rule does not fix)"""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and got[~nan].tobytes() == want[~nan].tobytes()


def test_apply_pairs_alone():
    import torch
    from mustache_amd import _lib
    from mustache_amd.balance_genome import apply_pairs
    n, bias, seg, row_off, col_off, x, y, v, want = _apply_case()
    dev = torch.device("cuda")
    d = {k: torch.from_numpy(a).to(dev) for k, a in dict(bias=bias, seg=seg, row=row_off, col=col_off, x=x, y=y, v=v).items()}
    got = apply_pairs(d["x"], d["y"], d["v"], d["seg"], d["row"], d["col"], d["bias"]).cpu().numpy()
    _same(got, want)
    # the records at n - 1 (both segments) are read and kept; the ones at n and past it and the negative bin come out as 0
    assert got[0] == (v[0] / bias[150]) / bias[299] > 0 and got[1] == (v[1] / bias[x[1]]) / bias[299]
    assert got[2] == 0.0 and got[3] == 0.0 and got[4] == 0.0 and np.isnan(got[10])
    for k in (3, 120, 250, 7, 121, 298):                    # NaN and < 0.2 bins drop their records
        hit = np.concatenate([[False], (x[1:] == k) | (y[1:] + 150 == k)])
        assert hit.any() and not (got[hit] > 0).any(), k
    assert (got[np.concatenate([[False], (y[1:] + 150 == 200) & np.isin(x[1:], [3, 120, 7, 121], invert=True)])] > 0).all()
    dropped = ~(want > 0)
    assert dropped.sum() > 100 and (want > 0).sum() > 3000
    # the one-record-a-thread form (pointers not aligned for the 16-byte form): the same bits
    seg1 = torch.from_numpy(np.concatenate([[0, 0], seg[2:] - 1])).to(dev)       # the single record of segment 1 left out
    got1 = apply_pairs(d["x"][1:], d["y"][1:], d["v"][1:], seg1, d["row"], d["col"], d["bias"]).cpu().numpy()
    _same(got1, want[1:])
    # an odd record count in the two-records-a-thread form: the last record goes alone
    seg_odd = torch.from_numpy(np.minimum(seg, 4097)).to(dev)
    got_odd = apply_pairs(d["x"][:4097], d["y"][:4097], d["v"][:4097], seg_odd, d["row"], d["col"], d["bias"]).cpu().numpy()
    _same(got_odd, want[:4097])
    # in place
    vv = d["v"].clone()
    assert apply_pairs(d["x"], d["y"], vv, d["seg"], d["row"], d["col"], d["bias"], out=vv) is vv
    _same(vv.cpu().numpy(), want)
    # nothing to do: success, nothing launched, nothing written
    lib = _lib.load()
    assert lib.mst_balance_apply_pairs(None, None, None, 0, None, None, None, 0, None, 0, None, None) == 0
    assert lib.mst_balance_apply_pairs(None, None, None, 0, _lib.ptr(d["seg"]), _lib.ptr(d["row"]), _lib.ptr(d["col"]), 3,
                                       _lib.ptr(d["bias"]), n, None, None) == 0
    empty_i, empty_v = torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.float64, device=dev)
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    assert apply_pairs(empty_i, empty_i, empty_v, zero, zero[:0], zero[:0], d["bias"]).numel() == 0
    assert lib.mst_balance_apply_pairs(_lib.ptr(d["x"]), _lib.ptr(d["y"]), _lib.ptr(d["v"]), -1, _lib.ptr(d["seg"]), _lib.ptr(d["row"]),
                                       _lib.ptr(d["col"]), 3, _lib.ptr(d["bias"]), n, _lib.ptr(vv), None) == _lib.MST_E_ARG
    torch.cuda.synchronize()


# ---- 4. end to end, one sample ----------------------------------------------------------------------------------------------
def _file_rows(path):
    lines = open(path).read().splitlines()
    assert lines[0].startswith("BIN1_CHR")
    return lines[1:]


def _loop_text(tmp_path, name, per_pair):
    """what the command line writes for {(a, b): loops} in pair order"""
    from mustache_amd.mustache import write_loops
    p = str(tmp_path / name)
    first = True
    for (a, b), loops in per_pair:
        if first or loops:
            write_loops(p, a, b, RES, loops, first=first)
            first = False
    return _file_rows(p)


def _numpy_balanced(gb, names):
    """every pair's resident records balanced in NumPy with the device's bias"""
    out = []
    for a, b in names:
        rec = gb.records(a, b)
        x, y, v = (t.cpu().numpy() for t in rec)
        out.append(gr.balanced(gb.bias, gb.offsets[gb.index(a)], gb.offsets[gb.index(b)], x, y, v))
    return out


THREE = [("1", "2"), ("1", "3"), ("2", "3")]


@pytest.fixture(scope="module")
def call_files(tmp_path_factory):
    import diff_trans_reference as dr
    d = tmp_path_factory.mktemp("balance_genome_call")
    rec1, rec2 = dr.synth_pair(180, 140, density=0.6, nloops=6, seed=41)
    s1 = gr.synth_call_genome(tr.synth_trans(180, 140, density=0.6, nloops=6, seed=41), seed=7)
    s2 = gr.synth_call_genome(rec2, seed=8)
    assert np.array_equal(rec1[2], tr.synth_trans(180, 140, density=0.6, nloops=6, seed=41)[2])     # sample 1 of the pair
    return _write(d / "s1.hic", gr.CALL_BINS, *s1), _write(d / "s2.hic", gr.CALL_BINS, *s2)


def test_one_sample_end_to_end(call_files, tmp_path, capsys, monkeypatch):
    import mustache_amd.hicfile as hicfile
    from mustache_amd.balance_genome import genome_bias
    from mustache_amd.mustache import main
    from mustache_amd.trans_genome import call_trans_genome
    f = call_files[0]
    gb = genome_bias(f, RES, method="NEWTON", pixels="all")
    balanced = _numpy_balanced(gb, THREE)
    # the restatement's own job on the balanced values of the one full tile returns loops
    assert len(balanced[0][2]) >= 10000
    assert len(tr.trans_loops(*balanced[0], ST, PT, OCT)) >= 1
    want = call_trans_genome(balanced, OCT, ST, PT)
    assert len(want[0]) >= 1
    expected = _loop_text(tmp_path, "want.tsv", list(zip(THREE, want)))
    reads = []
    real = hicfile.read_intra_packed
    monkeypatch.setattr(hicfile, "read_intra_packed", lambda *a, **k: (reads.append(a[1]), real(*a, **k))[1])
    out = tmp_path / "all.tsv"
    capsys.readouterr()
    main(["-f", f, "-r", "10kb", "--trans-all", "--balance-genome", "NEWTON", "-o", str(out)])
    said = capsys.readouterr().out
    assert "NEWTON balancing of the genome (all pixels):" in said and said.count("balancing of") == 1
    assert _file_rows(out) == expected and len(expected) >= 1
    assert reads == ["1", "2", "3"]                                  # every cis matrix once
    one = tmp_path / "one.tsv"
    main(["-f", f, "-r", "10kb", "-ch", "1", "-ch2", "2", "--balance-genome", "NEWTON", "-o", str(one)])
    assert _file_rows(one) == [r for r in expected if r.split("\t")[0] == "1" and r.split("\t")[3] == "2"]
    assert len(_file_rows(one)) == len(want[0])
    # inter: no cis matrix is read
    del reads[:]
    capsys.readouterr()
    inter = tmp_path / "inter.tsv"
    main(["-f", f, "-r", "10kb", "--trans-all", "--balance-genome", "NEWTON", "--balance-pixels", "inter", "-o", str(inter)])
    assert "balancing of the genome (inter pixels)" in capsys.readouterr().out
    assert reads == [] and os.path.exists(inter)


# ---- 5. end to end, two samples -----------------------------------------------------------------------------------------------
def test_two_samples_end_to_end(call_files, tmp_path, capsys):
    from mustache_amd.balance_genome import genome_bias
    from mustache_amd.diff_mustache import SUFFIX, main
    from mustache_amd.diff_trans_genome import call_diff_trans_genome
    f1, f2 = call_files
    gbs = [genome_bias(f, RES, method="NEWTON", pixels="all") for f in (f1, f2)]
    assert gbs[0].bias.tobytes() != gbs[1].bias.tobytes()                # each sample is balanced on its own
    ok = ~(gbs[0].info["masked"] | gbs[1].info["masked"])
    assert _rel(gbs[0].bias[ok], gbs[1].bias[ok]) > 1e-3
    both = [_numpy_balanced(gb, THREE) for gb in gbs]
    want = call_diff_trans_genome(list(zip(both[0], both[1])), OCT, ST, PT, PT2)
    out = tmp_path / "d"
    capsys.readouterr()
    main(["-f1", f1, "-f2", f2, "-r", "10kb", "--trans-all", "--balance-genome", "NEWTON", "-o", str(out)])
    said = capsys.readouterr().out
    assert said.count("NEWTON balancing of the genome (all pixels):") == 2      # one line per sample
    total = 0
    for tag, suf in SUFFIX.items():
        rows = [(a, b, r) for (a, b), pr in zip(THREE, want) for r in pr if r[4] == tag]
        lines = ["%s\t%d\t%d\t%s\t%d\t%d\t%r\t%r" % (a, int(r[0]) * RES, (int(r[0]) + 1) * RES, b, int(r[1]) * RES,
                                                     (int(r[1]) + 1) * RES, float(r[2]), float(r[3])) for a, b, r in rows]
        assert _file_rows(str(out) + suf) == lines, suf
        total += len(lines)
    assert total >= 1
    pair = tmp_path / "p"
    main(["-f1", f1, "-f2", f2, "-r", "10kb", "-ch", "1", "-ch2", "2", "--balance-genome", "NEWTON", "-o", str(pair)])
    for suf in SUFFIX.values():
        assert _file_rows(str(pair) + suf) == [r for r in _file_rows(str(out) + suf) if r.split("\t")[3] == "2"
                                               and r.split("\t")[0] == "1"]


# ---- 6. the memory refusal ----------------------------------------------------------------------------------------------------
def test_memory_refusal(genome, tmp_path, capsys, monkeypatch):
    import torch
    from mustache_amd.balance_genome import estimate_bytes
    from mustache_amd.diff_mustache import SUFFIX
    from mustache_amd.diff_mustache import main as diff_main
    from mustache_amd.mustache import main
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (100000, 1 << 30))
    out = tmp_path / "o.tsv"
    capsys.readouterr()
    main(["-f", genome["v8"], "-r", "10kb", "--trans-all", "--balance-genome", "NEWTON", "-o", str(out)])
    said = capsys.readouterr().out
    line = [ln for ln in said.splitlines() if ln.startswith("Error:")]
    assert len(line) == 1 and "100000 bytes are free" in line[0], said
    # the first matrix read is chromosome 1's own: its pixels at distance >= 2 alone exceed the 100 000 bytes
    i, j, _ = genome["cis"][0]
    assert "needs about %d bytes" % estimate_bytes(int((j - i >= 2).sum())) in line[0]
    assert not out.exists()
    main(["-f", genome["v8"], "-r", "10kb", "-ch", "1", "-ch2", "2", "--balance-genome", "ICE", "-o", str(out)])
    assert "100000 bytes are free" in capsys.readouterr().out and not out.exists()
    diff_main(["-f1", genome["v8"], "-f2", genome["v8"], "-r", "10kb", "--trans-all", "--balance-genome", "NEWTON", "-o", str(out)])
    assert "100000 bytes are free" in capsys.readouterr().out
    assert not any(os.path.exists(str(out) + suf) for suf in SUFFIX.values())
