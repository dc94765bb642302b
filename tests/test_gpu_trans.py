"""Inter-chromosomal pairs on the MI355X (mustache_amd/trans.py): the device z-score, the loops of every tile against the NumPy
restatement (tests/trans_reference.py) run on the device-normalised values, the `.hic` trans read for both stored orders, and
the command line end to end."""
import numpy as np
import pytest

import trans_reference as tr
from hic_trans_writer import expected_trans, write_hic_pairs

pytestmark = pytest.mark.gpu


def test_device_zscore_matches_numpy_and_ignores_record_order():
    from mustache_amd.trans import zscore_device
    rng = np.random.default_rng(7)
    v = np.exp(rng.normal(0.0, 1.5, 200003)) * 10.0
    z, mean, std, n = zscore_device(v)
    zr, mr, sr = tr.zscore(v)
    assert n == v.size
    assert abs(mean - mr) <= 1e-12 * abs(mr) and abs(std - sr) <= 1e-12 * sr
    np.testing.assert_allclose(z.cpu().numpy(), zr, rtol=0, atol=1e-12)
    perm = rng.permutation(v.size)
    z2, mean2, std2, _ = zscore_device(v[perm])
    assert mean2 == mean and std2 == std
    assert np.array_equal(z2.cpu().numpy(), z.cpu().numpy()[perm])
    _, m0, s0, _ = zscore_device(np.full(10, 4.0))            # std = 0: the caller's "no loops" case
    assert m0 == 4.0 and s0 == 0.0


def _compare(got, ref):
    assert len(ref) > 0, "the case should produce loops"
    assert [(int(a), int(b)) for a, b, _, _ in got] == [(int(a), int(b)) for a, b, _, _ in ref]
    assert [float(s) for _, _, _, s in got] == [float(s) for _, _, _, s in ref]
    for g, r in zip(got, ref):
        assert abs(float(g[2]) - float(r[2])) <= 1e-9, (g, r)


@pytest.mark.parametrize("case", [
    dict(n1=420, n2=300, chunk=2000, oct=[1.6, 3.2], seed=1),        # one tile of 420, padded in y
    dict(n1=900, n2=1200, chunk=600, oct=[1.6, 3.2], seed=2),        # 2 x 3 tiles, ragged last tiles on both axes
    dict(n1=330, n2=360, chunk=2000, oct=[1.6, 3.2, 6.4], seed=3),   # -oc 3
    dict(n1=300, n2=340, chunk=2000, oct=[2.0, 4.0], seed=4),        # -sz 2.0
])
def test_tile_loops_match_the_restatement(case):
    from mustache_amd.trans import call_trans_coo, zscore_device
    x, y, v = tr.synth_trans(case["n1"], case["n2"], density=0.3, nloops=10, seed=case["seed"])
    vz = zscore_device(v)[0].cpu().numpy()
    ref = tr.trans_loops_normalized(x, y, vz, 0.88, 0.2, case["oct"], chunk=case["chunk"])
    got = call_trans_coo(x, y, v, case["oct"], 0.88, 0.2, chunk=case["chunk"], tiles_per_launch=4)
    _compare(got, ref)
    # the record order does not matter (z-score bit-identical, scatter order free)
    perm = np.random.default_rng(0).permutation(len(v))
    again = call_trans_coo(x[perm], y[perm], v[perm], case["oct"], 0.88, 0.2, chunk=case["chunk"])
    assert [[int(a), int(b), float(q), float(s)] for a, b, q, s in again] == [[int(a), int(b), float(q), float(s)] for a, b, q, s in got]


def _norm_vec(n, rng):
    return rng.choice([0.5, 1.0, 1.25, 2.0, np.nan], size=n, p=[0.3, 0.3, 0.2, 0.15, 0.05])   # float32-exact, some NaN bins


def _pair_records(n1, n2, rng, k):
    flat = rng.choice(n1 * n2, size=k, replace=False)
    return flat // n2, flat % n2, rng.integers(1, 200, size=k).astype(np.float64)


@pytest.mark.parametrize("version,dense", [(8, False), (8, True), (9, False)])
@pytest.mark.parametrize("norm", ["KR", "NONE"])
def test_hic_trans_read_matches_a_numpy_reading(tmp_path, version, dense, norm):
    from mustache_amd.trans import read_hic_trans
    rng = np.random.default_rng(11)
    res = 10000
    chroms = [("All", 1000), ("1", 150 * res), ("2", 110 * res), ("3", 90 * res)]
    n = {1: 150, 2: 110, 3: 90}
    recs = {(1, 2): _pair_records(150, 110, rng, 3000), (1, 3): _pair_records(150, 90, rng, 2500),
            (2, 3): _pair_records(110, 90, rng, 2000)}
    norms = {i: _norm_vec(n[i], rng) for i in (1, 2, 3)}
    path = str(tmp_path / ("t%d.hic" % version))
    write_hic_pairs(path, chroms, {k: {res: r} for k, r in recs.items()},
                    norms={("KR", i, res): norms[i] for i in (1, 2, 3)}, version=version, dense_blocks=dense, block_bin_count=32)
    for a, b in ((1, 2), (2, 1), (3, 1), (2, 3), (3, 2)):
        lo, hi = min(a, b), max(a, b)
        xs, ys, cs = recs[(lo, hi)]
        if a > b:
            xs, ys = ys, xs                                      # stored as (b, a): the read transposes
        ex, ey, ec = expected_trans(xs, ys, cs, norms[a] if norm == "KR" else None, norms[b] if norm == "KR" else None)
        gx, gy, gv = read_hic_trans(path, norm, str(a), str(b), res)
        gx, gy, gv = gx.cpu().numpy().astype(np.int64), gy.cpu().numpy().astype(np.int64), gv.cpu().numpy()
        o = np.lexsort((gy, gx))
        np.testing.assert_array_equal(gx[o], ex)
        np.testing.assert_array_equal(gy[o], ey)
        np.testing.assert_array_equal(gv[o], ec)


def _read_tsv(path):
    with open(path) as fh:
        lines = fh.read().splitlines()
    return lines[0], [ln.split("\t") for ln in lines[1:]]


def _trans_file(path, res=10000):
    """chr1 x chr2 trans records from synth_trans (float32 counts), chr1 intra records, chr2 x chr3 trans records"""
    from mustache_amd.synth import synth_coo
    x12, y12, v12 = tr.synth_trans(400, 300, density=0.3, nloops=10, seed=21)
    x23, y23, v23 = tr.synth_trans(300, 350, density=0.3, nloops=10, seed=22)
    xi, yi, vi = synth_coo(600, 150, depth=300.0, seed=5, nloops=20)
    chroms = [("All", 1000), ("1", 600 * res), ("2", 400 * res), ("3", 350 * res)]
    # the file keys (1, 2) as stored; chr2 x chr3 is written as (2, 3)
    mats = {(1, 1): {res: (xi, yi, vi)}, (1, 2): {res: (y12, x12, v12)}, (2, 3): {res: (x23, y23, v23)}}
    write_hic_pairs(str(path), chroms, mats, version=8)
    return (y12, x12, v12), (x23, y23, v23)


def test_cli_writes_the_restatements_trans_rows(tmp_path):
    from mustache_amd.mustache import main
    from mustache_amd.trans import read_hic_trans, zscore_device
    f = tmp_path / "m.hic"
    _trans_file(f)
    out = tmp_path / "t.tsv"
    main(["-f", str(f), "-ch", "2", "-ch2", "1", "-r", "10kb", "-norm", "NONE", "-o", str(out)])
    header, rows = _read_tsv(out)
    assert header.startswith("BIN1_CHR")
    x, y, v = read_hic_trans(str(f), "NONE", "2", "1", 10000)
    vz = zscore_device(v)[0].cpu().numpy()
    ref = tr.trans_loops_normalized(x.cpu().numpy(), y.cpu().numpy(), vz, 0.88, 0.2, [1.6, 3.2])
    assert len(ref) > 0 and len(rows) == len(ref)
    for r, (a, b, q, s) in zip(rows, ref):
        assert r[0] == "2" and r[3] == "1"
        assert (int(r[1]), int(r[2]), int(r[4]), int(r[5])) == (a * 10000, (a + 1) * 10000, b * 10000, (b + 1) * 10000)
        assert float(r[7]) == float(s) and abs(float(r[6]) - q) <= 1e-9


def test_mixed_run_writes_cis_rows_then_trans_rows(tmp_path):
    from mustache_amd.mustache import main
    f = tmp_path / "m.hic"
    _trans_file(f)
    cis, mixed, trans = tmp_path / "cis.tsv", tmp_path / "mixed.tsv", tmp_path / "trans.tsv"
    main(["-f", str(f), "-ch", "1", "-r", "10kb", "-norm", "NONE", "-o", str(cis)])
    main(["-f", str(f), "-ch", "1", "2", "-ch2", "1", "3", "-r", "10kb", "-norm", "NONE", "-o", str(mixed)])
    main(["-f", str(f), "-ch", "2", "-ch2", "3", "-r", "10kb", "-norm", "NONE", "-o", str(trans)])
    cis_text, mixed_text, trans_text = (p.read_text() for p in (cis, mixed, trans))
    assert len(cis_text.splitlines()) > 1 and len(trans_text.splitlines()) > 1
    assert mixed_text.startswith(cis_text)
    tail = mixed_text[len(cis_text):]
    assert tail == "".join(ln + "\n" for ln in trans_text.splitlines()[1:])
