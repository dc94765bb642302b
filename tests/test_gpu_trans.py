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


# ---- the production geometry: C = 2000 and several tiles -------------------------------------------------------------------
@pytest.fixture(scope="module")
def production_ahead():
    """the restatement of every production case in worker processes while the device tests run"""
    tr.start_ahead(list(tr.PRODUCTION_CASES))
    yield
    tr.stop_ahead()


def _rows(loops):
    return [[int(a), int(b), float(q), float(s)] for a, b, q, s in loops]


@pytest.mark.parametrize("name", list(tr.PRODUCTION_CASES))
def test_production_tiles_match_the_restatement(name, production_ahead):
    from mustache_amd.mustache import _engine
    from mustache_amd.trans import call_trans_coo, trans_tiling, zscore_device
    case = tr.PRODUCTION_CASES[name]
    x, y, v = tr.production_records(name)
    C, (rs, _), (cs, _) = trans_tiling(case["n1"], case["n2"])
    ntiles = len(rs) * len(cs)
    assert C == 2000 and ntiles >= 4
    # the reference runs on zscore_exact's values: they ARE the device-normalised values, bit for bit
    vz = zscore_device(v)[0].cpu().numpy()
    assert np.array_equal(vz.view(np.uint64), tr.zscore_exact(v)[0].view(np.uint64))
    got = call_trans_coo(x, y, v, case["oct"], 0.88, 0.2)                       # chunk = 2000, the default grouping
    ref = tr.production_reference(name)
    tr.assert_production_conditions(name, ref)
    print("%s: %d tiles, %d records, %d loops (overlap / inner: %r)" % (name, ntiles, len(v), len(ref),
                                                                        tr.loop_geometry(ref, case["n1"], case["n2"])))
    _compare(got, ref)
    # bit-identical under the launch grouping (one tile per launch, a ragged last group, more than there are tiles) ...
    for tpl in (1, ntiles - 1, ntiles + 3):
        assert _rows(call_trans_coo(x, y, v, case["oct"], 0.88, 0.2, tiles_per_launch=tpl)) == _rows(got), tpl
    # ... under a permutation of the records ...
    perm = np.random.default_rng(1).permutation(len(v))
    assert _rows(call_trans_coo(x[perm], y[perm], v[perm], case["oct"], 0.88, 0.2)) == _rows(got)
    # ... and after a record-capacity overflow of the trans launch (the engine grows the buffer and runs again)
    eng = _engine(case["oct"])
    eng._found_cap[C] = 32                                     # a sparse tile holds a few hundred records, a dense one 10^5
    try:
        again = call_trans_coo(x, y, v, case["oct"], 0.88, 0.2)
        assert eng._found_cap[C] > 32, "the launch should have overflowed 32 records per tile"
    finally:
        eng._found_cap.clear()
    assert _rows(again) == _rows(got)


# ---- rule 4's thresholds and filters on small crafted maps ----------------------------------------------------------------
def _threshold_map(n1, n2, count, seed, window_cols=None):
    """synth_trans records trimmed (background records left of the last 300 columns only) until the window [0, n1) x
    [0, window_cols) holds exactly `count` records"""
    x, y, v = tr.synth_trans(n1, n2, density=0.12, nloops=8, seed=seed)
    wc = n2 if window_cols is None else window_cols
    inside = y < wc
    free = inside & (y < (n2 - 300 if n2 > 300 else n2)) & (v < 3.0) & ~((x == n1 - 1) & (y == n2 - 1))
    extra = int(inside.sum()) - count
    assert 0 <= extra <= int(free.sum())
    drop = np.random.default_rng(seed + 100).choice(np.nonzero(free)[0], extra, replace=False)
    keep = np.ones(len(v), bool)
    keep[drop] = False
    return x[keep], y[keep], v[keep]


def _device_and_reference(x, y, v, chunk, oct=(1.6, 3.2)):
    from mustache_amd.trans import call_trans_coo, zscore_device
    vz = zscore_device(v)[0].cpu().numpy()
    ref = tr.trans_loops_normalized(x, y, vz, 0.88, 0.2, list(oct), chunk=chunk)
    got = call_trans_coo(x, y, v, list(oct), 0.88, 0.2, chunk=chunk)
    return got, ref, vz


def test_fifty_tested_pixels_threshold():
    rng = np.random.default_rng(6)
    for k in (49, 50, 51):
        flat = rng.choice(60 * 60 - 1, size=k - 1, replace=False)
        x = np.concatenate([flat // 60, [59]])
        y = np.concatenate([flat % 60, [59]])
        v = np.exp(rng.normal(0.0, 0.5, k))
        got, ref, vz = _device_and_reference(x, y, v, 2000)
        assert np.count_nonzero(vz) == k and ref == [] and got == []


@pytest.mark.parametrize("seed", [1, 3])
def test_ten_thousand_tested_pixels_threshold_in_one_tile(seed):
    x, y, v = _threshold_map(300, 300, 10000, seed)
    got, ref, vz = _device_and_reference(x, y, v, 2000)
    assert len(v) == 10000 and np.count_nonzero(vz) == 10000
    _compare(got, ref)                                                     # the 10 000 case yields loops
    x, y, v = _threshold_map(300, 300, 9999, seed)
    got, ref, vz = _device_and_reference(x, y, v, 2000)
    assert len(v) == 9999 and ref == [] and got == []


def test_ten_thousand_tested_pixels_threshold_next_to_a_full_tile():
    """two tiles (columns 0 / 200 of 500, C = 300): the left one holds 9 999 or 10 000 records, the right one 11 330"""
    x, y, v = _threshold_map(300, 500, 9999, 3, window_cols=300)
    assert int((y < 300).sum()) == 9999 and int((y >= 200).sum()) > 10000
    got, ref, _ = _device_and_reference(x, y, v, 300)
    _compare(got, ref)
    assert all(b >= 300 for _, b, _, _ in ref)                             # the neighbour still reports its own
    x, y, v = _threshold_map(300, 500, 10000, 3, window_cols=300)
    got, ref, _ = _device_and_reference(x, y, v, 300)
    _compare(got, ref)
    assert any(b < 300 for _, b, _, _ in ref) and any(b >= 300 for _, b, _, _ in ref)


def test_records_on_the_mean_are_not_tested_pixels():
    """values in 1/64 steps with an exactly representable mean m: the records equal to m have v' == 0.0 and are no records"""
    x, y, v = _threshold_map(300, 300, 10020, 1)
    v = np.maximum(np.round(v * 64.0), 1.0) / 64.0
    n = len(v)
    m = np.round(v.mean() * 64.0) / 64.0
    v[v == m] += 1.0 / 64.0                                                # only the chosen records sit on the mean
    rng = np.random.default_rng(2)
    on_mean = rng.choice(np.nonzero(v < 3.0)[0][:-1], 20, replace=False)
    v[on_mean] = m
    big = int(np.argmax(v))
    v[big] += m * n - float(np.sum(v))                                     # every term a small multiple of 1/64: exact
    assert v[big] > 3.0 and float(np.sum(v)) == m * n
    got, ref, vz = _device_and_reference(x, y, v, 2000)
    assert np.array_equal(np.nonzero(vz == 0.0)[0], np.sort(on_mean)) and np.count_nonzero(vz) == 10000
    _compare(got, ref)                                                     # 10 000 tested pixels: loops
    # one tested record fewer: 9 999 tested pixels among 10 019 records, no loops
    drop = int(np.nonzero((v < 3.0) & (v != m))[0][0])
    keep = np.arange(n) != drop
    x2, y2, v2 = x[keep], y[keep], v[keep].copy()
    big2 = int(np.argmax(v2))
    v2[big2] += m * (n - 1) - float(np.sum(v2))
    assert float(np.sum(v2)) == m * (n - 1)
    got, ref, vz = _device_and_reference(x2, y2, v2, 2000)
    assert np.count_nonzero(vz) == 9999 and len(v2) == 10019 and ref == [] and got == []


def test_blobs_on_a_tile_s_first_row_and_at_the_column_edges():
    """500 x 300, C = 300: row tiles start at 0 and 200.  A blob on map row 200 is on row 0 of the second tile (dropped there
    by x != 0) inside the overlap: the first tile owns and reports it.  Blobs on map row 0, in column 0 and in the last
    column of the same rows (x >> y in the second tile) go through both sides alike."""
    blobs = [(200, 150, 2.0), (0, 80, 2.0), (1, 200, 2.0), (450, 0, 2.0), (450, 299, 2.0), (451, 4, 2.5), (451, 295, 2.5)]
    x, y, v = tr.synth_trans(500, 300, density=0.3, nloops=6, seed=2, blobs=blobs)
    got, ref, _ = _device_and_reference(x, y, v, 300)
    _compare(got, ref)
    assert any(a == 200 and b == 150 for a, b, _, _ in ref)
    assert all(a != 0 and a != 200 or (a, b) == (200, 150) for a, b, _, _ in ref)
    assert any(a > 300 and b > a - 200 for a, b, _, _ in ref) and any(a > 300 and b < a - 200 for a, b, _, _ in ref)


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


def _sorted_read(path, norm, a, b, res, **kw):
    from mustache_amd.trans import read_hic_trans
    gx, gy, gv = read_hic_trans(path, norm, a, b, res, **kw)
    gx, gy, gv = gx.cpu().numpy().astype(np.int64), gy.cpu().numpy().astype(np.int64), gv.cpu().numpy()
    o = np.lexsort((gy, gx))
    return gx[o], gy[o], gv[o]


@pytest.mark.parametrize("version,dense", [(8, False), (8, True), (9, False)])
@pytest.mark.parametrize("norm", ["KR", "NONE"])
def test_hic_trans_read_over_many_slabs(tmp_path, version, dense, norm):
    """40 000 records through 2 slabs of 4096 bytes (the tightest legal setting): more than a hundred slab hand-overs, each
    with its own row directory and capacity, against the NumPy reading and the one-slab read"""
    import ctypes
    from mustache_amd.hicfile import HicFile, HicTransRawStream
    from mustache_amd.trans import read_trans_contacts
    rng = np.random.default_rng(13)
    res = 10000
    chroms = [("All", 1000), ("1", 600 * res), ("2", 500 * res), ("3", 90 * res)]
    recs = _pair_records(600, 500, rng, 40000)
    norms = {1: _norm_vec(600, rng), 2: _norm_vec(500, rng), 3: _norm_vec(90, rng)}
    path = str(tmp_path / ("s%d.hic" % version))
    write_hic_pairs(path, chroms, {(1, 2): {res: recs}, (2, 3): {res: ([], [], [])}},
                    norms={("KR", i, res): norms[i] for i in (1, 2, 3)}, version=version, dense_blocks=dense, block_bin_count=64)
    mem = ctypes.create_string_buffer(2 * 4096 + 16)
    base = (ctypes.addressof(mem) + 15) // 16 * 16
    with HicFile(path) as h:                                               # the host side alone: how many slabs that is
        st = HicTransRawStream(h, "1", "2", res, "NONE", base, 2, 4096)
        slabs = 0
        while True:
            got = st.next(-1)
            if got is False:
                break
            if got:
                assert got[1] + 16 * got[2] <= 4096
                slabs += 1
                st.release(got[0])
        st.close()
    assert slabs > 100
    for a, b in ((1, 2), (2, 1)):
        xs, ys, cs = recs if a < b else (recs[1], recs[0], recs[2])
        ex, ey, ec = expected_trans(xs, ys, cs, norms[a] if norm == "KR" else None, norms[b] if norm == "KR" else None)
        assert len(ec) > 20000
        for kw in (dict(slab_bytes=4096, n_slabs=2), dict(slab_bytes=8192, n_slabs=3), dict()):
            gx, gy, gv = _sorted_read(path, norm, str(a), str(b), res, **kw)
            np.testing.assert_array_equal(gx, ex)
            np.testing.assert_array_equal(gy, ey)
            np.testing.assert_array_equal(gv, ec)
    assert read_trans_contacts(path, norm, "2", "3", res) is None          # a pair without a record
    assert read_trans_contacts(path, norm, "3", "2", res) is None


def test_hic_trans_read_refuses_illegal_slabs_and_rows_longer_than_a_slab(tmp_path):
    from mustache_amd.hicfile import HicError
    from mustache_amd.trans import read_hic_trans
    rng = np.random.default_rng(14)
    res = 10000
    # row y = 5 holds 800 records of 6 bytes in one block: 4800 bytes, more than a slab of 4096
    x = np.concatenate([np.arange(800), rng.integers(0, 1000, 300)])
    y = np.concatenate([np.full(800, 5), rng.integers(6, 400, 300)])
    _, first = np.unique(x * 1000 + y, return_index=True)
    x, y = x[first], y[first]
    c = rng.integers(1, 50, x.size).astype(np.float64)
    path = str(tmp_path / "long.hic")
    write_hic_pairs(path, [("All", 1000), ("1", 1000 * res), ("2", 500 * res)], {(1, 2): {res: (x, y, c)}}, version=8,
                    block_bin_count=1024)
    with pytest.raises(HicError, match="a row holds more records than a slab"):
        read_hic_trans(path, "NONE", "1", "2", res, slab_bytes=4096, n_slabs=2)
    ex, ey, ec = expected_trans(x, y, c)
    gx, gy, gv = _sorted_read(path, "NONE", "1", "2", res, slab_bytes=8192, n_slabs=2)     # the same file with room for the row
    assert np.array_equal(gx, ex) and np.array_equal(gy, ey) and np.array_equal(gv, ec)
    for slab_bytes, n_slabs in ((4080, 2), (4100, 2), (4096, 1)):
        with pytest.raises(HicError, match="bad argument"):
            read_hic_trans(path, "NONE", "1", "2", res, slab_bytes=slab_bytes, n_slabs=n_slabs)


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
