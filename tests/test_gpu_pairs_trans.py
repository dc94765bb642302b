"""Trans loops from a `.pairs` file on the GPU (--pairs-trans): mst_pairs_bin_trans / mst_pairs_trans_compact /
mst_pairs_trans_decode against the restatement (tests/pairs_trans_reference.py), genome_bias from a pairs file against the same
contacts as a `.hic` file, and both command lines end to end."""
import gzip
import os

import numpy as np
import pytest

import balance_genome_reference as gr
import pairs_trans_reference as ptr
import trans_reference as tr
from hic_trans_writer import write_hic_pairs

pytestmark = pytest.mark.gpu

RES = 10000
OCT = [1.6, 3.2]
ST, PT, PT2 = 0.88, 0.2, 0.1
I32_MIN = -(1 << 31)

# ---- 5. bin + compact + decode against the restatement ----------------------------------------------------------------------
PAIR_BINS = [(5, 7), (9, 4), (60, 45), (30, 20)]            # (n_a, n_b) of four pairs: n_a != n_b everywhere
PAIR_ROWS = [0, 1, 4097, 700]                               # 4097 rows: more than a workgroup's 2048, the cut at row 4098 inside a wave
CELLS = [a * b for a, b in PAIR_BINS]
ALL_CELLS = sum(CELLS)
INSIDE_PAIR_2 = CELLS[0] + CELLS[1] + 1000                  # a dense_cells value that falls inside pair 2


def _tables(res):
    """limits = n * res - 1 (a last bin one position short), as a chromosome's length seldom is a multiple of res"""
    t = np.zeros((5, 4), np.int64)
    off = 0
    for p, (na, nb) in enumerate(PAIR_BINS):
        t[:, p] = (na * res - 1, nb * res - 1, na, nb, off)
        off += na * nb
    return t


def _case_rows(res, zero_based, seed=3):
    """pair-major rows: random in-range positions (many non-adjacent duplicates: 4097 rows on 2700 cells), a run of 130 identical
    rows at rows 51 .. 180 of the whole array (it crosses the lane 63 / lane 0 boundary at rows 64 and 128), rows out of range
    on each side alone and on both, INT32_MIN, the edges of both ranges"""
    rng = np.random.default_rng(seed)
    lo = 0 if zero_based else 1
    pa, pb = [], []
    for p, ((na, nb), rows) in enumerate(zip(PAIR_BINS, PAIR_ROWS)):
        la, lb = na * res - 1, nb * res - 1
        hi_a, hi_b = (la - 1, lb - 1) if zero_based else (la, lb)
        a = rng.integers(lo, hi_a + 1, rows)
        b = rng.integers(lo, hi_b + 1, rows)
        if p == 2:
            a[50:180], b[50:180] = 17 * res + lo, 3 * res + lo                    # rows 51 .. 180 of the whole array
            a[200:203], b[200:203] = [hi_a + 1, lo, hi_a + 1], [lo, hi_b + 1, hi_b + 1]     # a side only, b side only, both
            a[300:304], b[300:304] = [lo - 1, lo, I32_MIN, lo], [lo, lo - 1, lo, I32_MIN]
            a[400:402], b[400:402] = [lo, hi_a], [lo, hi_b]                         # the edges: kept
            a[2040:2056], b[2040:2056] = 5 * res + lo, 43 * res + lo                # a run across the workgroups' cut at row 2048
        if p == 3:
            a[0:3], b[0:3] = [hi_a + 1, lo, lo], [lo, hi_b + 1, lo]
            a[690:700], b[690:700] = 28 * res + lo, 18 * res + lo                   # the last rows of the array: one run
        pa.append(a)
        pb.append(b)
    seg = np.concatenate([[0], np.cumsum(PAIR_ROWS)]).astype(np.int64)
    return np.concatenate(pa).astype(np.int32), np.concatenate(pb).astype(np.int32), seg


def _want(pa, pb, seg, tables, res, zero_based):
    pix, dropped = {}, []
    for p in range(tables.shape[1]):
        s, e = int(seg[p]), int(seg[p + 1])
        px, d = ptr.pair_pixels(pa[s:e], pb[s:e], res, zero_based, *(int(v) for v in tables[:4, p]))
        dropped.append(d)
        if px:
            pix[p] = px
    return pix, dropped


def _got(pa, pb, seg, tables, res, zero_based, dense_cells, **kw):
    from mustache_amd.pairs import bin_trans_keys, decode_trans_keys
    keys, counts, dropped, far = bin_trans_keys(pa, pb, seg, tables, res, zero_based, dense_cells, **kw)
    k = keys.cpu().numpy()
    assert np.all(np.diff(k) > 0)                                                   # ascending and unique
    rec = decode_trans_keys(keys, counts, tables)
    out = {}
    for p, (x, y, v) in rec.items():
        assert x.dtype.is_floating_point is False and str(v.dtype) == "torch.float64"
        out[p] = ptr.records_to_pixels(x.cpu().numpy(), y.cpu().numpy(), v.cpu().numpy())
        kk = tables[4, p] + x.cpu().numpy().astype(np.int64) * tables[3, p] + y.cpu().numpy()
        assert np.all(np.diff(kk) > 0)                                              # key order within the pair
    return out, dropped.tolist(), far, (k, counts.cpu().numpy())


@pytest.mark.parametrize("res", [1, 5000])
@pytest.mark.parametrize("zero_based", [False, True])
def test_bin_compact_decode_match_the_restatement(res, zero_based):
    tables = _tables(res)
    pa, pb, seg = _case_rows(res, zero_based)
    want, want_dropped = _want(pa, pb, seg, tables, res, zero_based)
    assert want_dropped == [0, 0, 7, 2] and sorted(want) == [1, 2, 3] and want[2][(17, 3)] >= 130 and want[3][(28, 18)] >= 10
    assert sum(sum(px.values()) for px in want.values()) == sum(PAIR_ROWS) - 9
    rng = np.random.default_rng(9)
    shuffled = np.concatenate([seg[p] + rng.permutation(PAIR_ROWS[p]) for p in range(4)]).astype(np.int64)
    first = None
    for dense_cells in (0, INSIDE_PAIR_2, ALL_CELLS):
        got, dropped, far, raw = _got(pa, pb, seg, tables, res, zero_based, dense_cells)
        assert got == want and dropped == want_dropped, dense_cells
        assert (far == 0) == (dense_cells == ALL_CELLS)
        if dense_cells == 0:
            assert len(raw[0]) < far < sum(PAIR_ROWS) - 9                           # runs were merged, duplicates remained
        again, dropped2, _, raw2 = _got(pa[shuffled], pb[shuffled], seg, tables, res, zero_based, dense_cells)
        assert again == want and dropped2 == want_dropped
        assert np.array_equal(raw[0], raw2[0]) and np.array_equal(raw[1], raw2[1])
        if first is None:
            first = raw
        assert np.array_equal(raw[0], first[0]) and np.array_equal(raw[1], first[1])     # the same records whatever is dense


def test_a_second_trip():
    """2048 workgroups of 2048 rows are the grid's cap: row 2048 * 2048 is the first row of workgroup 0's second trip, on the
    other parity of the LDS slots.  The array is no multiple of 2048 long, the middle pair is empty, the last one starts at lane 5
    of the second trip's first group, a run of identical rows crosses the cut between the trips and each trip has rows out of
    range.  Expected values: ptr.pair_keys per pair."""
    res, cut = 5000, 2048 * 2048
    bins, rows = [(60, 45), (30, 20), (9, 4)], [cut + 5, 0, 316]
    tables = np.zeros((5, 3), np.int64)
    for p, (na, nb) in enumerate(bins):
        tables[:, p] = (na * res - 1, nb * res - 1, na, nb, sum(a * b for a, b in bins[:p]))
    cells = sum(a * b for a, b in bins)
    seg = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    rng = np.random.default_rng(23)
    pa, pb = (np.concatenate([rng.integers(1, bins[p][side] * res, rows[p]) for p in range(3)]).astype(np.int32) for side in (0, 1))
    pa[cut - 8:cut + 4], pb[cut - 8:cut + 4] = 41 * res + 7, 12 * res + 9           # twelve rows of one pixel across the cut
    lim_a, lim_b = int(tables[0, 0]), int(tables[1, 0])
    pa[[10, 70000, cut - 9]], pb[[3000, cut - 2048, cut - 100]] = [0, lim_a + 1, I32_MIN], [lim_b + 1, 0, -5]     # the first trip
    pa[cut + 4] = lim_a + 1                                                         # the second trip: pair 0's last row ...
    pa[[cut + 5, cut + 200]], pb[cut + 320] = [int(tables[0, 2]) + 1, 0], I32_MIN   # ... and pair 2's first, last and one between
    want_keys, want_counts, want_dropped = [], [], []
    for p in range(3):
        k, c, d = ptr.pair_keys(pa[seg[p]:seg[p + 1]], pb[seg[p]:seg[p + 1]], res, False, *(int(v) for v in tables[:4, p]))
        want_keys.append(k + tables[4, p])
        want_counts.append(c)
        want_dropped.append(d)
    want_keys, want_counts = np.concatenate(want_keys), np.concatenate(want_counts)
    assert want_dropped == [7, 0, 3] and int(want_counts.sum()) == sum(rows) - 10 and sum(rows) % 2048 == 321
    assert want_counts[list(want_keys).index(41 * 45 + 12)] >= 12
    shuffled = np.concatenate([seg[p] + rng.permutation(rows[p]) for p in range(3)]).astype(np.int64)
    from mustache_amd.pairs import bin_trans_keys
    for dense_cells in (0, cells):
        for order in (slice(None), shuffled):
            keys, counts, dropped, far = bin_trans_keys(pa[order], pb[order], seg, tables, res, False, dense_cells)
            assert np.array_equal(keys.cpu().numpy(), want_keys) and np.array_equal(counts.cpu().numpy(), want_counts)
            assert dropped.tolist() == want_dropped and (far == 0) == (dense_cells == cells)


def test_keys_beyond_32_bits():
    """one pair of 70 000 x 70 000 bins behind another of the same size: cell_off = 4.9e9 > 2^32; positions up to 2^31 - 1 at
    res 30 000 reach bin 71 582, so a bin >= n drops rows as well"""
    n, res = 70000, 30000
    tables = np.array([[1 << 31] * 2, [1 << 31] * 2, [n, n], [n, n], [0, n * n]], np.int64)
    assert tables[4, 1] > 1 << 32
    rng = np.random.default_rng(4)
    rows = 3000
    pa = rng.integers(1, 1 << 31, rows).astype(np.int32)
    pb = rng.integers(1, 1 << 31, rows).astype(np.int32)
    pa[:5], pb[:5] = [(1 << 31) - 1, 1, 69999 * res + 1, 70000 * res + 1, 15 * res + 7], [1, (1 << 31) - 1, 70000 * res, 5, 22 * res + 1]
    pa[10:14], pb[10:14] = 123456789, 987654321                                     # a run, and again further down
    pa[2000], pb[2000] = 123456789, 987654321
    seg = np.array([0, 5, rows], np.int64)                                          # five rows in the first pair
    want, want_dropped = _want(pa, pb, seg, tables, res, False)
    assert want_dropped[1] > 50 and want_dropped[0] == 3 and want[1][(123456788 // res, 987654320 // res)] == 5
    assert want[0] == {(69999, 69999): 1, (15, 22): 1}                              # bins 71 582 and 70 000 are dropped, 69 999 is kept
    got, dropped, far, raw = _got(pa, pb, seg, tables, res, False, 0)
    assert got == want and dropped == want_dropped
    assert raw[0].max() > 1 << 32 and max(x for x, _ in got[1]) > 60000


def test_the_far_list_is_never_overrun_and_empty_inputs():
    import torch
    from mustache_amd import _lib
    lib = _lib.require_gpu()
    res, tables = 5000, _tables(5000)
    pa, pb, seg = _case_rows(res, False)
    N, P, cap, guard = len(pa), 4, 100, 4096
    dev = torch.device("cuda")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dpa, dpb, dseg, t = d(pa), d(pb), d(seg), d(tables)
    far_key = torch.full((cap + guard,), -7, dtype=torch.int64, device=dev)
    far_mult = torch.full((cap + guard,), -7, dtype=torch.int32, device=dev)
    counters = torch.zeros(P + 1, dtype=torch.int64, device=dev)
    p = _lib.ptr

    def call(n_rows, n_pairs, far_cap):
        return lib.mst_pairs_bin_trans(p(dpa), p(dpb), n_rows, p(dseg), n_pairs, p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), res, 0,
                                       0, None, p(far_key), p(far_mult), far_cap, p(counters[P:]), p(counters), None)
    assert call(N, P, cap) == _lib.MST_OK
    torch.cuda.synchronize()
    c = counters.cpu().tolist()
    assert c[P] > cap and c[:P] == [0, 0, 7, 2]                                     # the loss is reported, the drops still counted
    assert bool((far_key[cap:] == -7).all()) and bool((far_mult[cap:] == -7).all())     # the guard region is untouched
    assert bool((far_key[:cap] >= 0).all()) and bool((far_mult[:cap] >= 1).all())
    with pytest.raises(_lib.MstOverflow):
        from mustache_amd.pairs import bin_trans_keys
        bin_trans_keys(pa, pb, seg, tables, res, False, 0, far_capacity=cap)
    counters.zero_()
    assert call(0, P, cap) == _lib.MST_OK and call(N, 0, cap) == _lib.MST_OK and call(0, 0, 0) == _lib.MST_OK
    assert call(-1, P, cap) == _lib.MST_E_ARG and call(N, -1, cap) == _lib.MST_E_ARG and call(N, P, -1) == _lib.MST_E_ARG
    torch.cuda.synchronize()
    assert counters.cpu().tolist() == [0] * (P + 1)
    from mustache_amd.pairs import bin_trans_device
    assert bin_trans_device(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(4, np.int64), [100, 200, 300], 10) == {}


# ---- 6. the compaction alone -------------------------------------------------------------------------------------------------
def test_compact_alone():
    import torch
    from mustache_amd import _lib
    lib = _lib.require_gpu()
    dev = torch.device("cuda")
    cells = 5000
    dense = np.zeros(cells, np.uint32)
    at = [0, 2047, 2048, 3000, 3001, cells - 1]
    dense[at] = [3, 1, (1 << 32) - 1, 7, 8, 2]
    dd = torch.from_numpy(dense.view(np.int32)).to(dev)
    ws = torch.empty(int(lib.mst_pairs_trans_compact_workspace_bytes(cells)), dtype=torch.uint8, device=dev)
    for cap in (len(at), 4, 0):
        guard = 64
        key = torch.full((cap + guard,), -7, dtype=torch.int64, device=dev)
        cnt = torch.full((cap + guard,), -7, dtype=torch.int32, device=dev)
        found = torch.zeros(1, dtype=torch.int64, device=dev)
        _lib.check(lib.mst_pairs_trans_compact(_lib.ptr(dd), cells, _lib.ptr(key), _lib.ptr(cnt), cap, _lib.ptr(found), _lib.ptr(ws),
                                               ws.numel(), None))
        torch.cuda.synchronize()
        assert int(found.item()) == len(at)                                        # reported even when cap is too small
        assert key[:cap].cpu().tolist() == at[:cap]
        assert (cnt[:cap].cpu().numpy().view(np.uint32)).tolist() == dense[at].tolist()[:cap]      # 2^32 - 1 survives
        assert bool((key[cap:] == -7).all()) and bool((cnt[cap:] == -7).all())
    found = torch.full((1,), 5, dtype=torch.int64, device=dev)
    _lib.check(lib.mst_pairs_trans_compact(None, 0, None, None, 0, _lib.ptr(found), None, 0, None))
    assert int(found.item()) == 0
    assert lib.mst_pairs_trans_compact(_lib.ptr(dd), -1, None, None, 0, _lib.ptr(found), None, 0, None) == _lib.MST_E_ARG
    # the decode: counts above 2^24 and 2^32 reach float64 exactly
    from mustache_amd.pairs import decode_trans_keys
    tables = _tables(1)
    keys = torch.tensor([0, 34, 35, ALL_CELLS - 1], dtype=torch.int64, device=dev)
    counts = torch.tensor([(1 << 24) + 1, (1 << 32) + 3, 1, (1 << 52) + 1], dtype=torch.int64, device=dev)
    rec = decode_trans_keys(keys, counts, tables)
    assert sorted(rec) == [0, 1, 3]
    assert rec[0][0].cpu().tolist() == [0, 4] and rec[0][1].cpu().tolist() == [0, 6] and rec[1][0].cpu().tolist() == [0]
    assert rec[3][0].cpu().tolist() == [29] and rec[3][1].cpu().tolist() == [19]
    assert rec[0][2].cpu().tolist() == [float((1 << 24) + 1), float((1 << 32) + 3)] and rec[3][2].cpu().tolist() == [float((1 << 52) + 1)]


# ---- 7. genome_bias from a pairs file against the same contacts as a .hic ------------------------------------------------------
BINS = (70, 50, 40)
NAMES = ["1", "2", "3"]


def _lengths(bins):
    return [b * RES - 1 for b in bins]                      # those gr.hic_arguments uses


def _write_both(d, tag, bins, cis, trans, seed):
    chroms, mats = gr.hic_arguments(bins, RES, cis, trans)
    hic = str(d / (tag + ".hic"))
    write_hic_pairs(hic, chroms, mats, version=8)
    text, rows = ptr.pairs_text(NAMES, _lengths(bins), RES, cis, trans, seed)
    plain, gz = str(d / (tag + ".pairs")), str(d / (tag + ".pairs.gz"))
    with open(plain, "w") as fh:
        fh.write(text)
    with open(gz, "wb") as fh:
        fh.write(gzip.compress(text.encode(), 1))
    return {"hic": hic, "pairs": plain, "gz": gz, "rows": rows}


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    cis, trans = gr.synth_genome(BINS)
    out = _write_both(tmp_path_factory.mktemp("pairs_trans_genome"), "g", BINS, cis, trans, 5)
    out.update(cis=cis, trans=trans)
    return out


@pytest.mark.parametrize("pixels", ["all", "inter"])
@pytest.mark.parametrize("method", ["NEWTON", "ICE"])
def test_genome_bias_from_pairs_has_the_bits_of_the_hic_run(genome, method, pixels, monkeypatch, capsys):
    from mustache_amd import pairs
    from mustache_amd.balance_genome import genome_bias
    calls = []
    real = pairs.bin_pairs_device
    monkeypatch.setattr(pairs, "bin_pairs_device", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    want = genome_bias(genome["hic"], RES, method=method, pixels=pixels)
    assert calls == []
    before = pairs.PairsFile.OPENS
    got = genome_bias(genome["pairs"], RES, method=method, pixels=pixels, verbose=True)
    said = capsys.readouterr().out
    assert len(calls) == (3 if pixels == "all" else 0)                             # under `inter` no cis row is binned
    assert got.chromosomes == want.chromosomes == NAMES and got.bins == want.bins == list(BINS) and got.offsets == want.offsets
    assert got.bias.tobytes() == want.bias.tobytes() and int(np.isfinite(got.bias).sum()) > 100
    assert got.info["records"] == want.info["records"] > 0 and np.array_equal(got.info["masked"], want.info["masked"])
    assert got.info["pixels"] == pixels and got.info["method"] == method
    for a, b in (("1", "3"), ("3", "1"), ("2", "3")):
        rec, ref = ([t.cpu().numpy() for t in g.records(a, b)] for g in (got, want))
        assert rec[0].dtype == ref[0].dtype == np.int32 and rec[2].dtype == ref[2].dtype == np.float64
        o, q = np.lexsort((rec[1], rec[0])), np.lexsort((ref[1], ref[0]))
        assert all(np.array_equal(r[o], w[q]) for r, w in zip(rec, ref)) and len(o) > 1000
    ex, ey, ec = genome["trans"][(0, 2)]
    x, y, c = (t.cpu().numpy() for t in got.records("1", "3"))                     # key order is (x, y) order
    assert np.array_equal(x, ex) and np.array_equal(y, ey) and np.array_equal(c, ec)
    n_trans = sum(int(v.sum()) for _, _, v in genome["trans"].values())
    assert "pairs g.pairs: %d rows read, %d trans rows (%d stored, 2 naming a chromosome the table lacks, 4 out of range), " \
           "%d trans pixels, 3 pairs with records" % (genome["rows"], n_trans + 6, n_trans + 4,
                                                      sum(len(v) for _, _, v in genome["trans"].values())) in said
    gz = genome_bias(genome["gz"], RES, method=method, pixels=pixels)
    assert gz.bias.tobytes() == want.bias.tobytes()
    assert pairs.PairsFile.OPENS <= before + 2                                     # each file parsed once at the most
    pairs.close_pairs_handles()


# ---- 8 / 9. end to end --------------------------------------------------------------------------------------------------------
THREE = [("1", "2"), ("1", "3"), ("2", "3")]


def _integer(rec):
    x, y, v = rec
    return np.asarray(x), np.asarray(y), np.maximum(np.round(2.0 * np.asarray(v)), 1.0)


@pytest.fixture(scope="module")
def call_files(tmp_path_factory):
    import diff_trans_reference as dr
    d = tmp_path_factory.mktemp("pairs_trans_call")
    s1 = gr.synth_call_genome(_integer(tr.synth_trans(180, 140, density=0.6, nloops=6, seed=41)), seed=7)
    s2 = gr.synth_call_genome(_integer(dr.synth_pair(180, 140, density=0.6, nloops=6, seed=41)[1]), seed=8)
    return {"s1": _write_both(d, "s1", gr.CALL_BINS, *s1, 21), "s2": _write_both(d, "s2", gr.CALL_BINS, *s2, 22), "genomes": (s1, s2)}


def _numpy_balanced_01(genome):
    """the pair (1, 2) of a synthetic genome, balanced by the NumPy restatement alone (NEWTON, all pixels)"""
    cis, trans = genome
    bins, off, _ = gr.layout(_lengths(gr.CALL_BINS), RES)
    bias, _ = gr.genome_bias("NEWTON", bins, off, cis, trans, "all")
    return gr.balanced(bias, off[0], off[1], *trans[(0, 1)])


def _lines(path):
    return open(path).read().splitlines()


def test_one_sample_end_to_end(call_files, tmp_path, capsys):
    from mustache_amd import pairs
    from mustache_amd.mustache import main
    f = call_files["s1"]
    assert 100000 < f["rows"] < 125000
    assert len(tr.trans_loops(*_numpy_balanced_01(call_files["genomes"][0]), ST, PT, OCT)) == 6     # the comparison is not empty
    want = tmp_path / "hic.tsv"
    main(["-f", f["hic"], "-r", "10kb", "--trans-all", "--balance-genome", "NEWTON", "-o", str(want)])
    assert len(_lines(want)) >= 2
    one = tmp_path / "hic_one.tsv"
    main(["-f", f["hic"], "-r", "10kb", "-ch", "1", "-ch2", "2", "--balance-genome", "NEWTON", "-o", str(one)])
    for k, (path, extra) in enumerate(((f["pairs"], ["--trans-all"]), (f["gz"], ["--trans-all"]), (f["pairs"], ["-ch", "1", "-ch2", "2"]),
                                       (f["gz"], ["-ch", "1", "-ch2", "2"]))):
        pairs.close_pairs_handles()
        before = pairs.PairsFile.OPENS
        out = tmp_path / ("p%d.tsv" % k)
        capsys.readouterr()
        main(["-f", path, "--pairs-trans", "--balance-genome", "NEWTON", "-r", "10kb", "-o", str(out)] + extra)
        said = capsys.readouterr().out
        assert "Error" not in said and "NEWTON balancing of the genome (all pixels):" in said and "trans pixels" in said
        assert open(out, "rb").read() == open(want if extra == ["--trans-all"] else one, "rb").read()
        assert pairs.PairsFile.OPENS == before + 1                                 # one parse per run
        assert pairs.pairs_handle(path).keep_trans and pairs.PairsFile.OPENS == before + 1
    assert len(_lines(one)) >= 2
    pairs.WANT_TRANS.clear()
    pairs.close_pairs_handles()


def test_two_samples_end_to_end(call_files, tmp_path, capsys):
    import diff_trans_reference as dr
    from mustache_amd import pairs
    from mustache_amd.diff_mustache import SUFFIX, main
    s1, s2 = call_files["s1"], call_files["s2"]
    rows = dr.diff_trans_rows(_numpy_balanced_01(call_files["genomes"][0]), _numpy_balanced_01(call_files["genomes"][1]), ST, PT, PT2, OCT)
    assert [sum(1 for r in rows if r[4] == t) for t in (1, 2, 3, 4)] == [6, 3, 9, 1]     # the comparison is not empty
    want = tmp_path / "hh"
    main(["-f1", s1["hic"], "-f2", s2["hic"], "-r", "10kb", "--trans-all", "--balance-genome", "NEWTON", "-o", str(want)])
    assert sum(len(_lines(str(want) + suf)) - 1 for suf in SUFFIX.values()) >= 1
    for tag, (f1, f2) in (("pp", (s1["pairs"], s2["pairs"])), ("ph", (s1["pairs"], s2["hic"])), ("hp", (s1["hic"], s2["gz"]))):
        pairs.close_pairs_handles()
        before = pairs.PairsFile.OPENS
        out = tmp_path / tag
        capsys.readouterr()
        main(["-f1", f1, "-f2", f2, "-r", "10kb", "--trans-all", "--pairs-trans", "--balance-genome", "NEWTON", "-o", str(out)])
        said = capsys.readouterr().out
        assert "Error" not in said and said.count("NEWTON balancing of the genome (all pixels):") == 2
        for suf in SUFFIX.values():
            assert open(str(out) + suf, "rb").read() == open(str(want) + suf, "rb").read(), (tag, suf)
        assert pairs.PairsFile.OPENS == before + tag.count("p")
    pairs.WANT_TRANS.clear()
    pairs.close_pairs_handles()


# ---- 10. the memory refusal ---------------------------------------------------------------------------------------------------
def test_memory_refusal(genome, tmp_path, capsys, monkeypatch):
    import torch
    from mustache_amd import pairs
    from mustache_amd.balance_genome import pairs_upload_bytes
    from mustache_amd.mustache import main
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (100000, 1 << 30))
    stored = sum(int(v.sum()) for _, _, v in genome["trans"].values()) + 4
    cells = 70 * 50 + 70 * 40 + 50 * 40
    need = pairs_upload_bytes(stored, cells, 25000)
    assert need == 20 * stored > 100000                                            # 4 bytes per cell do not fit a quarter of 100 000
    out = tmp_path / "o.tsv"
    for extra in (["--trans-all"], ["-ch", "1", "-ch2", "2", "--balance-pixels", "inter"]):
        capsys.readouterr()
        main(["-f", genome["pairs"], "-r", "10kb", "--pairs-trans", "--balance-genome", "NEWTON", "-o", str(out)] + extra)
        line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Error:")]
        assert len(line) == 1 and "needs about %d bytes" % need in line[0] and "100000 bytes are free" in line[0], line
        assert not out.exists()
    pairs.WANT_TRANS.clear()
    pairs.close_pairs_handles()
