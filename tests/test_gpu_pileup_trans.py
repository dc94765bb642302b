"""The inter-chromosomal pile-up on the MI355X (mustache_amd/pileup.py, csrc/mst_pileup_trans_batch.hip) against the NumPy
restatement (tests/pileup_trans_reference.py): windows, E, valid flags, aggregates and metrics; bit-identity under permutation
of the records and of the loops; repeated pixels; the edges (no record, no loop, the reduce's chunk edge, row flags beyond
LDS, the window limit); a `--trans` run on a `.hic` file; planted loops."""
import functools
import itertools

import numpy as np
import pytest

import pileup_trans_reference as ptr
import trans_reference as tr
from hic_trans_writer import expected_trans, write_hic_pairs

pytestmark = pytest.mark.gpu

HEADER = "BIN1_CHR\tBIN1_START\tBIN1_END\tBIN2_CHROMOSOME\tBIN2_START\tBIN2_END\tFDR\tDETECTION_SCALE"
STRIP = 64                                                   # half-width of the row strip without a record


def _close(a, b, rel=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(invalid="ignore"):
        ok = both_nan | (a == b) | (np.abs(a - b) <= rel * np.maximum(np.abs(a), np.abs(b)))
    return bool(ok.all())


def _same_bits(a, b):
    a, b = np.atleast_1d(np.ascontiguousarray(a, np.float64)), np.atleast_1d(np.ascontiguousarray(b, np.float64))
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@functools.lru_cache(maxsize=None)
def _records(n1, n2, seed=0, density=0.3):
    """records of an n1 x n2 map at `density`, none in the rows n1 // 2 +- STRIP; 200 pixels occur twice more with other values"""
    rng = np.random.default_rng(seed)
    m = rng.random((n1, n2)) < density
    m[max(0, n1 // 2 - STRIP):n1 // 2 + STRIP + 1] = False
    x, y = np.nonzero(m)
    v = np.exp(rng.normal(0.0, 0.5, x.size))
    again = rng.integers(0, x.size, 400)
    x, y = np.concatenate([x, x[again]]), np.concatenate([y, y[again]])
    v = np.concatenate([v, np.exp(rng.normal(0.0, 0.5, 400))])
    o = rng.permutation(x.size)
    out = x[o].astype(np.int64), y[o].astype(np.int64), v[o]
    for a in out:
        a.setflags(write=False)
    return out


def _loop_list(n1, n2, w, extra, seed=1):
    """the four map corners, (0, 0) a second time ((0, 0) and (0, n2 - 1) share a row), two loops 3 bins apart on both axes, one
    loop whose window holds no record, and `extra` random ones"""
    rng = np.random.default_rng(seed)
    fixed = [(0, 0), (n1 - 1, n2 - 1), (0, n2 - 1), (n1 - 1, 0), (0, 0), (n1 // 5, n2 // 3), (n1 // 5 + 3, n2 // 3 + 3),
             (n1 // 2, n2 // 2)]
    xs = np.concatenate([[f[0] for f in fixed], rng.integers(0, n1, extra)]).astype(np.int64)
    ys = np.concatenate([[f[1] for f in fixed], rng.integers(0, n2, extra)]).astype(np.int64)
    if extra:                                                # two more on one row, away from the corners
        xs[-1], ys[-1] = xs[-2], (ys[-2] + n2 // 2) % n2
    return xs, ys


def _dev(x, y, v):
    import torch
    return (torch.from_numpy(np.array(x)).to("cuda", dtype=torch.int32),
            torch.from_numpy(np.array(y)).to("cuda", dtype=torch.int32),
            torch.from_numpy(np.array(v)).cuda())


def _check(r, ref, w, q):
    obs = r["obs"].cpu().numpy()
    assert np.array_equal(np.isnan(obs), np.isnan(ref["obs"]))
    assert np.array_equal(obs, ref["obs"], equal_nan=True)
    assert r["expected"] == ref["expected"]
    rows, cols = r["valid"]
    assert np.array_equal(rows.cpu().numpy().astype(bool), ref["valid"][0])
    assert np.array_equal(cols.cpu().numpy().astype(bool), ref["valid"][1])
    oe = r["oe"].cpu().numpy()
    assert np.array_equal(np.isnan(oe), np.isnan(ref["oe"])) and _close(oe, ref["oe"])
    assert np.array_equal(r["count_obs"], ref["count_obs"]) and np.array_equal(r["count_oe"], ref["count_oe"])
    assert _close(r["sum_obs"], ref["sum_obs"]) and _close(r["sum_oe"], ref["sum_oe"])
    assert _close(r["apa"], ref["apa"]) and _close(r["apa_oe"], ref["apa_oe"])
    assert _same_bits(r["center_obs"], ref["center_obs"]) and _close(r["center_oe"], ref["center_oe"])
    assert _close(r["p2ll"], ref["p2ll"])
    for k in ref["metrics"]:
        assert _close(r["metrics"][k], ref["metrics"][k]), (k, r["metrics"][k], ref["metrics"][k])
        assert _close(r["metrics_oe"][k], ref["metrics_oe"][k]), k


@pytest.mark.parametrize("w,q", [(0, 1), (5, 3), (10, 6), (64, 6)])
@pytest.mark.parametrize("n1,n2", [(300, 180), (180, 300), (4000, 130)])
def test_windows_against_the_restatement(n1, n2, w, q):
    from mustache_amd.pileup import pileup_trans_records
    x, y, v = _records(n1, n2)
    if (n1, n2) == (4000, 130):
        assert x.size > 150000                               # several workgroups, more than one grid-stride trip
    xs, ys = _loop_list(n1, n2, w, 0 if w == 64 else 40)
    assert len(xs) == (8 if w == 64 else 48)
    ref = ptr.pileup_trans_records(x, y, v, n1, n2, xs, ys, w, q)
    assert not np.nan_to_num(ref["obs"][7]).any()            # the loop in the strip: no record in its window
    assert np.isnan(ref["obs"][:4]).any() == (w > 0) and ref["expected"] > 0
    r = pileup_trans_records(*_dev(x, y, v), n1, n2, xs, ys, w, q)
    _check(r, ref, w, q)
    assert _same_bits(r["obs"][0].cpu().numpy(), r["obs"][4].cpu().numpy())      # the loop listed twice


def test_bit_identical_under_permutation_and_from_run_to_run():
    from mustache_amd.pileup import pileup_trans_records
    n1, n2, w, q = 4000, 130, 10, 6
    x, y, v = _records(n1, n2)
    xs, ys = _loop_list(n1, n2, w, 600)                      # two chunks of the reduce
    a = pileup_trans_records(*_dev(x, y, v), n1, n2, xs, ys, w, q)
    b = pileup_trans_records(*_dev(x, y, v), n1, n2, xs, ys, w, q)
    rng = np.random.default_rng(5)
    pr_, pl_ = rng.permutation(x.size), rng.permutation(xs.size)
    c = pileup_trans_records(*_dev(x[pr_], y[pr_], v[pr_]), n1, n2, xs[pl_], ys[pl_], w, q)
    for k in ("sum_obs", "count_obs", "sum_oe", "count_oe", "apa", "apa_oe"):
        assert _same_bits(a[k], b[k]) and _same_bits(a[k], c[k]), k
    for k in ("center_obs", "center_oe", "p2ll"):
        assert _same_bits(a[k], b[k]) and _same_bits(a[k][pl_], c[k]), k
    for k in ("obs", "oe"):
        ak = a[k].cpu().numpy()
        assert _same_bits(ak, b[k].cpu().numpy()) and _same_bits(ak[pl_], c[k].cpu().numpy()), k
    assert a["expected"] == b["expected"] == c["expected"]
    for i in (0, 1):
        assert np.array_equal(a["valid"][i].cpu().numpy(), c["valid"][i].cpu().numpy())
    for k in a["metrics"]:
        assert _same_bits(a["metrics"][k], c["metrics"][k]) and _same_bits(a["metrics_oe"][k], c["metrics_oe"][k]), k


def test_a_repeated_pixel_takes_its_largest_value_in_every_order():
    from mustache_amd.pileup import pileup_trans_records
    base = (np.array([2, 9, 9]), np.array([3, 3, 11]), np.array([0.5, 1.5, 2.5]))
    for vals in itertools.permutations([0.75, 6.0, 3.25]):
        x = np.concatenate([base[0], [5, 5, 5]])
        y = np.concatenate([base[1], [7, 7, 7]])
        v = np.concatenate([base[2], vals])
        r = pileup_trans_records(*_dev(x, y, v), 10, 12, [5, 4], [7, 6], 1, 1)
        obs = r["obs"].cpu().numpy()
        assert obs[0, 1, 1] == 6.0 and obs[1, 2, 2] == 6.0
        assert r["expected"] == (0.5 + 1.5 + 2.5 + 10.0) / 9.0          # every record counts in E: 3 rows x 3 columns


def test_no_record_and_no_loop():
    from mustache_amd.pileup import pileup_trans_records
    e = np.zeros(0, np.int64)
    r = pileup_trans_records(e, e, np.zeros(0), 50, 40, [0, 25], [0, 20], 2, 2)             # N = 0
    obs = r["obs"].cpu().numpy()
    assert r["expected"] == 0.0 and np.isnan(r["oe"].cpu().numpy()).all()
    assert np.isnan(obs[0][:2]).all() and np.isnan(obs[0][:, :2]).all() and not obs[0][2:, 2:].any() and not obs[1].any()
    assert not r["valid"][0].any().item() and not r["valid"][1].any().item()
    assert np.array_equal(r["count_obs"][2:, 2:], np.full((3, 3), 2.0)) and not r["count_oe"].any()
    x, y, v = _records(300, 180)
    r = pileup_trans_records(*_dev(x, y, v), 300, 180, [], [], 10, 6)                       # L = 0: flags and E all the same
    ref = ptr.pileup_trans_records(x, y, v, 300, 180, [], [], 10, 6)
    assert r["expected"] == ref["expected"] > 0
    assert np.array_equal(r["valid"][0].cpu().numpy().astype(bool), ref["valid"][0])
    assert np.array_equal(r["valid"][1].cpu().numpy().astype(bool), ref["valid"][1])
    assert not r["count_obs"].any() and np.isnan(r["apa"]).all() and len(r["p2ll"]) == 0


@pytest.mark.parametrize("L", [1, 513])
def test_the_reduces_chunk_edge(L):
    from mustache_amd.pileup import pileup_trans_records
    n1, n2, w, q = 300, 180, 10, 6
    x, y, v = _records(n1, n2)
    xs, ys = _loop_list(n1, n2, w, 505)
    xs, ys = xs[-L:], ys[-L:]
    r = pileup_trans_records(*_dev(x, y, v), n1, n2, xs, ys, w, q)
    ref = ptr.pileup_trans_records(x, y, v, n1, n2, xs, ys, w, q)
    for k in ("obs", "oe"):
        assert np.array_equal(np.isnan(r[k].cpu().numpy()), np.isnan(ref[k]))
    assert np.array_equal(r["obs"].cpu().numpy(), ref["obs"], equal_nan=True)
    assert np.array_equal(r["count_obs"], ref["count_obs"]) and _close(r["sum_obs"], ref["sum_obs"])
    assert _close(r["sum_oe"], ref["sum_oe"]) and _close(r["p2ll"], ref["p2ll"])


def test_row_flags_beyond_the_lds_switch_point():
    """n1 = 140 000 > 131 072 rows: the record pass reads its row bits from global memory"""
    from mustache_amd.pileup import pileup_trans_records
    n1, n2, w, q = 140000, 50, 5, 3
    rng = np.random.default_rng(9)
    xs = np.array([0, 70, 131070, 131075, 139999, 139999, 65536], np.int64)
    ys = np.array([0, 10, 25, 28, 49, 0, 20], np.int64)
    near = np.repeat(np.arange(len(xs)), 40)
    x = np.clip(xs[near] + rng.integers(-7, 8, near.size), 0, n1 - 1)
    y = np.clip(ys[near] + rng.integers(-7, 8, near.size), 0, n2 - 1)
    x = np.concatenate([x, rng.integers(0, n1, 300), [n1 - 1]])
    y = np.concatenate([y, rng.integers(0, n2, 300), [n2 - 1]])
    v = np.exp(rng.normal(0.0, 0.5, x.size))
    ref = ptr.pileup_trans_records(x, y, v, n1, n2, xs, ys, w, q)
    assert np.nansum(ref["obs"], (1, 2)).all()               # every window holds records
    _check(pileup_trans_records(*_dev(x, y, v), n1, n2, xs, ys, w, q), ref, w, q)


def test_window_limit():
    from mustache_amd.pileup import PileupError, pileup_trans_records
    x, y, v = _records(300, 180)
    with pytest.raises(PileupError, match="64"):
        pileup_trans_records(x, y, v, 300, 180, [100], [90], w=65)
    with pytest.raises(PileupError, match="corner size"):
        pileup_trans_records(x, y, v, 300, 180, [100], [90], w=10, q=0)


# ---- the command line ------------------------------------------------------------------------------------------------------
def _read_matrix(path):
    return np.array([[float(c) for c in line.split("\t")] for line in open(path).read().splitlines()])


def test_cli_trans_on_a_hic_file(tmp_path):
    from mustache_amd.pileup import main
    res, w, q = 10000, 4, 2
    rng = np.random.default_rng(31)
    n = {1: 150, 2: 110, 3: 90}
    chroms = [("All", 1000), ("1", n[1] * res), ("2", n[2] * res), ("3", n[3] * res)]

    def pair(na, nb, k):
        flat = rng.choice(na * nb, size=k, replace=False)
        return flat // nb, flat % nb, rng.integers(1, 200, size=k).astype(np.float64)
    stored = {(1, 2): pair(n[1], n[2], 5000), (2, 3): pair(n[2], n[3], 3000)}          # the file has no (1, 3) matrix
    norms = {i: rng.choice([0.5, 1.0, 1.25, 2.0, np.nan], size=n[i], p=[0.3, 0.3, 0.2, 0.15, 0.05]) for i in n}
    for i in n:
        norms[i][-1] = 1.0                                   # the last bin of every chromosome keeps its records
    hic = str(tmp_path / "m.hic")
    write_hic_pairs(hic, chroms, {k: {res: r} for k, r in stored.items()}, norms={("KR", i, res): norms[i] for i in n},
                    version=8, block_bin_count=32)

    def records(A, B):
        a, b = int(ptr._key(A)), int(ptr._key(B))
        if (min(a, b), max(a, b)) not in stored:
            return None
        sx, sy, sc = stored[(min(a, b), max(a, b))]
        if a > b:                                            # the list orients the pair (2, 1), the file stores (1, 2)
            sx, sy = sy, sx
        return expected_trans(sx, sy, sc, norms[a], norms[b])

    def row(c1, b1, c2, b2):
        return (c1, b1 * res, (b1 + 1) * res, c2, b2 * res, (b2 + 1) * res)
    rows = [row("2", 30, "1", 70),            # pair {1, 2} as (2, 1): stored swapped in the file
            row("2", 50, "3", 40),            # pair {2, 3} as (2, 3)
            row("chr1", 2, "chr2", 107),      # (1, 2): anchors swapped; its window leaves the map on both axes
            row("2", 10, "2", 60),            # cis
            row("3", 88, "chr2", 1),          # (3, 2): anchors swapped
            row("1", 149, "2", 105),          # written (1, 2), so a = 105 on chr2, b = 149 on chr1
            row("2", 109, "3", 400),          # off the map
            row("1", 10, "3", 10),            # a pair the file does not hold
            row("2", 30, "1", 70)]
    lp = str(tmp_path / "l.tsv")
    with open(lp, "w") as fh:
        fh.write(HEADER + "\n" + "".join("\t".join(str(c) for c in r) + "\t0.01\t1.6\n" for r in rows))
    out = str(tmp_path / "o")
    main(["-f", hic, "-l", lp, "-r", str(res), "-o", out, "--trans", "-w", str(w), "-q", str(q)])
    status, centre, parts, whole = ptr.pileup_trans(rows, records, res, w, q)
    assert status == ["used", "used", "used", "cis", "used", "used", "off_map", "no_pair", "used"]
    assert _close(_read_matrix(out + ".apa.tsv"), whole["apa"]) and _close(_read_matrix(out + ".oe.tsv"), whole["apa_oe"])
    body = [r.split("\t") for r in open(out + ".loops.tsv").read().splitlines()[1:]]
    assert [r[8] for r in body] == status
    assert _close([[float(c) for c in r[9:12]] for r in body], centre)
    assert not np.isnan(centre[[0, 1, 2, 4, 5, 8], 0]).any()
    stats = [r.split("\t") for r in open(out + ".stats.tsv").read().splitlines()[1:]]
    assert [r[:3] for r in stats] == [["2,1", "4", "4"], ["2,3", "3", "2"], ["1,3", "1", "0"], ["all", "9", "6"]]
    from mustache_amd.pileup import METRICS
    for r, (_name, _rows, _used, p) in zip(stats, parts + [("all", 0, 0, whole)]):
        assert _close([float(c) for c in r[3:9]], [p["metrics"][m] for m in METRICS]), r[0]
        assert _close(float(r[9]), p["metrics_oe"]["P2LL"]), r[0]


# ---- planted loops ---------------------------------------------------------------------------------------------------------
def _planted_case():
    n1, n2, k = 600, 500, 40
    rng = np.random.default_rng(3)
    cx, cy = rng.integers(20, n1 - 20, k), rng.integers(20, n2 - 20, k)
    x, y, v = tr.synth_trans(n1, n2, density=0.3, nloops=0, seed=12, blobs=[(int(a), int(b), 2.0) for a, b in zip(cx, cy)])
    ux, uy = rng.integers(0, n1, k), rng.integers(0, n2, k)
    return n1, n2, x, y, v, (cx, cy), (ux, uy)


def test_planted_loops_are_enriched():
    from mustache_amd.pileup import pileup_trans_records
    n1, n2, x, y, v, planted, uniform = _planted_case()
    ref_p = ptr.pileup_trans_records(x, y, v, n1, n2, *planted)["metrics"]["P2M"]
    ref_u = ptr.pileup_trans_records(x, y, v, n1, n2, *uniform)["metrics"]["P2M"]
    assert ref_p > 1 and ref_p > ref_u                       # the restatement alone says so
    d = _dev(x, y, v)
    got_p = pileup_trans_records(*d, n1, n2, *planted)
    got_u = pileup_trans_records(*d, n1, n2, *uniform)
    assert got_p["metrics"]["P2M"] > 1 and got_p["metrics"]["P2M"] > got_u["metrics"]["P2M"]
    assert got_p["metrics_oe"]["P2M"] > 1
    assert _close(got_p["metrics"]["P2M"], ref_p) and _close(got_u["metrics"]["P2M"], ref_u)
