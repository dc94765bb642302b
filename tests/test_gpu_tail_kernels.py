"""Every kernel of mustache_amd/csrc/mst_tail.hip against a plain NumPy / SciPy restatement (tests/tail_reference.py) at its
edges: the window counts where Python's slices wrap and truncate, the diagonal gathers at the fills and past the block, the
exponential fit and the p-values on every branch of the kernel, the packed record arrays at every pitch, the clustering on
long chains, at the largest block the entry point admits, and straight against scipy.ndimage.label."""
import functools

import numpy as np
import pytest

import tail_reference as tr
from test_gpu_cluster import _batch as _record_batch, _case as _clump_case

pytestmark = pytest.mark.gpu
OCT = [1.6, 3.2]
HALFS = (1, 2, 3, 7, 13, 26)
T = 48                                  # MST_MAX_TESTED: the pitch of the statistics and of the fits


# ---- inputs and expectations (host; built once) ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _chrom(n, dpx, depth, seed):
    from mustache_amd.synth import synth_coo
    return synth_coo(n, dpx, depth=depth, seed=seed)


def _frame(CH, width=12):
    """every pixel within `width` of one of the four block edges that can be a candidate (off >= 4)"""
    x, y = np.nonzero(np.ones((CH, CH), dtype=bool))
    edge = np.minimum(np.minimum(x, y), np.minimum(CH - 1 - x, CH - 1 - y)) < width
    return (x * CH + y)[edge & (y - x >= 4)].astype(np.uint32)


def _hand(CH, dpx):
    """candidates placed by hand: on off == 4 (tested, value 2), off == dpx (the last raw value), off == dpx + 1 (tested,
    value 2), off == dpx + 2, the block's corners, and a few in the middle"""
    pts = [(0, 4), (1, 5), (40, 44), (CH - 5, CH - 1), (0, 5), (40, 45), (CH - 6, CH - 1)]
    for off in (dpx - 1, dpx, dpx + 1, dpx + 2):
        pts += [(0, off), (1, off + 1), (33, 33 + off), (CH - 1 - off, CH - 1), (CH - 2 - off, CH - 2)]
    pts += [(0, CH - 1), (CH // 2, CH // 2 + 8), (CH // 2 - 1, CH // 2 + 11), (20, 37), (47, 60), (48, 61)]
    return np.array([x * CH + y for x, y in pts], dtype=np.uint32)


def _with_halfs(pix, halfs):
    """every candidate at every half"""
    return np.tile(pix, len(halfs)), np.repeat(np.asarray(halfs, dtype=np.int64), len(pix))


def _expected(block, pix, half):
    c, nz = block
    c1, c2 = tr.window_counts(nz, pix, half)
    return c1, c2, c.ravel()[pix.astype(np.int64)]


@functools.lru_cache(maxsize=None)
def _small_case(n, seed=21):
    """n = 150: the base case, two blocks of 96 at 0 and 54; n = 70: one block of 96 that reaches past the chromosome end"""
    dpx, CH = 30, 96
    starts = [0, 54] if n == 150 else [0]
    x, y, v = _chrom(n, dpx, 1.5, seed)
    blocks = [tr.block_from_coo(x, y, v, s, CH, dpx, n) for s in starts]
    pix, half = _with_halfs(np.unique(np.concatenate([_frame(CH), _hand(CH, dpx)])), HALFS)
    return dict(n=n, dpx=dpx, CH=CH, starts=starts, coo=(x, y, v), blocks=blocks, pix=pix, half=half,
                exp=[_expected(b, pix, half) for b in blocks])


def edge_classes(CH, pix, half, cnt2):
    """how many (candidate, half) entries sit in each class the window arithmetic treats differently"""
    x, y, s = pix.astype(np.int64) // CH, pix.astype(np.int64) % CH, half
    return {
        "x - s < 0": int(np.sum(x - s < 0)),
        "y - 2s < 0 <= y - s": int(np.sum((y - 2 * s < 0) & (y - s >= 0))),
        "x + 2s + 1 > CH": int(np.sum(x + 2 * s + 1 > CH)),
        "y + s + 1 > CH": int(np.sum(y + s + 1 > CH)),
        "wrapped and non-empty (CH < 4s + 1, x - 2s < 0, cnt2 > 0)": int(np.sum((CH < 4 * s + 1) & (x - 2 * s < 0) & (cnt2 > 0))),
    }


# ---- device plumbing ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _engine():
    from mustache_amd.engine import ScaleSpaceEngine
    return ScaleSpaceEngine(OCT)


def _band(coo, n, dpx):
    import torch
    from mustache_amd.normalize import band_from_coo
    x, y, v = coo
    return band_from_coo(torch.from_numpy(x.astype(np.int64)).cuda(), torch.from_numpy(y.astype(np.int64)).cuda(),
                         torch.from_numpy(v.astype(np.float64)).cuda(), n, dpx)


def _dense_batch(blocks, CH):
    import torch
    from mustache_amd.batches import BlockBatch
    c = torch.from_numpy(np.stack([b[0] for b in blocks])).cuda()
    nz = torch.from_numpy(np.stack([b[1] for b in blocks]).astype(np.uint8)).cuda()
    return BlockBatch(_engine(), c, nz, CH, len(blocks), None, None, None)


def _band_batch(band, n, dpx, starts, CH):
    from mustache_amd.batches import BandBatch
    return BandBatch(_engine(), band, n, dpx, starts, CH, None, None, None)


def _features_band(band, n, dpx, CH, pix, half, start=None, starts=None, pad=4):
    """mst_candidate_features_band (start) or mst_candidate_features_band_multi (starts: one per candidate) called directly;
    the outputs have `pad` more entries than candidates, which must come back untouched"""
    import torch
    from mustache_amd import _lib
    lib, m = _engine().lib, len(pix)
    d_pix = torch.from_numpy(np.ascontiguousarray(pix, dtype=np.uint32).view(np.int32)).cuda()
    d_half = torch.from_numpy(np.ascontiguousarray(half, dtype=np.int32)).cuda()
    cnt = torch.full((2, m + pad), -1, dtype=torch.int32, device="cuda")
    cval = torch.full((m + pad,), -7.0, dtype=torch.float64, device="cuda")
    args = (_lib.ptr(d_pix), _lib.ptr(d_half), m, _lib.ptr(cnt), _lib.off(cnt, m + pad), _lib.ptr(cval), _lib.stream())
    if starts is None:
        _lib.check(lib.mst_candidate_features_band(_lib.ptr(band), n, dpx, int(start), CH, *args))
    else:
        d_s = torch.from_numpy(np.ascontiguousarray(starts, dtype=np.int64)).cuda()
        _lib.check(lib.mst_candidate_features_band_multi(_lib.ptr(band), n, dpx, _lib.ptr(d_s), CH, *args))
    cnt_h, cval_h = cnt.cpu().numpy(), cval.cpu().numpy()
    assert (cnt_h[:, m:] == -1).all() and (cval_h[m:] == -7.0).all(), "entries past the last candidate were written"
    return cnt_h[0, :m].view(np.uint32), cnt_h[1, :m].view(np.uint32), cval_h[:m]


def _same(got, exp, what):
    for g, e, name in zip(got, exp, ("cnt1", "cnt2", "cval")):
        bad = np.nonzero(np.asarray(g) != np.asarray(e))[0]
        assert bad.size == 0, "%s: %s differs at %d entries, first %d: got %r, expected %r" % (what, name, bad.size, bad[0],
                                                                                               g[bad[0]], e[bad[0]])


# ---- window counts and centre values --------------------------------------------------------------------------------------
def test_window_counts_at_the_block_edges_dense_band_and_starts_form():
    """n = 150, dpx = 30, two blocks of 96: the 12-wide frame along all four edges and the hand-placed candidates, each at every
    half of HALFS -- 11 658 entries per block, of which 3428 have x - s < 0 (a wrapped, empty row slice), 520 have
    y - 2s < 0 <= y - s, 770 have x + 2s + 1 > CH, 3427 have y + s + 1 > CH (truncated), and 1389 / 1388 (block 0 / 1) a wrapped
    slice that is NOT empty (half = 26: 4s + 1 = 105 > 96) with a non-zero count."""
    k = _small_case(150)
    n, dpx, CH, pix, half = k["n"], k["dpx"], k["CH"], k["pix"], k["half"]
    for b in range(2):
        nz = k["blocks"][b][1]
        off = np.arange(CH)[None, :] - np.arange(CH)[:, None]
        assert 0.3 < nz[(off >= 4) & (off <= dpx + 1)].mean() < 0.9, "nz neither empty nor full"
        classes = edge_classes(CH, pix, half, k["exp"][b][1])
        print("block %d, %d entries, per class: %r" % (b, len(pix), classes))
        assert all(v >= 20 for name, v in classes.items() if not name.startswith("wrapped")), classes
        assert classes["wrapped and non-empty (CH < 4s + 1, x - 2s < 0, cnt2 > 0)"] >= 1, classes
    px, py = pix.astype(np.int64) // CH, pix.astype(np.int64) % CH
    for off in (4, dpx, dpx + 1):
        assert np.sum(py - px == off) >= 5 * len(HALFS)
    on4 = py - px == 4
    assert (k["exp"][0][2][on4] == 2.0).all() and k["blocks"][0][1][px[on4], py[on4]].any(), "off == 4: tested, value 2"
    band = _band(k["coo"], n, dpx)
    dense, bandb = _dense_batch(k["blocks"], CH), _band_batch(band, n, dpx, k["starts"], CH)
    for b, start in enumerate(k["starts"]):
        _same(dense.candidate_features(b, pix, half), k["exp"][b], "mst_candidate_features, block %d" % b)
        _same(_features_band(band, n, dpx, CH, pix, half, start=start), k["exp"][b], "mst_candidate_features_band, block %d" % b)
        _same(bandb.candidate_features(b, pix, half), k["exp"][b], "BandBatch.candidate_features, block %d" % b)
    # both blocks through the batched forms, the dense one launch per block, the band in one launch with a start per entry
    for batch in (dense, bandb):
        got = batch.candidate_features_multi([1, 0], [pix, pix[:1001]], [half, half[:1001]])
        _same(got[0], k["exp"][1], "multi, block 1")
        _same(got[1], [e[:1001] for e in k["exp"][0]], "multi, block 0")


def test_window_counts_of_a_block_past_the_chromosome_end():
    """n = 70 <= CH = 96 (the tiny-chromosome tiling): columns and rows >= n read nothing from the band, but keep their fills"""
    k = _small_case(70)
    n, dpx, CH, pix, half = k["n"], k["dpx"], k["CH"], k["pix"], k["half"]
    assert np.sum(pix.astype(np.int64) % CH >= n) > 500 and np.sum(pix.astype(np.int64) // CH >= n) > 100
    assert k["blocks"][0][1][:n, :n].any() and not k["blocks"][0][1][:, n:].any()
    band = _band(k["coo"], n, dpx)
    _same(_dense_batch(k["blocks"], CH).candidate_features(0, pix, half), k["exp"][0], "mst_candidate_features")
    _same(_features_band(band, n, dpx, CH, pix, half, start=0), k["exp"][0], "mst_candidate_features_band")
    _same(_band_batch(band, n, dpx, [0], CH).candidate_features(0, pix, half), k["exp"][0], "BandBatch.candidate_features")


def test_window_counts_starts_form_with_interleaved_blocks():
    """mst_candidate_features_band_multi directly: the candidates of both blocks shuffled into one launch, so neighbouring
    waves of a workgroup read different blocks; entry counts that do not fill the last workgroup (4 waves each)"""
    k = _small_case(150)
    n, dpx, CH = k["n"], k["dpx"], k["CH"]
    band = _band(k["coo"], n, dpx)
    rng = np.random.default_rng(8)
    m = len(k["pix"])
    blk = np.tile([0, 1], m)[:2 * m - 1]                            # alternating, an odd number of entries
    idx = np.concatenate([rng.permutation(m), rng.permutation(m)])[:2 * m - 1]
    assert len(blk) % 4 != 0
    for ncand in (len(blk), 1, 3, 4, 5):
        bb, ii = blk[:ncand], idx[:ncand]
        exp = [np.where(bb == 0, k["exp"][0][j][ii], k["exp"][1][j][ii]) for j in range(3)]
        got = _features_band(band, n, dpx, CH, k["pix"][ii], k["half"][ii], starts=np.asarray(k["starts"])[bb])
        _same(got, exp, "mst_candidate_features_band_multi, %d entries" % ncand)


def test_pair_band_batch_runs_alternate_between_two_bands():
    """PairBandBatch with bs = [0, P, 1, P + 1]: every run of _runs is one block, the bands alternate, one block is empty"""
    from mustache_amd.batches import PairBandBatch
    k1, k2 = _small_case(150), _small_case(150, seed=22)
    n, dpx, CH, starts = k1["n"], k1["dpx"], k1["CH"], k1["starts"]
    assert any(not np.array_equal(a[1], b[1]) for a, b in zip(k1["blocks"], k2["blocks"])), "two different maps"
    batch = PairBandBatch(_engine(), [_band(k1["coo"], n, dpx), _band(k2["coo"], n, dpx)], n, dpx, starts, CH, None, None, None)
    rng = np.random.default_rng(9)
    m = len(k1["pix"])
    for bs, sizes, nruns in (([0, 2, 1, 3], [37, 0, 501, 41], 3), ([0, 2, 1, 3], [0, 23, 5, 0], 2),
                             ([3, 0, 2, 1, 0], [9, 1, 3, 4, 5], 4), ([0, 1, 2, 3], [m, m, m, m], 2)):
        pick = [np.sort(rng.choice(m, s, replace=False)) for s in sizes]
        got = batch.candidate_features_multi(bs, [k1["pix"][p] for p in pick], [k1["half"][p] for p in pick])
        assert len(list(batch._runs(bs, sizes))) == nruns
        for b, p, g in zip(bs, pick, got):
            exp = (k1 if b < 2 else k2)["exp"][b % 2]
            _same(g, [e[p] for e in exp], "PairBandBatch block %d of bs = %r" % (b, bs))


@functools.lru_cache(maxsize=None)
def _production_case():
    """the production block shape: n = 4300, dpx = 400 -> three blocks of 2000 at 0, 1600, 2300"""
    import oracle
    from mustache_amd.levels import LevelTable
    n, dpx = 4300, 400
    CH, starts, _ = oracle.block_bounds(n, dpx)
    assert CH == 2000 and starts == [0, 1600, 2300]
    x, y, v = _chrom(n, dpx, 6.0, 23)
    halfs = np.ceil(np.asarray(LevelTable(OCT).tested_sigma)).astype(np.int64)       # s = math.ceil(sigma), mustache.py:802
    rng = np.random.default_rng(10)
    frame = np.concatenate([_frame(CH), _hand(CH, dpx)])
    blocks, pixs, hfs, exps = [], [], [], []
    for s in starts:
        blk = tr.block_from_coo(x, y, v, s, CH, dpx, n)
        found = rng.choice(np.flatnonzero(blk[1].ravel()), 300, replace=False).astype(np.uint32)
        pix = np.concatenate([found, frame])
        half = halfs[np.arange(len(pix)) % len(halfs)]               # every tested level in turn
        blocks.append(blk)
        pixs.append(pix)
        hfs.append(half)
        exps.append(_expected(blk, pix, half))
    return dict(n=n, dpx=dpx, CH=CH, starts=starts, coo=(x, y, v), blocks=blocks, pix=pixs, half=hfs, exp=exps)


def test_window_counts_at_the_production_block_shape():
    k = _production_case()
    n, dpx, CH, starts = k["n"], k["dpx"], k["CH"], k["starts"]
    assert set(np.unique(k["half"][0])) == {2, 3, 4, 5, 6, 7}
    assert all(np.median(e[0][:300]) > 5 and e[1][:300].max() > 200 for e in k["exp"])
    band = _band(k["coo"], n, dpx)
    bs = [0, 1, 2]
    for batch in (_dense_batch(k["blocks"], CH), _band_batch(band, n, dpx, starts, CH)):
        for b, got in zip(bs, batch.candidate_features_multi(bs, k["pix"], k["half"])):
            _same(got, k["exp"][b], "%s, block %d" % (type(batch).__name__, b))


# ---- diagonals ------------------------------------------------------------------------------------------------------------
def _diag_ks(CH, dpx):
    return [-1, 0, 3, 4, 5, dpx - 1, dpx, dpx + 1, dpx + 2, CH - 2, CH - 1, CH, CH + 5]


@pytest.mark.parametrize("case", ["two blocks of 96", "short chromosome", "production shape"])
def test_diagonal_gathers_equal_np_diagonal(case):
    k = {"two blocks of 96": lambda: _small_case(150), "short chromosome": lambda: _small_case(70),
         "production shape": _production_case}[case]()
    n, dpx, CH, starts = k["n"], k["dpx"], k["CH"], k["starts"]
    ks = _diag_ks(CH, dpx)
    assert CH <= 256 or CH > 3 * 256, "one workgroup per diagonal, or several"
    dense, band = _dense_batch(k["blocks"], CH), _band_batch(_band(k["coo"], n, dpx), n, dpx, starts, CH)
    for b in range(len(starts)):
        exp = tr.diagonals(k["blocks"][b][0], ks)
        assert exp[ks.index(dpx)].any() and (exp[ks.index(dpx + 1), :CH - dpx - 1] == 2.0).all() and not exp[ks.index(CH)].any()
        for batch in (dense, band):
            got = batch.diagonals(b, ks)
            assert got.shape == exp.shape and np.array_equal(got, exp), (type(batch).__name__, b,
                                                                          [kk for kk, g, e in zip(ks, got, exp) if not np.array_equal(g, e)])
    # several blocks in one call (one launch per block into one output)
    for batch in (dense, band):
        bs = list(range(len(starts)))[::-1]
        for b, got in zip(bs, batch.diagonals_multi(bs, [ks[b:] for b in bs])):
            assert np.array_equal(got, tr.diagonals(k["blocks"][b][0], ks[b:]))


def test_diagonal_means_with_more_than_64_kb_of_lds():
    """CH = 8200: the compaction buffer is 65 600 bytes, past the 64 KB a kernel gets without asking (the hipFuncSetAttribute
    branch fine resolutions take).  A diagonal of the filled block is the constant 2 for k <= 4 and k >= dpx + 1 and the raw
    band row in between (tests/test_tail_reference.py holds that rule to np.diagonal of the oracle's block)."""
    import torch
    from mustache_amd import _lib
    n = CH = 8200
    dpx = 20
    rng = np.random.default_rng(12)
    band_h = rng.uniform(0.5, 9.0, (dpx + 2, n)) * (rng.random((dpx + 2, n)) < 0.7)
    for d in range(dpx + 2):
        band_h[d, n - d:] = 0.0                                      # pixel (i, i + d) past the chromosome end
    ks = [0, 5, 10, 20, 21, 8199]
    exp = np.array([np.mean(dg[dg != 0]) for dg in
                    (np.full(CH - kk, 2.0) if (kk <= 4 or kk >= dpx + 1) else band_h[kk, :CH - kk] for kk in ks)])
    assert (exp[[0, 4, 5]] == 2.0).all() and len(np.unique(exp)) == 4
    band = torch.from_numpy(band_h).cuda()
    d_k = torch.from_numpy(np.asarray(ks, dtype=np.int32)).cuda()
    out = torch.full((len(ks) + 2,), -7.0, dtype=torch.float64, device="cuda")
    _lib.check(_engine().lib.mst_diag_means_band(_lib.ptr(band), n, dpx, 0, CH, _lib.ptr(d_k), len(ks), _lib.ptr(out), _lib.stream()))
    got = out.cpu().numpy()
    assert np.array_equal(got[:len(ks)], exp), (got, exp)
    assert (got[len(ks):] == -7.0).all()
    # ... and the same numbers through the batch, next to the whole diagonals
    batch = _band_batch(band, n, dpx, [0], CH)
    assert np.array_equal(batch.diagonal_means_multi([0], [ks])[0], exp)
    dg = batch.diagonals(0, ks)
    assert np.array_equal(np.array([np.mean(r[r != 0]) for r in dg]), exp)


def test_diagonal_means_refuse_a_block_that_does_not_fit_the_lds():
    """CH = 20353: 162 824 bytes, 8 more than a workgroup can have.  The call returns before any launch."""
    import torch
    from mustache_amd import _lib
    lib = _engine().lib
    band = torch.zeros((3, 64), dtype=torch.float64, device="cuda")
    d_k = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.full((1,), -7.0, dtype=torch.float64, device="cuda")
    for CH, rc_exp in ((20353, _lib.MST_E_ARG),):
        rc = lib.mst_diag_means_band(_lib.ptr(band), 64, 1, 0, CH, _lib.ptr(d_k), 1, _lib.ptr(out), _lib.stream())
        assert rc == rc_exp
        assert "does not fit the LDS" in lib.mst_last_error().decode()
        rc = lib.mst_diag_means(_lib.ptr(band), CH, 0, _lib.ptr(d_k), 1, _lib.ptr(out), _lib.stream())
        assert rc == rc_exp and "does not fit the LDS" in lib.mst_last_error().decode()
    torch.cuda.synchronize()
    assert float(out.cpu()[0]) == -7.0


# ---- fit and p-values -----------------------------------------------------------------------------------------------------
FOUND_DT = np.dtype([("pixel", "<u4"), ("level", "<u4"), ("value", "<f8")])
X_TARGETS = (-1.0, 0.0, 1e-300, 1e-17, 0.25, 0.5, float(np.nextafter(0.5, 1)), 0.7, 1.0, 10.0, 36.0, 37.0, 40.0, 745.0, 800.0)


def _x_of(value, loc, scale):
    with np.errstate(all="ignore"):
        return (np.abs(value) - loc) / scale


def _land(target, loc, scale):
    """a value whose x = (|v| - loc) / scale is `target` exactly if a double near loc + target * scale gives it, else the
    nearest one"""
    v0 = np.float64(loc + target * scale)
    best = v0
    for steps in (0, 1, -1, 2, -2, 3, -3):
        v = v0
        for _ in range(abs(steps)):
            v = np.nextafter(v, np.inf if steps > 0 else -np.inf)
        if v >= 0 and _x_of(v, loc, scale) == target:
            return v
    return best


@functools.lru_cache(maxsize=None)
def _pvalue_case(B=301, n_tested=48, cap=256, seed=13, special=True, counts=None):
    """statistics, records and SciPy's p-values of B blocks.  special: blocks 2 .. 15 get a degenerate or an exactly
    representable fit; counts: the record counts, random in 0 .. cap when None"""
    rng = np.random.default_rng(seed)
    nzc = rng.integers(1000, 200000, B).astype(np.uint32)
    mn = rng.uniform(1e-6, 0.05, (B, T))
    ratio = np.exp(rng.uniform(np.log(1.05), np.log(40.0), (B, T)))              # mean / min; below 2: loc > scale
    count = rng.integers(0, cap + 1, B).astype(np.uint32)
    count[0], count[-1] = 0, cap
    if counts is not None:
        count[:] = counts
    # blocks with a degenerate or an exactly representable fit
    zero, neg, pow2, wide = (range(2, 5), range(5, 8), range(8, 14), range(14, 16)) if special else ((), (), (), ())
    for b in zero:                                                               # sum / count == min: scale 0
        nzc[b] = 4096
        ratio[b] = 1.0
    for b in neg:                                                                # sum / count < min: negative scale
        ratio[b] = 0.5
    sm = mn * ratio * nzc[:, None]
    for j, b in enumerate(pow2):                                                 # loc = the smallest double, scale = 2^(j-3) exactly
        nzc[b] = 1 << 12
        mn[b] = 5e-324
        sm[b] = 2.0 ** (j - 3) * 4096.0
    for b in wide:                                                               # loc = 3, scale = 2: x = -1 at |v| = 1
        nzc[b] = 4
        mn[b] = 3.0
        sm[b] = 20.0
    for b in list(zero) + list(neg) + list(pow2) + list(wide):
        count[b] = cap
    stats = np.full((B, T, 2), np.nan)
    stats[:, :n_tested, 0] = mn[:, :n_tested]
    stats[:, :n_tested, 1] = sm[:, :n_tested]
    loc, scale = tr.expon_fit(stats[..., 0], stats[..., 1], nzc[:, None])
    if special:
        assert (scale[list(zero), :n_tested] == 0).all() and (scale[list(neg), :n_tested] < 0).all()
        assert (scale[pow2[0], :n_tested] == 0.125).all() and (scale[wide[0], :n_tested] == 2.0).all()
    found = np.zeros((B, cap), dtype=FOUND_DT)
    found["value"] = np.nan
    for b in range(B):
        m = int(count[b])
        lvl = (rng.permutation(max(m, 1)) % n_tested + 1)[:m]                    # every level when m >= n_tested
        lo, sc = loc[b, lvl - 1], scale[b, lvl - 1]
        kind = rng.integers(0, 4, m)
        x = np.where(kind == 0, -rng.uniform(0.0, 2.0, m), np.where(kind == 1, rng.uniform(0.0, 0.5, m),
                     np.where(kind == 2, rng.uniform(0.5, 40.0, m), rng.uniform(40.0, 900.0, m))))
        v = lo + x * sc
        for i in range(0, m, 3):                                                 # every third record aims at a listed x
            v[i] = _land(X_TARGETS[((i // 3) + b) % len(X_TARGETS)], lo[i], sc[i])
        if m > 7 and b % 50 == 20:
            v[7] = np.nan
        found["pixel"][b, :m] = np.sort(rng.choice(65535 ** 2, m, replace=False)).astype(np.uint32)
        found["level"][b, :m] = lvl
        found["value"][b, :m] = v * rng.choice([-1.0, 1.0], m)
    p = np.full((B, cap), -7.0)
    for b in range(B):
        m = int(count[b])
        p[b, :m] = tr.expon_pvalues(found["value"][b, :m], found["level"][b, :m], loc[b], scale[b])
    return dict(B=B, n_tested=n_tested, cap=cap, nzc=nzc, count=count, stats=stats, loc=loc, scale=scale, found=found, p=p)


def pvalue_classes(k):
    """x of every record as the kernel forms it, and the records of each class of the assertions"""
    B, cap = k["B"], k["cap"]
    live = np.arange(cap)[None, :] < k["count"][:, None]
    lv = np.where(live, k["found"]["level"], 1).astype(np.int64) - 1
    rows = np.arange(B)[:, None]
    x = _x_of(k["found"]["value"], k["loc"][rows, lv], k["scale"][rows, lv])
    nan = live & np.isnan(k["p"])
    ok = live & ~nan
    return x, live, nan, ok


def _upload_found(k):
    import torch
    B, cap = k["B"], k["cap"]
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).cuda()
    return (dev(k["found"].reshape(-1), np.int64).reshape(B, cap, 2), dev(k["count"], np.int32), dev(k["nzc"], np.int32),
            dev(k["stats"], np.float64))


def _found_pvalues(k):
    import torch
    from mustache_amd import _lib
    B, cap = k["B"], k["cap"]
    found, count, nzc, stats = _upload_found(k)
    pval = torch.full((B, cap), -7.0, dtype=torch.float64, device="cuda")
    fit = torch.full((B, T, 2), -7.0, dtype=torch.float64, device="cuda")
    rc = _engine().lib.mst_found_pvalues(_lib.ptr(found), cap, _lib.ptr(count), _lib.ptr(nzc), _lib.ptr(stats), B, k["n_tested"],
                                         _lib.ptr(pval), _lib.ptr(fit), _lib.stream())
    return rc, pval.cpu().numpy(), fit.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def test_fit_and_pvalues_on_every_branch_against_scipy():
    """B = 301 blocks (more than the fit kernel's 256 threads, odd), n_tested = MST_MAX_TESTED, 0 .. cap records per block.
    The bound on |p - p_scipy| is 2^-52: HIP's double exp and expm1 are within 1 ulp, the results lie in [0, 1], and two more
    roundings follow.  Measured on an MI355X: the largest deviation is exactly 2^-52 (2.22e-16); 1682 of the 41 409 records
    that SciPy gives a number for differ from it at all."""
    from mustache_amd import _lib
    k = _pvalue_case()
    B, nt = k["B"], k["n_tested"]
    x, live, nan, ok = pvalue_classes(k)
    classes = {"x <= 0": int(np.sum(ok & (x <= 0))), "0 < x <= 0.5": int(np.sum(ok & (x > 0) & (x <= 0.5))),
               "0.5 < x < 40": int(np.sum(ok & (x > 0.5) & (x < 40))), "x >= 40": int(np.sum(ok & (x >= 40))),
               "NaN (scale <= 0)": int(np.sum(nan & ~np.isnan(k["found"]["value"]))),
               "NaN (value)": int(np.sum(nan & np.isnan(k["found"]["value"])))}
    print("p-value records per class: %r" % classes)
    assert min(classes.values()) >= 5 and min(list(classes.values())[:5]) > 500
    for t in X_TARGETS:
        assert np.any(ok & (x == t)), "no record lands on x = %r" % t
    assert set(np.unique(k["found"]["level"][live])) == set(range(1, nt + 1))
    assert k["count"].min() == 0 and k["count"].max() == k["cap"] and np.any(k["p"][ok] == 0.0)
    rc, p, fit = _found_pvalues(k)
    assert rc == _lib.MST_OK
    assert _same_bits(fit[:, :nt, 0], k["loc"][:, :nt]) and _same_bits(fit[:, :nt, 1], k["scale"][:, :nt]), "fit = (min, sum / count - min)"
    assert (fit[:, nt:] == -7.0).all()
    assert (p[~live] == -7.0).all(), "a p-value past a block's count was written"
    assert np.array_equal(np.isnan(p) & live, nan), "NaN exactly where SciPy gives NaN"
    assert (p[ok & (x <= 0)] == 1.0).all()
    assert (p[ok & (x >= 40)] == 0.0).all()
    dev = np.abs(p[ok] - k["p"][ok])
    print("largest |p - p_scipy| = %.3e = %.3f * 2^-52 over %d records (%d differ at all)"
          % (dev.max(), dev.max() * 2.0 ** 52, dev.size, int(np.sum(dev > 0))))
    assert dev.max() <= 2.0 ** -52
    assert ((p[ok] >= 0) & (p[ok] <= 1)).all()


def test_found_pvalues_overflow_and_non_finite_statistics():
    from mustache_amd import _lib
    base = _pvalue_case(B=4, n_tested=18, cap=256, seed=14, special=False, counts=(256, 100, 31, 0))
    assert np.isnan(base["stats"][:, 18:]).all(), "statistics past n_tested are never read"
    rc, p, _ = _found_pvalues(base)
    live = np.arange(256)[None, :] < base["count"][:, None]
    assert rc == _lib.MST_OK and not (p[live] == -7.0).any() and (p[~live] == -7.0).all()
    # one block over the capacity: the error, and nothing of that block written
    k = dict(base, count=base["count"].copy())
    k["count"][2] = k["cap"] + 1
    rc, p, _ = _found_pvalues(k)
    assert rc == _lib.MST_E_OVERFLOW and "capacity" in _engine().lib.mst_last_error().decode()
    assert (p[2] == -7.0).all() and not (p[0] == -7.0).any()
    # NaN statistics where pixels were tested: the error; where none were: fine
    for nz2, rc_exp in ((int(base["nzc"][2]), _lib.MST_E_NONFINITE), (0, _lib.MST_OK)):
        k = dict(base, stats=base["stats"].copy(), nzc=base["nzc"].copy(), count=base["count"].copy())
        k["stats"][2, 17, 0] = np.nan
        k["nzc"][2] = nz2
        k["count"][2] = 0 if nz2 == 0 else k["count"][2]
        rc, p, fit = _found_pvalues(k)
        assert rc == rc_exp, (nz2, rc)
        assert np.isnan(fit[2, 17]).all()
    k = dict(base, stats=base["stats"].copy())
    k["stats"][1, 3, 1] = np.inf
    assert _found_pvalues(k)[0] == _lib.MST_E_NONFINITE


@pytest.mark.parametrize("B,counts,nt", [(1, [9], 18), (2, [5, 12], 18), (5, [7, 0, 20, 3, 20], 48)])
def test_found_finish_summary_and_packed_arrays(B, counts, nt):
    """mst_found_finish: the summary block as launch.parse_summary reads it, and the first min(pitch, count) records of every
    block once more as three narrow arrays -- at pitches below, at and above the largest count"""
    import torch
    from mustache_amd import _lib
    from mustache_amd.launch import parse_summary
    lib = _engine().lib
    k = _pvalue_case(B=B, n_tested=nt, cap=32, seed=15 + B, special=False, counts=tuple(counts))
    exp_p = k["p"]
    assert k["found"]["pixel"].max() > 2 ** 31, "pixels past the int32 range of the packed array"
    found, count, nzc, stats = _upload_found(k)
    nbytes = int(lib.mst_found_summary_bytes(B))
    cmax = max(counts)
    for pitch in (1, cmax - 1, cmax, cmax + 7):
        pval = torch.full((B, 32), -7.0, dtype=torch.float64, device="cuda")
        fit = torch.full((B, T, 2), -7.0, dtype=torch.float64, device="cuda")
        pix_out = torch.full((B, pitch), -1, dtype=torch.int32, device="cuda")
        lvl_out = torch.full((B, pitch), 255, dtype=torch.uint8, device="cuda")
        pv_out = torch.full((B, pitch), -7.0, dtype=torch.float64, device="cuda")
        scratch = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        summ = torch.full((nbytes,), 0xEE, dtype=torch.uint8).pin_memory()
        _lib.check(lib.mst_found_finish(_lib.ptr(found), 32, _lib.ptr(count), _lib.ptr(nzc), _lib.ptr(stats), B, nt, _lib.ptr(pval),
                                        _lib.ptr(fit), pitch, _lib.ptr(pix_out), _lib.ptr(lvl_out), _lib.ptr(pv_out),
                                        _lib.ptr(scratch), _lib.ptr(summ), None, None, None, 0, _lib.stream()))
        s_count, s_nz, s_fit = parse_summary(summ.numpy(), B)
        assert list(s_count) == list(counts) and list(s_nz) == [int(v) for v in k["nzc"]]
        assert _same_bits(s_fit[:, :nt, 0], k["loc"][:, :nt]) and _same_bits(s_fit[:, :nt, 1], k["scale"][:, :nt])
        assert _same_bits(fit.cpu().numpy()[:, :nt], s_fit[:, :nt])
        assert int(summ.numpy()[:4].view(np.int32)[0]) == 0
        p = pval.cpu().numpy()
        live = np.arange(32)[None, :] < np.asarray(counts)[:, None]
        assert (p[~live] == -7.0).all()
        assert np.array_equal(np.isnan(p), np.isnan(exp_p)) and np.nanmax(np.abs(p - exp_p)[live], initial=0.0) <= 2.0 ** -52
        pix_h, lvl_h, pv_h = pix_out.cpu().numpy().view(np.uint32), lvl_out.cpu().numpy(), pv_out.cpu().numpy()
        for b in range(B):
            w = min(pitch, counts[b])
            assert np.array_equal(pix_h[b, :w], k["found"]["pixel"][b, :w]), (pitch, b)
            assert np.array_equal(lvl_h[b, :w], k["found"]["level"][b, :w].astype(np.uint8)), (pitch, b)
            assert _same_bits(pv_h[b, :w], p[b, :w]), (pitch, b)
            assert (pix_h[b, w:] == 0xFFFFFFFF).all() and (lvl_h[b, w:] == 255).all() and (pv_h[b, w:] == -7.0).all(), (pitch, b)


# ---- clustering -----------------------------------------------------------------------------------------------------------
def _by_label(CH, rec, q, cand, pt=0.1):
    sel = np.nonzero(q < pt)[0]
    return [int(sel[r]) for r in tr.cluster_by_label(CH, rec["pixel"][sel], q[sel], np.searchsorted(sel, cand))]


def test_clustering_equals_scipy_label_on_the_painted_matrix():
    rng = np.random.default_rng(16)
    params = {64: ((60, 1, 0.7, 0.05), (150, 2, 0.5, 0.0)), 200: ((300, 3, 0.5, 0.0), (500, 5, 0.3, 0.01)),
              512: ((900, 4, 0.6, 0.02), (1500, 9, 0.9, 0.005))}
    total = several = 0
    for CH, pp in params.items():
        cases = [_clump_case(rng, CH, *pp[i % 2]) for i in range(10)]
        batch = _record_batch(CH, [c[0] for c in cases])
        got = batch.cluster_representatives_multi(list(range(10)), [c[1] for c in cases], [c[2] for c in cases], 0.1)
        for b, (rec, q, cand) in enumerate(cases):
            exp = _by_label(CH, rec, q, cand)
            assert got[b] == exp, (CH, b)
            total += len(exp)
            several += len(cand) - len(exp)
    assert total > 300 and several > 300, (total, several)


def _snake(count, run=300, x0=1, y0=2):
    """candidates exactly 3 apart (Chebyshev) along one chain: runs of `run` along rows x0, x0 + 6, ... in alternating
    direction, joined by one candidate at the run's end three rows down.  The chain is listed from its bottom end: its far end
    is the RIGHT end of the top row, while the raster-first candidate is that row's left end."""
    pts, row, right_to_left = [], x0, True
    while len(pts) < count:
        cols = [y0 + 3 * j for j in range(run)]
        cols = cols[::-1] if right_to_left else cols
        pts += [(row, c) for c in cols] + [(row + 3, cols[-1])]
        row += 6
        right_to_left = not right_to_left
    return pts[:count][::-1]


def _chain_record(CH, pts, q):
    pix = np.array([x * CH + y for x, y in pts], dtype=np.int64)
    o = np.argsort(pix)
    return {"pixel": pix[o].astype(np.uint32), "level": np.ones(len(pix), np.uint32), "q": np.asarray(q)[o]}, o


def test_clustering_of_long_chains():
    """label propagation over 2000 links, in an order that disagrees with the raster order of the candidates"""
    from mustache_amd.tail import cluster_representatives
    CH, N = 1000, 2000
    rng = np.random.default_rng(17)
    pts = _snake(N)
    d = np.abs(np.diff(np.array(pts), axis=0)).max(axis=1)
    assert (d == 3).all() and len(set(pts)) == N and max(max(p) for p in pts) < CH
    rows = np.array(pts)[:, 0]
    along = np.diff(np.array(pts)[:, 1])[np.diff(rows) == 0]
    assert np.sum(along > 0) > 500 and np.sum(along < 0) > 500, "the chain runs with and against the raster order"
    base_q = rng.uniform(0.01, 0.09, N)
    blocks, expect = [], []
    # (0) distinct q, the minimum somewhere inside; (1) the minimum at the far end with a tie at the near end: the far end is
    # raster-first; (2) the minimum at the near end alone
    q0 = base_q.copy()
    q1 = base_q.copy(); q1[0] = q1[-1] = 0.001
    q2 = base_q.copy(); q2[0] = 0.001
    for q, want in ((q0, pts[int(np.argmin(q0))]), (q1, pts[-1]), (q2, pts[0])):
        rec, _ = _chain_record(CH, pts, q)
        blocks.append(rec)
        expect.append([int(np.searchsorted(rec["pixel"], want[0] * CH + want[1]))])
    # (3) one link widened to 4: everything from the chain's 700th candidate on (towards the top) stays, the part below it
    # moves one row down -- the break is at a joint, whose two ends sit in one column
    joints = [i for i in range(1, N) if pts[i][1] == pts[i - 1][1]]
    cut = joints[len(joints) // 2]
    low = [(x + 1, y) for x, y in pts[:cut]]
    wide = low + pts[cut:]
    dw = np.abs(np.diff(np.array(wide), axis=0)).max(axis=1)
    assert np.sum(dw == 4) == 1 and np.sum(dw == 3) == N - 2
    rec, _ = _chain_record(CH, wide, base_q)
    blocks.append(rec)
    upper, lower = wide[cut + int(np.argmin(base_q[cut:]))], wide[int(np.argmin(base_q[:cut]))]
    expect.append([int(np.searchsorted(rec["pixel"], x * CH + y)) for x, y in (upper, lower)])
    batch = _record_batch(CH, blocks)
    cand = [np.arange(N, dtype=np.int64)] * 4
    got = batch.cluster_representatives_multi([0, 1, 2, 3], [b["q"] for b in blocks], cand, 0.1)
    for b in range(4):
        assert got[b] == expect[b], b
        assert cluster_representatives(batch, b, blocks[b]["q"], cand[b]) == expect[b], b
    assert blocks[1]["pixel"][expect[1][0]] != blocks[1]["pixel"][0], "the representative is not the raster-first candidate"


def test_clustering_at_the_largest_block_the_entry_point_admits():
    """CH = 65535: pixel keys up to 2^32 - 131 072 and r * CH + y in uint32; candidates and selected neighbours on the block's
    first and last two rows and columns; (r, CH - 1) and (r + 1, 0) are neighbours as keys, not as pixels"""
    from mustache_amd.tail import cluster_representatives
    CH = 65535
    E = CH - 1
    recs = [  # (x, y, q, candidate)
        (0, 0, 0.05, True), (1, 1, 0.01, False),
        (10, E, 0.05, True), (11, 0, 0.001, False), (10, E - 1, 0.02, False),
        (20, 0, 0.05, True), (19, E, 0.001, False), (21, 1, 0.03, False),
        (E, E, 0.03, True), (E - 1, E - 1, 0.02, False), (E - 1, E, 0.025, False),
        (E, 0, 0.04, True), (E - 1, 3, 0.03, True), (E, 6, 0.035, True), (E - 1, 10, 0.001, True),
        (1, 30000, 0.05, True), (1, 30003, 0.04, True), (0, 30006, 0.03, True), (0, 30007, 0.02, False),
        (E, 40000, 0.05, True), (E, 40001, 0.05, False), (E - 1, 39999, 0.06, False),
        (30000, E, 0.05, True), (30003, E - 1, 0.04, True), (30001, E, 0.045, False),
    ]
    pix = np.array([x * CH + y for x, y, _, _ in recs], dtype=np.int64)
    assert pix.max() == CH * CH - 1 == 2 ** 32 - 2 ** 17
    o = np.argsort(pix)
    edge = {"pixel": pix[o].astype(np.uint32), "level": np.ones(len(pix), np.uint32), "q": np.array([r[2] for r in recs])[o]}
    edge_cand = np.nonzero(np.array([r[3] for r in recs])[o])[0]
    where = lambda x, y: int(np.searchsorted(edge["pixel"], x * CH + y))
    edge_exp = [where(1, 1), where(0, 30007), where(10, E - 1), where(21, 1), where(30003, E - 1), where(E - 1, 3),
                where(E - 1, 10), where(E, 40000), where(E - 1, E - 1)]
    rng = np.random.default_rng(18)
    clumps = [_clump_case(rng, CH, 2400, 4, 0.6, 0.02), _clump_case(rng, CH, 1200, 2, 0.9, 0.0)]
    blocks = [edge] + [c[0] for c in clumps]
    qs = [edge["q"]] + [c[1] for c in clumps]
    cands = [edge_cand] + [c[2] for c in clumps]
    batch = _record_batch(CH, blocks)
    got = batch.cluster_representatives_multi([0, 1, 2], qs, cands, 0.1)
    assert got[0] == edge_exp
    total = 0
    for b in range(3):
        exp = cluster_representatives(batch, b, qs[b], cands[b])
        assert got[b] == exp, b
        total += len(exp)
    assert total > 300
    assert max(int(c[0]["pixel"].max()) for c in clumps) > 2 ** 31
