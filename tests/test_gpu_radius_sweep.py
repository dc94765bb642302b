"""The sigma-stack kernel at every blur radius each of its tiles is built for (tests/radius_sweep.py: TileDefault 1..14,
TileWide 1..28, TileDefaultFma 1..14 -- 56 instantiations of vpass / hpass / fir_chunk) against SciPy itself:
oracle.block_prologue + oracle.scale_space_levels(blur="scipy") on synthetic normalised blocks, the COMPLETE found set.
Pixels, levels, DoG values and loc identical, scale to 1e-12, p-values to 1e-9 (the tolerances of test_gpu_block.py), the
tested-pixel count exact.  Every list runs from the dense block and from the band (three overlapping blocks in one launch,
tiles shared and not), with and without empty tiles skipped, on an odd block edge with partial tiles, on a block smaller
than one tile and on a block smaller than its largest blur radius (reflection folds more than once).  Tables of 36 and 45
tested levels (4 and 5 octaves) and lists whose octaves do not double (no blur kept across octaves) are among them."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radius_sweep as rs      # noqa: E402

pytestmark = pytest.mark.gpu

RAN = set()           # (tile, radius) pairs whose comparison passed


def _tile(name):
    return rs.sigma_tile(rs.level_table(rs.SIGMA_SWEEP[name][0]))


CASES = [(name, g) for name in rs.SIGMA_SWEEP for g in range(3)]
IDS = ["%s-%dx%d" % (name, *rs.SIGMA_GEOMETRY[_tile(name)][g]) for name, g in CASES]


@functools.lru_cache(maxsize=None)
def _engine(name):
    from mustache_amd.engine import ScaleSpaceEngine
    eng = ScaleSpaceEngine(rs.SIGMA_SWEEP[name][0])
    if name in rs.LONG_LISTS:
        assert eng.levels.n_tested == rs.LONG_LISTS[name] and eng.levels.n_tested in (36, 45)
    return eng


@functools.lru_cache(maxsize=None)
def _dense_case(name, g):
    n, dpx = rs.SIGMA_GEOMETRY[_tile(name)][g]
    c = rs.sweep_block(n, dpx)
    return c, dpx, rs.reference_found(c, dpx, rs.SIGMA_SWEEP[name][0])


@functools.lru_cache(maxsize=None)
def _band_case(name, g):
    """(COO of the chromosome, its length, dpx, block starts, CH)"""
    CH, dpx = rs.SIGMA_GEOMETRY[_tile(name)][g]
    step = rs.BAND_STEP[CH]
    n = CH + 2 * step
    return rs.sweep_coo(n, dpx), n, dpx, [0, step, 2 * step], CH


def _compare(eng, rec, fit, nzc, ref, what):
    nt = eng.levels.n_tested
    assert nzc == ref["n_tested_pixels"], what
    assert len(ref["pixel"]) > 0, ("the reference's found set is empty", what)
    assert np.array_equal(rec["pixel"].astype(np.int64), ref["pixel"]), what
    assert np.array_equal(rec["level"].astype(np.int64), ref["level"].astype(np.int64)), what
    assert np.array_equal(rec["value"], ref["value"]), (what, int((rec["value"] != ref["value"]).sum()))
    assert len(ref["loc"]) == nt
    assert np.array_equal(np.asarray(fit[0])[:nt], ref["loc"]), what
    np.testing.assert_allclose(np.asarray(fit[1])[:nt], ref["scale"], rtol=1e-12, err_msg=str(what))
    np.testing.assert_allclose(rec["pval"], ref["pval"], rtol=1e-9, atol=0, err_msg=str(what))


def _ran(name, tile=None):
    tile = _tile(name) if tile is None else tile
    RAN.update((tile, r) for r in rs.level_table(rs.SIGMA_SWEEP[name][0]).radius)


@pytest.mark.parametrize("name,g", CASES, ids=IDS)
def test_dense_source_every_radius_vs_scipy(name, g):
    import torch
    eng = _engine(name)
    c, dpx, ref = _dense_case(name, g)
    for skip_empty in (True, False):
        dev = torch.from_numpy(c.copy()).cuda().unsqueeze(0)
        nz, nzc = eng.prologue(dev, dpx, True)
        assert np.array_equal(nz[0].cpu().numpy().astype(bool), ref["nz"])
        found, fits = eng.sigma_loop(dev, nz, nzc, skip_empty=skip_empty)
        _compare(eng, found[0], fits[0], int(nzc.cpu().numpy()[0]), ref, (name, c.shape[0], dpx, "dense", skip_empty))
    if g == 0:
        assert len(ref["pixel"]) > 10000
    _ran(name)


@pytest.mark.parametrize("name,g", CASES, ids=IDS)
def test_band_source_every_radius_vs_scipy(name, g):
    """three overlapping blocks of one chromosome in ONE launch of the band-direct kernel; every block against the
    reference on the dense block cut from the same band.  With sharing, the blocks of 333 hand tiles on: the middle one
    receives some from the first and gives some to the last; the smaller blocks have no room for a shared tile (a tile with
    its halo is larger than they are)."""
    import torch
    from mustache_amd.normalize import band_from_coo
    eng = _engine(name)
    (x, y, v), n, dpx, starts, CH = _band_case(name, g)
    band = band_from_coo(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(v).cuda(), n, dpx)
    host = band.cpu().numpy()
    refs = [rs.reference_found(rs.block_from_band(host[:, s:s + CH], CH, dpx), dpx, rs.SIGMA_SWEEP[name][0]) for s in starts]
    try:
        for share in (True, False):
            eng.share_tiles = share
            for skip_empty in (True, False):
                items, tiles, shared = eng.band_items(starts, CH, dpx, skip_empty=skip_empty, share=share)
                assert items + shared == tiles
                if share and CH == 333:
                    first = eng.band_items(starts[:2], CH, dpx, skip_empty=skip_empty, share=True)[2]
                    assert 0 < first < shared, "the middle block receives tiles and gives tiles"
                else:
                    assert shared == 0
                found, fits, nzc = eng.sigma_loop_band(band, n, dpx, starts, CH, skip_empty=skip_empty)
                counts = nzc.cpu().numpy().view(np.uint32)
                for b in range(len(starts)):
                    _compare(eng, found[b], fits[b], int(counts[b]), refs[b], (name, CH, dpx, "band", share, skip_empty, b))
    finally:
        eng.share_tiles = True
    _ran(name)


@pytest.mark.parametrize("name", [n for n, (_, doubling) in rs.SIGMA_SWEEP.items() if not doubling])
def test_mustache_dropin_without_level_reuse_vs_oracle(name):
    """the lists whose octaves do not double through the drop-in mustache(): loops of the reference's restatement"""
    import oracle
    from mustache_amd.mustache import mustache
    octs = rs.SIGMA_SWEEP[name][0]
    assert not any(rs.level_reuse(rs.level_table(octs)))
    n, dpx = rs.SIGMA_GEOMETRY[_tile(name)][0]
    c = rs.sweep_block(n, dpx, ramp=False)
    exp = oracle.mustache_block(c.copy(), 40, dpx, octs, 0.3, 0.9)
    got = mustache(c, "1", "1", 5000, [], 40, 40 + n, 0, dpx, octs, 0.3, 0.9)
    assert len(exp) > 0
    assert [(int(a), int(b)) for a, b, _, _ in got] == [(int(a), int(b)) for a, b, _, _ in exp]
    assert [s for _, _, _, s in got] == [s for _, _, _, s in exp]
    np.testing.assert_allclose([q for _, _, q, _ in got], [q for _, _, q, _ in exp], rtol=1e-9)


def _sieve_margins(ss, nz, n_octaves, s=10):
    """per tested pixel, the smallest relative margin |a - b| / max(|a|, |b|) of any comparison of D_c against best, M_c,
    M_p, M_n the reference's sieve makes at any level (replayed from the DoGs oracle.scale_space_levels kept)"""
    import oracle

    def rel(a, b):
        m = np.maximum(np.abs(a), np.abs(b))
        return np.where(m > 0, np.abs(a - b) / np.where(m > 0, m, 1.0), 0.0)

    best = np.zeros(int(nz.sum()))
    out = np.full(best.shape, np.inf)
    for o in range(n_octaves):
        for i in range(3, s + 2):
            d_p, d_c, d_n = ss.dog[(o, i - 2)], ss.dog[(o, i - 1)], ss.dog[(o, i)]
            m_p, m_c, m_n = (oracle.scale_space.maxfilter3_zero(d)[nz] for d in (d_p, d_c, d_n))
            dc = d_c[nz]
            # (D_c == M_c holds exactly wherever the pixel is its own 3 x 3 maximum: the margin is to the other eight)
            pad = np.zeros((d_c.shape[0] + 2, d_c.shape[1] + 2))
            pad[1:-1, 1:-1] = d_c
            ring = np.max([pad[dy:dy + d_c.shape[0], dx:dx + d_c.shape[1]] for dy in range(3) for dx in range(3)
                           if (dy, dx) != (1, 1)], axis=0)[nz]
            for other in (best, ring, m_p, m_n):
                out = np.minimum(out, rel(dc, other))
            upd = (dc > best) & (dc == m_c) & ((d_p[nz] == m_p) | (d_n[nz] == m_n)) & (dc > m_p) & (dc > m_n)
            best[upd] = dc[upd]
    return out


def test_fma_tile_every_radius_against_the_exact_tile():
    """TileDefaultFma at radii 1..14 (the four-octave list, 36 tested levels) against the default tile's run of the same
    block, as test_opt_in_fma_mode_within_north_star_tolerance holds it at the default octaves: same pixels and levels,
    values to 1e-9, p-values to 1e-5, scale to 1e-9.  Where the two found sets differ, every pixel of the difference must
    have had a sieve comparison that a relative margin below 1e-9 decided (the reference's DoGs), and the rest is compared
    on the intersection."""
    import torch
    name = rs.FMA_LIST
    eng = _engine(name)
    nt = eng.levels.n_tested
    n, dpx = rs.SIGMA_GEOMETRY["default"][0]
    c = rs.sweep_block(n, dpx, far=False, ramp=False)
    dev = torch.from_numpy(c.copy()).cuda().unsqueeze(0)
    nz, nzc = eng.prologue(dev, dpx, True)
    a, fa = eng.sigma_loop(dev, nz, nzc, fma=False)
    b, fb = eng.sigma_loop(dev, nz, nzc, fma=True)
    ra, rb = a[0], b[0]
    assert len(ra["pixel"]) > 1000
    ka = ra["pixel"].astype(np.int64) * 64 + ra["level"].astype(np.int64)
    kb = rb["pixel"].astype(np.int64) * 64 + rb["level"].astype(np.int64)
    odd = np.setxor1d(ka, kb) // 64
    print("FMA tile, %d tested levels: %d found, %d records in one found set only" % (nt, len(ka), len(odd)))
    if len(odd):
        ref = rs.reference_found(c, dpx, rs.SIGMA_SWEEP[name][0], keep_levels=True)
        margins = _sieve_margins(ref["ss"], ref["nz"], len(rs.SIGMA_SWEEP[name][0]))
        where = np.searchsorted(np.flatnonzero(ref["nz"].ravel()), np.unique(odd))
        assert (margins[where] < 1e-9).all(), (np.unique(odd), margins[where])
    ia, ib = np.isin(ka, kb), np.isin(kb, ka)
    assert not np.array_equal(ra["value"][ia], rb["value"][ib]), "the relaxed mode really is a different rounding sequence"
    np.testing.assert_allclose(rb["value"][ib], ra["value"][ia], rtol=1e-9)
    np.testing.assert_allclose(rb["pval"][ib], ra["pval"][ia], rtol=1e-5, atol=1e-300)
    np.testing.assert_allclose(np.asarray(fb[0][1])[:nt], np.asarray(fa[0][1])[:nt], rtol=1e-9)
    _ran(name, "fma")


def test_every_instantiation_has_run():
    """all 56 (tile, radius) pairs of the sigma loop went through a comparison: in the tests above when the file runs as a
    whole, else here on the smallest blocks"""
    for name in rs.SIGMA_SWEEP:
        if not set((_tile(name), r) for r in rs.level_table(rs.SIGMA_SWEEP[name][0]).radius) <= RAN:
            test_dense_source_every_radius_vs_scipy(name, 1)
    if not any(t == "fma" for t, _ in RAN):
        test_fma_tile_every_radius_against_the_exact_tile()
    want = set((t, r) for t, rmax in rs.SIGMA_TILE_RMAX.items() for r in range(1, rmax + 1))
    print("sigma-loop instantiations compared:", sorted(RAN))
    assert RAN == want and len(RAN) == 56, sorted(want - RAN)
