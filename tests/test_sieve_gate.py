"""The fused kernel's sieve gate and level statistics on inputs that reach every branch of their forms
(mst_scale_space.hip: the sieve bits are shifted into their words pixel by pixel and shifted out again as the gate's lane
mask, a never-tested pixel holds best = +inf, the statistics select the words of D_c).  Each case is ONE launch of the
band-source kernel on the smallest geometry that spans several tiles in both directions with the block edge inside the last tile row and column (a block of 140 x 140,
distance limit 100: 5 x 3 default tiles), against oracle.block_prologue + oracle.scale_space_levels(blur="scipy"): pixels,
levels and values with np.array_equal, loc exactly, scale to 1e-12 and p-values to 1e-9 (the bounds of
test_gpu_radius_sweep.py), and the statistics of the same blocks through the staged and the launch-per-group form.

What the block holds, each asserted on the oracle's own DoG levels before anything is compared:
  * tested pixels whose gate is CLOSED at a level where D_c > max(best, M_n) nevertheless holds (neighbours of a peak, and
    a two-pixel plateau: mirror-symmetric input, so two adjacent pixels carry the same D_c bit for bit and both equal their
    3 x 3 maximum) and that are never found;
  * with octaves (1.6, 1.6) the second octave repeats the first bit for bit: every found pixel meets, gate open, a D_c that
    EQUALS its best -- the strict > must leave its level in the first octave;
  * a thinned band: lanes that own no, one and all (8, wide tile: 4) tested pixels of a thread in one wave, and a wave without
    any in a tile that has some -- counted with the thread mapping of the tile the case runs on (TILE_K);
  * tested pixels on the block's last column, inside a tile whose ring and right part lie outside the block (the zero-padded
    maxima), DoG values of both signs, and the same map scaled by 1e-300 and by 1e+150;
  * the same through the wide tile (octaves 1.6, 3.2, 6.4: four pixels per thread) and with two octaves.
test_inputs_on_the_oracle_alone makes these checks without a GPU; the GPU test repeats them before it launches."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radius_sweep as rs      # noqa: E402

CH, DPX = 140, 100
# Both tiles (mst_scale_space.hip, Tile<32, 64, RMAX, K>) are regions of 32 x 64 pixels with a ring of one: 30 x 62 owned pixels, on
# a lattice anchored at chromosome coordinate 0 (build_items: y0 = a * 30 - start - 1) -- the block's origin here, its start is 0.
# A thread owns K consecutive columns of one region row; lanes run along the 32 rows, so a wave is two column groups.
ITR, ITC, RGR = 30, 62, 32
TILE_K = {"default": 8, "wide": 4}
PLATEAU = (15, 60)              # (row, column) of the left pixel of the two-pixel plateau
EDGE_PEAK = (70, CH - 1)        # a peak on the block's last column
CASES = {
    "two-octaves": ([1.6, 3.2], 1.0),
    "two-octaves-1e-300": ([1.6, 3.2], 1e-300),
    "two-octaves-1e+150": ([1.6, 3.2], 1e+150),
    "wide-tile": ([1.6, 3.2, 6.4], 1.0),
    "wide-tile-1e-300": ([1.6, 3.2, 6.4], 1e-300),
    "wide-tile-1e+150": ([1.6, 3.2, 6.4], 1e+150),
    "repeated-octave": ([1.6, 1.6], 1.0),
}


def block(scale=1.0):
    """the dense block [CH, CH] (zero outside the band 0 <= col - row <= DPX + 1), every band value times `scale`"""
    rng = np.random.default_rng(11)
    i, j = np.indices((CH, CH))
    off = j - i
    c = 1.0 + 0.3 * np.sin(0.31 * i + 0.17 * j) + rng.uniform(0.0, 0.4, (CH, CH))
    for (y, x, a, w) in [(20, 100, 6.0, 1.5), (52, 75, 5.0, 1.2), (65, 118, 7.0, 2.0), (100, 130, 6.0, 1.4), (125, 136, 5.0, 1.3),
                         (33, 125, 4.0, 1.1), (EDGE_PEAK[0], EDGE_PEAK[1], 8.0, 1.6), (8, 30, 5.0, 1.5), (90, 104, 3.0, 2.5)]:
        c += a * np.exp(-((i - y) ** 2 + (j - x) ** 2) / (2.0 * w * w))
    # the plateau: a box of constant background, mirror-symmetric about the line between columns x and x + 1 within every
    # blur radius of the two-octave list (14), with two equal pixels on it
    y, x = PLATEAU
    c[max(y - 16, 0):y + 17, x - 16:x + 18] = 1.25
    c[y, x] = c[y, x + 1] = 4.0
    # thinning: exact zeros are not tested.  Tile (1, 1) owns rows 30..59, columns 62..123; its threads own groups of eight
    # columns starting at 61 + 8 g.  32 zero columns hold the 16 columns of a whole wave; three rows of one group get 1, 8
    # and 0 tested pixels.
    c[30:60, 70:102] = 0.0
    c[31, 109:117] = 0.0
    c[31, 112] = 1.5
    c[33, 109:117] = 0.0
    c[(rng.uniform(0.0, 1.0, (CH, CH)) < 0.2) & (i >= 60) & (j < 124)] = 0.0       # and a fifth of the lower left at random
    c[(off < 0) | (off > DPX + 1)] = 0.0
    return c * scale


def lane_counts(nz, K):
    """{(tile row, tile column, wave): [tested pixels of each of its 64 lanes]} for the tile with K pixels per thread:
    lane = region row + 32 * (column group % 2), wave = column group // 2, 64 / K column groups"""
    out = {}
    for ty in range((CH + ITR - 1) // ITR):
        for tx in range((CH + ITC - 1) // ITC):
            y0, x0 = ty * ITR - 1, tx * ITC - 1
            for g in range(64 // K):
                for rr in range(RGR):
                    cols = [x0 + g * K + k for k in range(K) if 1 <= g * K + k <= ITC and x0 + g * K + k < CH]
                    n = int(nz[y0 + rr, cols].sum()) if 1 <= rr <= ITR and y0 + rr < CH and cols else 0
                    out.setdefault((ty, tx, g // 2), [0] * 64)[rr + RGR * (g % 2)] = n
    return out


def replay(ss, nz, n_octaves, s=10):
    """the reference's sieve replayed on the DoG levels it kept: per tested pixel, whether at some tested level its gate was
    closed while D_c > max(best, M_n) held (closed_but_greater), and whether, gate open, D_c equalled best (tie)"""
    from oracle import scale_space as ssm
    best = np.zeros(int(nz.sum()))
    closed_but_greater = np.zeros(best.shape, bool)
    tie = np.zeros(best.shape, bool)
    signs = set()
    for o in range(n_octaves):
        for i in range(3, s + 2):
            d_p, d_c, d_n = ss.dog[(o, i - 2)], ss.dog[(o, i - 1)], ss.dog[(o, i)]
            m_p, m_c, m_n = (ssm.maxfilter3_scipy(d)[nz] for d in (d_p, d_c, d_n))
            dc = d_c[nz]
            gate = (dc == m_c) & ((d_p[nz] == m_p) | (d_n[nz] == m_n)) & (dc > m_p)
            closed_but_greater |= ~gate & (dc > np.maximum(best, m_n))
            tie |= gate & (dc == best) & (dc > m_n)
            upd = gate & (dc > np.maximum(best, m_n))
            best[upd] = dc[upd]
            signs.update(np.sign(dc).astype(int).tolist())
    return closed_but_greater, tie, signs


@functools.lru_cache(maxsize=None)
def case(name):
    """(block, reference_found of it, the checks of the module docstring on the reference) -- computed once per case"""
    octaves, scale = CASES[name]
    c = block(scale)
    ref = rs.reference_found(c, DPX, octaves, keep_levels=True)
    nz, ss = ref["nz"], ref["ss"]
    idx = -np.ones(nz.shape, np.int64)
    idx[nz] = np.arange(int(nz.sum()))
    closed, tie, signs = replay(ss, nz, len(octaves))
    facts = dict(found=int(ref["hit"].sum()), closed_never_found=int((closed & ~ref["hit"]).sum()), ties=int(tie.sum()),
                 signs=signs, K=TILE_K[rs.sigma_tile(rs.level_table(octaves))])
    facts["lanes"] = lane_counts(nz, facts["K"])
    # the plateau: both pixels tested, bit-identical DoG at every level of the first octave, and treated alike
    (y, x) = PLATEAU
    facts["plateau_equal"] = all(ss.dog[(0, k)][y, x] == ss.dog[(0, k)][y, x + 1] for k in range(1, 12))
    facts["plateau_found"] = (bool(ref["hit"][idx[y, x]]), bool(ref["hit"][idx[y, x + 1]]))
    facts["plateau_neighbour_closed"] = bool(closed[idx[y, x - 1]] or closed[idx[y + 1, x]] or closed[idx[y - 1, x]])
    facts["plateau_neighbour_found"] = bool(ref["hit"][idx[y, x - 1]] or ref["hit"][idx[y + 1, x]] or ref["hit"][idx[y - 1, x]])
    facts["edge_found"] = int(ref["hit"][idx[:, CH - 1][nz[:, CH - 1]]].sum())
    facts["tie_levels"] = ref["ss"].level[tie & ref["hit"]]
    return c, ref, facts


def check_reference(name):
    """what the module docstring promises of the inputs, on the oracle alone (no GPU): run before anything is launched"""
    octaves, scale = CASES[name]
    c, ref, f = case(name)
    assert f["found"] > 0, "positive cases: the oracle finds pixels"
    assert f["closed_never_found"] > 0, "gate closed, D_c > max(best, M_n) true, never found"
    assert f["signs"] >= {-1, 1}, "DoG values of both signs on tested pixels"
    assert f["edge_found"] > 0, "a found pixel on the block's last column"
    assert c[c != 0].min() >= 0.3 * scale and np.isfinite(c).all()
    if name == "two-octaves":
        assert f["plateau_equal"], "the plateau's two pixels carry the same DoG bits"
        assert f["plateau_found"][0] == f["plateau_found"][1], "and the sieve treats them alike"
        assert f["plateau_neighbour_closed"] and not f["plateau_neighbour_found"], "a plateau neighbour: gate closed, greater, not found"
    if name == "repeated-octave":
        assert f["ties"] >= f["found"] > 0, "every found pixel meets D_c == best with its gate open in the repeated octave"
        assert len(f["tie_levels"]) and f["tie_levels"].max() <= 9, "and keeps its level of the first octave"
    lanes, K = f["lanes"], f["K"]
    assert K == (4 if name.startswith("wide-tile") else 8)
    own = slice(1, ITR + 1), slice(RGR + 1, RGR + ITR + 1)          # the lanes of owned rows (not the ring rows 0 and 31)
    assert any(all(n in w[own[0]] + w[own[1]] for n in (0, 1, K)) for w in lanes.values()), \
        "owned-row lanes with 0, 1 and K tested pixels in one wave"
    assert any(sum(w) == 0 and any(sum(v) for (uy, ux, _), v in lanes.items() if (uy, ux) == (ty, tx))
               for (ty, tx, _), w in lanes.items()), "a wave without a tested pixel in a tile that has some"
    last = [w for (ty, tx, _), w in lanes.items() if ty == (CH - 1) // ITR or tx == (CH - 1) // ITC]
    assert sum(sum(w) for w in last) > 0, "tested pixels in the last tile row and column, which the block's edge cuts"


@functools.lru_cache(maxsize=None)
def _engine(name):
    from mustache_amd.engine import ScaleSpaceEngine
    return ScaleSpaceEngine(CASES[name][0])


@pytest.mark.parametrize("name", list(CASES))
def test_inputs_on_the_oracle_alone(name):
    """no GPU: the oracle alone finds pixels in every case and none where it must not, and the block holds what the module
    docstring lists"""
    check_reference(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_sieve_gate_vs_oracle(name):
    import torch
    from mustache_amd.normalize import band_from_coo
    check_reference(name)
    c, ref, _ = case(name)
    eng = _engine(name)
    nt = eng.levels.n_tested
    x, y = np.nonzero(c)
    band = band_from_coo(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(c[x, y]).cuda(), CH, DPX)
    assert np.array_equal(rs.block_from_band(band.cpu().numpy(), CH, DPX), c)
    found, fits, nzc = eng.sigma_loop_band(band, CH, DPX, [0], CH, skip_empty=True)
    rec = {k: v.copy() for k, v in found[0].items()}
    loc, scale = np.asarray(fits[0][0])[:nt].copy(), np.asarray(fits[0][1])[:nt].copy()
    print("%s: %d tested pixels, %d found (oracle %d)" % (name, int(nzc.cpu().numpy().view(np.uint32)[0]), len(rec["pixel"]), len(ref["pixel"])))
    assert int(nzc.cpu().numpy().view(np.uint32)[0]) == ref["n_tested_pixels"]
    assert np.array_equal(rec["pixel"].astype(np.int64), ref["pixel"])
    assert np.array_equal(rec["level"].astype(np.int64), ref["level"].astype(np.int64))
    assert np.array_equal(rec["value"], ref["value"])
    assert np.array_equal(loc, ref["loc"])
    np.testing.assert_allclose(scale, ref["scale"], rtol=1e-12)
    np.testing.assert_allclose(rec["pval"], ref["pval"], rtol=1e-9, atol=0)
    # the statistics of the same block through the staged launch and through the launch-per-group form
    try:
        for staged in (True, False):
            eng.staged_launches = staged
            (recs, fits_g, nzc_g), = list(eng.sigma_loop_band_overlapped(band, CH, DPX, [[0]], CH, skip_empty=True))
            assert np.array_equal(np.asarray(fits_g[0][0])[:nt], loc) and np.array_equal(np.asarray(fits_g[0][1])[:nt], scale), staged
            assert np.array_equal(recs[0]["pixel"], rec["pixel"]) and np.array_equal(recs[0]["value"], rec["value"]), staged
    finally:
        eng.staged_launches = True
