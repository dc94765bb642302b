"""The octave lists that run every (tile, blur radius) instantiation of the two fused blur kernels, and what the tests
around them share.  TEST INFRASTRUCTURE: a plain helper module (like fuzz_cases.py), imported by the CPU coverage test
(tests/test_radius_coverage.py) and by the GPU sweeps (tests/test_gpu_radius_sweep.py, tests/test_gpu_pair_kernels.py).

blur_dispatch (mst_scale_space.hip) and diff_blur_dispatch (mst_diff.hip) instantiate vpass / hpass / fir_chunk of mst_fir.h
once per radius R <= T::RMAX: 14 + 28 + 14 = 56 for the sigma loop (TileDefault, TileWide, TileDefaultFma), 8 + 14 + 28 = 50
for the difference kernel (DiffTile8, DiffTile14, DiffTile28).  A level table reaches an instantiation through its radii
r = int(truncate * sigma + 0.5) (levels.py) and the tile its LARGEST radius selects, so the tables below are chosen by their
radii; test_radius_coverage.py asserts that they cover every pair and that none of them can be dropped."""
import ctypes

import numpy as np

SIGMA_TILE_RMAX = {"default": 14, "wide": 28, "fma": 14}      # TileDefault / TileWide / TileDefaultFma of mst_scale_space.hip
DIFF_TILE_RMAX = {8: 8, 14: 14, 28: 28}                       # DiffTile8 / DiffTile14 / DiffTile28 of mst_diff.hip

# ---- the sigma loop -----------------------------------------------------------------------------------------------------
# name -> (octave list, doubling).  with_tile (mst_scale_space.hip): largest radius <= 14 -> TileDefault, else TileWide;
# MST_FLAG_FMA -> TileDefaultFma (radii <= 14 only).  The 4- and 5-octave lists are `-sz 0.4 -oc 4 / 5` and `-sz 0.385 -oc 5`:
# 36 and 45 tested levels, 48 and 60 levels (MST_MAX_TESTED = 48, MST_MAX_LEVELS = 64).  The lists that do not double get
# first_level = 1 in every octave (make_dev_levels): no blur is kept from one octave to the next.
SIGMA_SWEEP = {
    "sz0.4-oc4": ([0.4, 0.8, 1.6, 3.2], True),
    "nondoubling-2": ([1.2, 3.0], False),
    "sz0.4-oc5": ([0.4, 0.8, 1.6, 3.2, 6.4], True),
    "sz0.385-oc5": ([0.385 * 2 ** i for i in range(5)], True),
    "nondoubling-3": ([1.5, 3.5, 6.0], False),
}
FMA_LIST = "sz0.4-oc4"
LONG_LISTS = {"sz0.4-oc4": 36, "sz0.4-oc5": 45, "sz0.385-oc5": 45}       # name -> tested levels

# (block edge, distance limit in pixels): an odd edge with partial tiles; a block smaller than one tile; a block whose edge
# is smaller than the tile's largest blur radius (reflect_idx folds more than once)
SIGMA_GEOMETRY = {"default": ((333, 200), (61, 40), (13, 11)), "wide": ((333, 200), (61, 40), (24, 20))}
# the band form: three blocks of the same edge, `step` apart, on a chromosome of edge + 2 * step bins.  For 333 the step is
# chosen so that a staged window (tile + halo: 60 x 92 default, 88 x 120 wide) fits into the overlap of both block pairs.
BAND_STEP = {333: 150, 61: 30, 24: 12, 13: 6}


def level_table(octaves):
    from mustache_amd.levels import LevelTable
    return LevelTable(octaves)


def sigma_tile(lt):
    return "default" if max(lt.radius) <= SIGMA_TILE_RMAX["default"] else "wide"


def level_reuse(lt):
    """make_dev_levels' rule, per octave o > 0: levels k = 11, 12 of octave o - 1 and k = 1, 2 of octave o have the same
    radius and byte-identical taps (first_level[o] = 3: the kernel keeps those two blurs)"""
    lpo = lt.levels_per_octave
    out = []
    for o in range(1, len(lt.octave_values)):
        same = True
        for q in range(2):
            a, b = (o - 1) * lpo + lpo - 2 + q, o * lpo + q
            same = same and lt.radius[a] == lt.radius[b] and \
                np.asarray(lt.taps[a], dtype=np.float64).tobytes() == np.asarray(lt.taps[b], dtype=np.float64).tobytes()
        out.append(same)
    return out


def sigma_lists_of(tile):
    """names of the sweep lists a launch on `tile` runs"""
    if tile == "fma":
        return [FMA_LIST]
    return [name for name, (octs, _) in SIGMA_SWEEP.items() if sigma_tile(level_table(octs)) == tile]


def sigma_witnesses(sweep=None):
    """(tile, radius) -> (list name, level index): a level of a list on that tile with that radius -- one in the middle of
    its octave (k = 2 .. 11: its blur enters a tested DoG) before one at its ends (k = 1, 12: the blur enters the sieve's
    neighbour terms D_p / D_n only), then the first list, then the first level"""
    sweep = SIGMA_SWEEP if sweep is None else sweep
    out = {}
    for tile in SIGMA_TILE_RMAX:
        for ends in (False, True):
            for name in sigma_lists_of(tile):
                if name not in sweep:
                    continue
                lt = level_table(sweep[name][0])
                for l, r in enumerate(lt.radius):
                    if (l % lt.levels_per_octave in (0, lt.levels_per_octave - 1)) == ends:
                        out.setdefault((tile, r), (name, l))
    return out


# ---- the difference kernel ----------------------------------------------------------------------------------------------
# mst_diff_dog_band blurs levels k = 2, 3 of every octave and nothing else; the largest of those radii selects the tile
# (<= 8, 9-14, 15-28).  A table the sigma loop accepts has all twelve levels of every octave at radius <= 28, which keeps
# k = 2, 3 at <= 16: DiffTile28's instantiations 17..28 are reached through the C ABI alone, with a level table whose OTHER
# levels are wider than any kernel supports (the entry point reads k = 2, 3 only).  DiffLevels builds such tables.
DIFF_SWEEP = {
    "t8": [0.45, 1.35, 2.25, 3.2],                     # radii 1..8
    "t14-low": [0.45, 1.35, 2.25, 3.2, 4.05],          # 1..10
    "t14-high": [5.0, 5.9],                           # 11..14
    "t28-low": [0.45, 1.35, 2.25, 3.2, 12.15],          # 1..8, 27, 28
    "t28-mid": [4.05, 5.0, 5.9, 6.8, 11.3],           # 9..16, 25, 26
    "t28-high": [7.7, 8.55, 9.45, 10.38],              # 17..24
}
DIFF_BASE_LISTS = ([1.6, 3.2], [2.0, 4.0], [5.0], [3.2, 6.4], [1.6, 3.2, 6.4])     # test_gpu_pair_kernels.OCTAVE_LISTS


class DiffLevels:
    """The level table of an octave list by levels.py's arithmetic (oracle.level_table restates it) WITHOUT the sigma
    loop's limits, in the form the difference kernel's tests use: sigma, truncate, radius, taps (centre first) per level and
    the C struct, whose taps are filled for the levels that fit it (radius <= MST_MAX_RADIUS)."""

    def __init__(self, octaves, s=10):
        import oracle
        self.octave_values = [float(o) for o in octaves]
        self.s = s
        self.levels_per_octave = s + 2
        rows = oracle.level_table(self.octave_values, s)
        self.sigma = [lv["sigma"] for lv in rows]
        self.truncate = [lv["truncate"] for lv in rows]
        self.radius = [lv["radius"] for lv in rows]
        self.taps = [lv["weights"][lv["radius"]:].copy() for lv in rows]

    def diff_radii(self):
        lpo = self.levels_per_octave
        return [self.radius[o * lpo + q] for o in range(len(self.octave_values)) for q in (1, 2)]

    def as_struct(self):
        from mustache_amd import _lib
        st = _lib.MstLevels()
        st.n_octaves = len(self.octave_values)
        st.levels_per_octave = self.levels_per_octave
        for l, (r, sg, tp) in enumerate(zip(self.radius, self.sigma, self.taps)):
            st.radius[l] = r
            st.sigma[l] = sg
            if r <= _lib.MST_MAX_RADIUS:
                for j in range(r + 1):
                    st.taps[l][j] = float(tp[j])
        return st


def diff_tile(lt):
    mr = max(lt.diff_radii())
    return next(t for t in sorted(DIFF_TILE_RMAX) if mr <= DIFF_TILE_RMAX[t])


def diff_lists():
    """every list the difference kernel's tests run: (name, octaves)"""
    return [(",".join(map(str, o)), o) for o in DIFF_BASE_LISTS] + list(DIFF_SWEEP.items())


def diff_witnesses(lists=None):
    """(tile, radius) -> (list name, level index)"""
    out = {}
    for name, octs in (diff_lists() if lists is None else lists):
        lt = DiffLevels(octs)
        lpo = lt.levels_per_octave
        for o in range(len(octs)):
            for q in (1, 2):
                out.setdefault((diff_tile(lt), lt.radius[o * lpo + q]), (name, o * lpo + q))
    return out


# ---- inputs and the reference's runs ------------------------------------------------------------------------------------
def sweep_coo(n, dpx, seed=29):
    """a synthetic normalised chromosome of n bins as COO (the input form of test_exact_zero_pvalue_and_top_edge_candidates)"""
    import oracle
    from mustache_amd.synth import synth_coo
    x, y, v = synth_coo(n, dpx, depth=300.0, seed=seed, nloops=max(n // 16, 2))
    oracle.normalize_sparse(x, y, v, 50000, dpx)
    return x, y, v


def sweep_block(n, dpx, seed=29, far=True, ramp=True, plane=(3.0, 5.0, 256.0)):
    """the dense block [n, n] of sweep_coo, with two additions that make the found set depend on every blur's last bit:
    `far`: contacts beyond the distance limit too -- tested pixels (the mask is taken before the fills) inside the constant
    fill; `ramp` (blocks of 200 or more): the band's pixels in the upper half of the block lie on an exact plane
    1 + (3 row + 5 col) / 256.  A symmetric blur of a plane returns the plane, so away from the plane's border every DoG
    there is a difference of rounding errors that changes from pixel to pixel, and the sieve's comparisons (D_c against the
    3 x 3 maxima of D_p and D_n) are decided by them: that is how the first and the last level of an octave, which enter
    the sieve only through D_p and D_n, show up in the found set."""
    x, y, v = sweep_coo(n, dpx, seed)
    c = np.zeros((n, n))
    c[x, y] = v
    i, j = np.indices((n, n))
    if ramp and n >= 200:
        on = (j - i >= 5) & (j - i <= dpx) & (i < n // 2 + 15)
        c[on] = 1.0 + (plane[0] * i[on] + plane[1] * j[on]) / plane[2]
    if far:
        rng = np.random.default_rng(seed)
        fi, fj = np.nonzero(j - i >= dpx + 2)
        pick = rng.random(fi.size) < 0.5
        c[fi[pick], fj[pick]] = rng.uniform(0.2, 3.0, int(pick.sum()))
    return c


def block_from_band(slab, CH, dpx):
    """the dense block whose band (offsets 0 .. dpx + 1, diagonal-major, CH columns) is `slab`"""
    c = np.zeros((CH, CH))
    r = np.arange(CH)
    for d in range(min(dpx + 2, CH)):
        c[r[:CH - d], r[:CH - d] + d] = slab[d, :CH - d]
    return c


def reference_found(c, dpx, octaves, blur="scipy", perturb=None, keep_levels=False):
    """oracle.block_prologue + oracle.scale_space_levels on a copy of block c -> dict(nz, n_tested_pixels, pixel, level,
    value, pval, loc, scale, ss).  perturb = (level index, factor): that level's outermost tap times `factor` (the explicit
    blur only: SciPy computes its own taps)."""
    import oracle
    from oracle import scale_space as ssm
    c = c.copy()
    nz = oracle.block_prologue(c, dpx)
    orig = ssm.level_table
    if perturb is not None:
        assert blur == "explicit"

        def patched(octave_values, s=10):
            rows = orig(octave_values, s)
            w = rows[perturb[0]]["weights"].copy()
            w[0] *= perturb[1]
            w[-1] *= perturb[1]
            rows[perturb[0]]["weights"] = w
            return rows
        ssm.level_table = patched
    try:
        ss = oracle.scale_space_levels(c, nz, octaves, blur=blur, keep_levels=keep_levels)
    finally:
        ssm.level_table = orig
    hit = ss.pval != 2
    return dict(nz=nz, n_tested_pixels=int(nz.sum()), pixel=np.flatnonzero(nz.ravel())[hit], level=ss.level[hit],
                value=ss.best[hit], pval=ss.pval[hit], loc=np.array([t["loc"] for t in ss.tested]),
                scale=np.array([t["scale"] for t in ss.tested]), ss=ss, hit=hit)


def same_found(a, b):
    """two reference_found results agree in everything the sweep compares bitwise: found pixels, levels, values, loc"""
    return all(np.array_equal(a[k].view(np.int64) if a[k].dtype == np.float64 else a[k],
                              b[k].view(np.int64) if b[k].dtype == np.float64 else b[k])
               for k in ("pixel", "level", "value", "loc"))


def levels_struct(lt):
    st = lt.as_struct()
    return st, ctypes.byref(st)
