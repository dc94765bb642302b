"""The fused kernel outside its level loop -- staging, tested mask, state initialisation, epilogue -- on the tiles where its
paths part (mst_scale_space.hip): a workgroup without a tested pixel leaves through the epilogue's short path, a tested one
that found nothing behind the exchange of the wave totals, a wave without records before the record loop; the tested mask is
gathered from the flag bytes the three staging forms (constant, inner diagonal walk, border with reflection) wrote; shared
tiles deliver to two blocks; the wide tile reads its epilogue's arguments again and has no short path.

Every case runs the band and the dense source, with and without skip_empty, against oracle.block_prologue +
oracle.scale_space_levels(blur="scipy") (tests/radius_sweep.py, as test_gpu_radius_sweep.py and test_sieve_gate.py do):
tested-pixel counts exactly, pixels, levels and values with np.array_equal, loc exactly, scale to 1e-12, p-values to 1e-9.
Where MUSTACHE_HIP_LIB names another build of the library (the parent commit's), the package runs THAT one; the test then
loads the tree's own library beside it, runs both, holds both against the oracle and compares every output of the two bit for
bit (records in pixel order: the order of a block's records in its list is not a result).

Blocks of 140 x 140 to 300 x 300; what each block holds is asserted on the oracle before anything is launched
(test_inputs_on_the_oracle_alone does that without a GPU)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radius_sweep as rs      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE_LIB = os.path.join(ROOT, "mustache_amd", "libmustache_hip.so")
ITR, ITC = 30, 62               # pixels a tile owns (both tiles); the lattice is anchored at chromosome coordinate 0
OCTAVES = [1.6, 3.2]
WIDE_OCTAVES = [1.65, 3.3]      # largest radius 15: the wide tile, one above the default tile's 14


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _noise_block(n, dpx, seed, peaks):
    rng = np.random.default_rng(seed)
    i, j = np.indices((n, n))
    c = 1.0 + 0.3 * np.sin(0.31 * i + 0.17 * j) + rng.uniform(0.0, 0.4, (n, n))
    for (y, x, a, w) in peaks:
        c += a * np.exp(-((i - y) ** 2 + (j - x) ** 2) / (2.0 * w * w))
    c[(j - i < 0) | (j - i > dpx + 1)] = 0.0
    return c


@functools.lru_cache(maxsize=None)
def tiles_chromosome():
    """one block of 200 x 200, distance limit 150 (7 x 4 tiles), whose tiles are of every kind the epilogue tells apart:
    (0, 1) found records in all four waves; (1, 2) tested pixels in the columns of wave 1 only; (2, 2) two tested pixels on the
    slope of a peak that belongs to tile (2, 1) -- never a maximum, never found; below the diagonal no tested pixel"""
    n, dpx = 200, 150
    c = _noise_block(n, dpx, 5, [(20, 100, 6.0, 1.5), (52, 75, 5.0, 1.2), (75, 122, 9.0, 1.6), (100, 160, 6.0, 1.4),
                                 (125, 170, 5.0, 1.3), (8, 40, 5.0, 1.5)])
    c[30:60, 124:139] = 0.0
    c[30:60, 155:186] = 0.0
    keep = c[75:77, 124].copy()
    c[60:90, 124:186] = 0.0
    c[75:77, 124] = keep
    return c, n, dpx, [0], n


@functools.lru_cache(maxsize=None)
def overlap_chromosome():
    """two blocks of 300 x 300, half a block apart: the tiles inside both (halo included) are computed once"""
    n, dpx = 450, 200
    return _noise_block(n, dpx, 7, [(40, 100, 6.0, 1.5), (170, 260, 5.0, 1.2), (200, 330, 7.0, 1.6), (320, 420, 6.0, 1.4),
                                    (260, 300, 5.0, 1.3)]), n, dpx, [0, 150], 300


@functools.lru_cache(maxsize=None)
def end_chromosome():
    """two blocks of 140 x 140 on a chromosome of 200 bins: every block's first and last tiles reflect (border staging), the
    second block starts at 100 and the chromosome ends at its column 100, inside its second tile column.  Its second half is
    thinned to a few contacts: a block with few records behind one with many (the record-capacity case)"""
    n, dpx = 200, 100
    c = _noise_block(n, dpx, 9, [(20, 90, 6.0, 1.5), (52, 75, 5.0, 1.2), (90, 130, 7.0, 1.6), (150, 180, 6.0, 1.4)])
    rng = np.random.default_rng(10)
    thin = rng.uniform(0.0, 1.0, (n, n)) < 0.97
    thin[:100, :] = False
    c[thin] = 0.0
    return c, n, dpx, [0, 100], 140


CHROMOSOMES = {"tiles": tiles_chromosome, "overlap": overlap_chromosome, "end": end_chromosome}


def cut(c, start, CH):
    """the CH x CH block at `start` of chromosome c, zeros beyond the chromosome's end"""
    out = np.zeros((CH, CH))
    m = min(CH, c.shape[0] - start)
    out[:m, :m] = c[start:start + m, start:start + m]
    return out


@functools.lru_cache(maxsize=None)
def references(name, octaves=tuple(OCTAVES)):
    """the oracle on every block of a chromosome: computed once, shared by all tests, never changed"""
    c, n, dpx, starts, CH = CHROMOSOMES[name]()
    return [rs.reference_found(cut(c, s, CH), dpx, list(octaves)) for s in starts]


def tile_kinds(ref, CH):
    """{(tile row, tile column): (tested pixels, found records, waves with records)}: wave = region column // 16"""
    py, px = np.divmod(ref["pixel"], CH)
    out = {}
    for ty in range((CH + ITR - 1) // ITR):
        for tx in range((CH + ITC - 1) // ITC):
            sel = (py // ITR == ty) & (px // ITC == tx)
            out[(ty, tx)] = (int(ref["nz"][ty * ITR:(ty + 1) * ITR, tx * ITC:(tx + 1) * ITC].sum()), int(sel.sum()),
                             sorted(set(((px[sel] - (tx * ITC - 1)) // 16).tolist())))
    return out


def check_inputs():
    # the wide tile's region is the same 32 x 64 in 8 waves of 8 columns: waves 2 w and 2 w + 1 there are wave w here
    for octaves in (OCTAVES, WIDE_OCTAVES):
        kinds = tile_kinds(references("tiles", tuple(octaves))[0], 200)
        assert kinds[(0, 1)][2] == [0, 1, 2, 3], "found records in all four waves"
        assert kinds[(1, 2)][0] > 0 and kinds[(1, 2)][2] == [1], "found records in exactly one wave"
        assert kinds[(2, 2)][0] == 2 and kinds[(2, 2)][1] == 0, "tested pixels, no found record"
        assert kinds[(4, 0)] == (0, 0, []) and kinds[(6, 1)] == (0, 0, []), "no tested pixel"
    for name in CHROMOSOMES:
        for ref in references(name):
            assert len(ref["pixel"]) > 0 and np.isfinite(ref["value"]).all(), name
    busy, sparse = (len(r["pixel"]) for r in references("end"))
    assert sparse < CAP < busy and busy - CAP > sparse, "records past the cap of block 0 would land in block 1's free slots"
    assert len(references("tiles", tuple(WIDE_OCTAVES))[0]["pixel"]) > 0
    assert max(rs.level_table(WIDE_OCTAVES).radius) == 15 and max(rs.level_table(OCTAVES).radius) == 14


CAP = 64        # record capacity of the overflow case: between the two blocks' record counts (check_inputs)


def test_inputs_on_the_oracle_alone():
    check_inputs()


# ---- the libraries under test -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _engines(octaves):
    """[(name, engine)]: the library the package loaded; and, where MUSTACHE_HIP_LIB made that another build, the tree's own"""
    from mustache_amd import _lib
    from mustache_amd.engine import ScaleSpaceEngine
    out = [("package", ScaleSpaceEngine(list(octaves)))]
    if os.environ.get("MUSTACHE_HIP_LIB") and os.path.realpath(_lib.LIB_PATH) != os.path.realpath(TREE_LIB):
        lib = ctypes.CDLL(TREE_LIB)
        for sym, (res, args) in _lib._SIGNATURES.items():
            fn = getattr(lib, sym)
            fn.restype, fn.argtypes = res, args
        eng = ScaleSpaceEngine(list(octaves))
        eng.lib = lib
        out.append(("tree", eng))
    return out


def _band(c, n, dpx):
    import torch
    from mustache_amd.normalize import band_from_coo
    x, y = np.nonzero(c)
    return band_from_coo(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(c[x, y]).cuda(), n, dpx)


def _run(eng, source, chrom, skip_empty, band=None):
    """one launch over the chromosome's blocks -> per block (records, (loc, scale), tested pixels)"""
    import torch
    c, n, dpx, starts, CH = chrom
    nt = eng.levels.n_tested
    if source == "band":
        found, fits, nzc = eng.sigma_loop_band(_band(c, n, dpx) if band is None else band, n, dpx, starts, CH, skip_empty=skip_empty)
        counts = nzc.cpu().numpy().view(np.uint32)
    else:
        dev = torch.from_numpy(np.stack([cut(c, s, CH) for s in starts])).cuda()
        nz, nzc = eng.prologue(dev, dpx, True)
        found, fits = eng.sigma_loop(dev, nz, nzc, skip_empty=skip_empty)
        counts = nzc.cpu().numpy()
    return [({k: np.array(v) for k, v in found[b].items()}, (np.array(fits[b][0])[:nt], np.array(fits[b][1])[:nt]), int(counts[b]))
            for b in range(len(starts))]


def _against_oracle(got, ref, what):
    rec, (loc, scale), nzc = got
    assert nzc == ref["n_tested_pixels"], what
    assert np.array_equal(rec["pixel"].astype(np.int64), ref["pixel"]), what
    assert np.array_equal(rec["level"].astype(np.int64), ref["level"].astype(np.int64)), what
    assert np.array_equal(rec["value"], ref["value"]), what
    assert np.array_equal(loc, ref["loc"]), what
    np.testing.assert_allclose(scale, ref["scale"], rtol=1e-12, err_msg=str(what))
    np.testing.assert_allclose(rec["pval"], ref["pval"], rtol=1e-9, atol=0, err_msg=str(what))


def _same_bits(a, b, what):
    (ra, (la, sa), na), (rb, (lb, sb), nb) = a, b
    assert na == nb and sorted(ra) == sorted(rb), what
    for k in ra:
        assert ra[k].dtype == rb[k].dtype and ra[k].tobytes() == rb[k].tobytes(), (what, k)
    assert la.tobytes() == lb.tobytes() and sa.tobytes() == sb.tobytes(), what


def _check_case(name, source, skip_empty, octaves=tuple(OCTAVES)):
    chrom = CHROMOSOMES[name]()
    refs = references(name, octaves)
    runs = []
    for tag, eng in _engines(octaves):
        got = _run(eng, source, chrom, skip_empty)
        for b, ref in enumerate(refs):
            print("%s %s %s skip_empty=%d block %d: %d tested, %d found (oracle %d, %d)"
                  % (name, source, tag, skip_empty, b, got[b][2], len(got[b][0]["pixel"]), ref["n_tested_pixels"], len(ref["pixel"])))
            _against_oracle(got[b], ref, (name, source, tag, skip_empty, b))
        runs.append(got)
    for b in range(len(refs)):
        for other in runs[1:]:
            _same_bits(runs[0][b], other[b], (name, source, skip_empty, b))
    return len(runs)


SOURCES = [(s, e) for s in ("band", "dense") for e in (True, False)]
IDS = ["%s-%s" % (s, "skip_empty" if e else "all_tiles") for s, e in SOURCES]


@pytest.mark.gpu
@pytest.mark.parametrize("source,skip_empty", SOURCES, ids=IDS)
def test_every_kind_of_tile_in_one_launch(source, skip_empty):
    """no tested pixel; tested pixels but no record; records in one wave; records in all four waves"""
    check_inputs()
    _check_case("tiles", source, skip_empty)


@pytest.mark.gpu
@pytest.mark.parametrize("source,skip_empty", SOURCES, ids=IDS)
def test_two_overlapping_blocks(source, skip_empty):
    """band source: the tiles both blocks hold are computed once and delivered to b and b + 1"""
    c, n, dpx, starts, CH = overlap_chromosome()
    if source == "band":
        for _, eng in _engines(tuple(OCTAVES)):
            items, tiles, shared = eng.band_items(starts, CH, dpx, skip_empty=skip_empty, share=True)
            assert shared > 0 and items + shared == tiles
    _check_case("overlap", source, skip_empty)


@pytest.mark.gpu
@pytest.mark.parametrize("source,skip_empty", SOURCES, ids=IDS)
def test_border_tiles_and_the_chromosome_end_inside_a_tile(source, skip_empty):
    c, n, dpx, starts, CH = end_chromosome()
    assert starts[1] + CH > n and (n - starts[1]) % ITC != 0 and CH < 2 * 14 + 2 * ITC
    _check_case("end", source, skip_empty)


@pytest.mark.gpu
@pytest.mark.parametrize("source,skip_empty", SOURCES, ids=IDS)
def test_the_wide_tile_at_radius_15(source, skip_empty):
    assert rs.sigma_tile(rs.level_table(WIDE_OCTAVES)) == "wide"
    _check_case("tiles", source, skip_empty, tuple(WIDE_OCTAVES))


@pytest.mark.gpu
@pytest.mark.parametrize("source,skip_empty", SOURCES, ids=IDS)
def test_record_capacity_smaller_than_a_blocks_records(source, skip_empty):
    """ONE launch at a capacity of CAP records per block: block 0 finds more, block 1 fewer.  The overflow is reported (the
    finish raises MstOverflow; a block's count is its whole number of records, as without a cap), block 0's list holds CAP of
    its records, and block 1's list is complete with every slot behind its records untouched -- records of block 0 past the cap
    would land there.  The engine's own rule (four times the capacity, same launch again) then returns the full sets."""
    import torch
    from mustache_amd import _lib, launch
    check_inputs()
    chrom = c, n, dpx, starts, CH = end_chromosome()
    refs = references("end")
    for tag, eng in _engines(tuple(OCTAVES)):
        flags = launch.flags(eng, skip_empty, False)
        if source == "band":
            kw = dict(band_src=(_band(c, n, dpx), n, dpx, starts, CH))
        else:
            dev = torch.from_numpy(np.stack([cut(c, s, CH) for s in starts])).cuda()
            nz, nzc = eng.prologue(dev, dpx, True)
            kw = dict(blocks=(dev, nz), nzc=nzc)
        # the launch's buffers are kept under a reuse slot: fill the record lists with a sentinel, then launch into them again
        L = launch.ss_launch(eng, flags, found_cap=CAP, reuse=1, **kw)
        torch.cuda.synchronize()
        L.found.view(torch.uint8).fill_(0xA5)
        where = L.found.data_ptr()
        L = launch.enqueue(eng, L)
        assert L.found.data_ptr() == where, "the second launch writes the lists that hold the sentinel"
        with pytest.raises(_lib.MstOverflow):
            launch.finish(eng, L, relaunch=False)
        count = L.count.cpu().numpy().view(np.uint32)[:2]
        raw = L.found.cpu().numpy().view(np.uint8).reshape(2, CAP, -1)
        print("%s %s: counts %s at capacity %d (oracle %d, %d)" % (source, tag, count.tolist(), CAP, len(refs[0]["pixel"]), len(refs[1]["pixel"])))
        assert count.tolist() == [len(refs[0]["pixel"]), len(refs[1]["pixel"])]
        assert (raw[1, count[1]:] == 0xA5).all(), "nothing written past the cap of block 0"
        pix = raw[:, :, :4].copy().view(np.uint32)[:, :, 0]
        assert len(set(pix[0].tolist())) == CAP and set(pix[0].tolist()) <= set(refs[0]["pixel"].tolist())
        assert sorted(pix[1, :count[1]].tolist()) == refs[1]["pixel"].tolist()
        eng._found_cap.pop(CH, None)
        got = _run(eng, source, chrom, skip_empty)
        for b in range(2):
            _against_oracle(got[b], refs[b], ("after the overflow", source, tag, b))


@pytest.mark.gpu
@pytest.mark.parametrize("skip_empty", [True, False], ids=["skip_empty", "all_tiles"])
def test_two_bands_in_one_launch(skip_empty):
    """band2 / split: blocks [split, B) read the second sample's band (the two-sample call's launch), one block pair"""
    from mustache_amd import launch
    c1, n, dpx, _, CH = tiles_chromosome()
    c2 = _noise_block(n, dpx, 6, [(30, 90, 6.0, 1.5), (110, 150, 5.0, 1.2)])
    c2[60:90, 124:186] = 0.0
    refs = references("tiles") + [rs.reference_found(c2, dpx, OCTAVES)]
    runs = []
    for tag, eng in _engines(tuple(OCTAVES)):
        nt = eng.levels.n_tested
        L = launch.ss_launch(eng, launch.flags(eng, skip_empty, False), band_src=(_band(c1, n, dpx), n, dpx, [0, 0], CH),
                             band2=(_band(c2, n, dpx), 1))
        found, fits = eng._finish_results(L, (True, True, True, True, None))
        counts = L.nzc.cpu().numpy().view(np.uint32)
        got = [({k: np.array(v) for k, v in found[b].items()}, (np.array(fits[b][0])[:nt], np.array(fits[b][1])[:nt]), int(counts[b]))
               for b in range(2)]
        for b in range(2):
            _against_oracle(got[b], refs[b], ("two bands", tag, skip_empty, b))
        runs.append(got)
    for b in range(2):
        for other in runs[1:]:
            _same_bits(runs[0][b], other[b], ("two bands", skip_empty, b))
