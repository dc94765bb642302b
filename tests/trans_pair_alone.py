"""A trans pair run ALONE on the device, independently of the batch body (mustache_amd/trans_genome.py) the product runs every
pair through: the expectation of the tests that say "every pair's rows equal the rows of that pair alone".

pair_alone / diff_pair_alone share no host step with PairBatcher before the launch body: the single-pair z-score
(mst_trans_zscore through trans.zscore_device) per sample, the extents from the records, trans_tiling, EVERY tile in groups
of `tiles_per_launch` -- no count, no skip rule, no work list --, mst_trans_scatter_tiles with each group's row0 / col0, then
trans.tile_loops / diff_trans.pair_tile_loops, the ownership filter and the sort.  Nothing is printed; a pair rule 2 leaves
nothing of (no record, a non-finite mean or std, std = 0, in either sample) gives []."""
import numpy as np

PAIRS_PER_LAUNCH = 32              # the two-sample default: tile PAIRS per launch (the one-sample default is 64 tiles)


def _normalized(eng, rec):
    """device (x int32, y int32, v') of one sample, or None where rule 2 leaves nothing to tile"""
    import torch
    from mustache_amd.trans import zscore_device
    x, y, v = rec
    if len(v) == 0:
        return None
    dev = eng.device
    x = torch.as_tensor(x).to(dev, dtype=torch.int32).contiguous()
    y = torch.as_tensor(y).to(dev, dtype=torch.int32).contiguous()
    vz, mean, std, _ = zscore_device(v, dev)
    if not (np.isfinite(mean) and np.isfinite(std)) or std == 0:
        return None
    return x, y, vz


def _groups(eng, samples, chunk, tiles_per_launch):
    """per launch group (tiling, group, B, C, fill): fill(s, c) scatters sample s's records into the group's B tiles c"""
    import torch
    from mustache_amd import _lib
    from mustache_amd.trans import _ptr, _stream, trans_tiling
    dev, lib = eng.device, eng.lib
    n1 = max(int(torch.max(s[0]).item()) for s in samples) + 1
    n2 = max(int(torch.max(s[1]).item()) for s in samples) + 1
    tiling = trans_tiling(n1, n2, chunk)
    C, (rs, _), (cs, _) = tiling
    tiles = [(i, j) for i in range(len(rs)) for j in range(len(cs))]
    for g0 in range(0, len(tiles), tiles_per_launch):
        group = tiles[g0:g0 + tiles_per_launch]
        B = len(group)
        row0 = torch.tensor([rs[i] for i, _ in group], dtype=torch.int64, device=dev)
        col0 = torch.tensor([cs[j] for _, j in group], dtype=torch.int64, device=dev)

        def fill(s, c, B=B, row0=row0, col0=col0):
            x, y, vz = samples[s]
            _lib.check(lib.mst_trans_scatter_tiles(_ptr(x), _ptr(y), _ptr(vz), int(vz.numel()), _ptr(row0), _ptr(col0), B, C,
                                                   _ptr(c), _stream()))
        yield tiling, group, B, C, fill


def pair_alone(x, y, v, oct, st, pt, chunk=2000, tiles_per_launch=64):
    """[[x, y, fdr, sigma], ...] of one sample's pair, sorted by (x, y): mustache_amd/trans.py rules 2-6"""
    from mustache_amd.mustache import _engine
    from mustache_amd.trans import owned_rows, tile_loops
    eng = _engine(oct)
    sample = _normalized(eng, (x, y, v))
    if sample is None:
        return []
    out = []
    for tiling, group, B, C, fill in _groups(eng, [sample], int(chunk), int(tiles_per_launch)):
        for (i, j), loops in zip(group, tile_loops(eng, eng.device, B, C, lambda c: fill(0, c), st, pt)):
            out += owned_rows(loops, tiling, i, j)
    out.sort(key=lambda r: (int(r[0]), int(r[1])))
    return out


def diff_pair_alone(rec1, rec2, oct, st, pt, pt2, chunk=2000, tiles_per_launch=PAIRS_PER_LAUNCH):
    """[[x, y, fdr, sigma, tag], ...] of two samples' pair, sorted by (tag, x, y): mustache_amd/diff_trans.py rules 2-5"""
    from mustache_amd.diff_trans import pair_tile_loops, row_order, tagged_owned_rows
    from mustache_amd.mustache import _engine
    eng = _engine(oct)
    samples = []
    for rec in (rec1, rec2):
        samples.append(_normalized(eng, rec))
        if samples[-1] is None:
            return []
    out = []
    for tiling, group, B, C, fill in _groups(eng, samples, int(chunk), int(tiles_per_launch)):
        for (i, j), res4 in zip(group, pair_tile_loops(eng, eng.device, B, C, fill, st, pt, pt2)):
            out += tagged_owned_rows(res4, tiling, i, j)
    out.sort(key=row_order)
    return out
