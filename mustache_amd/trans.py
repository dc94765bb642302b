"""Inter-chromosomal (trans) loop calling for one chromosome pair (A, B) on the GPU: the rules, the reader, and what one
launch of tiles runs.  The host path from records to rows is trans_genome.py's, for one pair (call_trans_coo: a batch of one)
as for many.

The reference's trans branch is dead code (mustache.py:939-942 calls inter_normalize_map with the wrong arguments and never
tiles), so the semantics are fixed here; tests/trans_reference.py restates them in NumPy / SciPy.

1. Input: every record of the A x B matrix, x = bin of A, y = bin of B, value > 0 and finite (readers.py / read_hic_trans).
2. Normalisation: over the N records, mean = sum v / N, std = sqrt(sum (v - mean)^2 / N), v' = (v - mean) / std, NaN / inf
   -> 0 (mst_trans_zscore; exact sums, bit-identical under record permutation).  N = 0 or std = 0: no loops.
3. Tiling: n1 = max(x) + 1, n2 = max(y) + 1, square tiles of C = min(2000, max(n1, n2)); per axis the reference's cis start
   formula with CHUNK = C and overlap 256 (trans_axis_tiles); tile (i, j) OWNS rows [end_{i-1}, end_i) and columns
   [end_{j-1}, end_j): every map pixel is owned by exactly one tile.  Cells outside the map are 0.
4. Per tile: nz = c != 0 over the whole tile (mst_trans_prologue: no triangle masks, no fills); the reference's sigma loop on
   nz (mst_scale_space, dense source); BH over the tile's found set, q < pt; fewer than 50 or 10 000 tested pixels: no loops;
   the cis sparsity filter (x != 0, the same window arithmetic); no diagonal-mean filter.
   The skip rule: a tile's tested pixels are its distinct pixels with v' != 0, never more than its records with v' != 0, so a
   tile whose window holds fewer than 10 000 such records (mst_trans_count_tiles) yields no loops and is dropped before it is
   scattered.  The rule never drops a tile that could report a loop; a tile it keeps still meets the thresholds in the tail.
5. Clustering: 8-connected components of the selected pixels each dilated by its 3 x 3 neighbourhood, clipped at the tile
   edges; the representative is the component's lowest q (o = q at found pixels, >= 1 elsewhere), ties to the first pixel in
   row-major order (mst_cluster_representatives does exactly this for any tile; its halo never wraps).  A representative
   is kept only if its tile owns it.
6. Output rows sorted by (x, y): [x, y, fdr, sigma] in map coordinates.
"""
import os

import numpy as np

from ._lib import ptr as _ptr, stream as _stream

TRANS_CHUNK = 2000
TRANS_OVERLAP = 256


class TransError(RuntimeError):
    """A trans request this package refuses (the CLI prints it as an `Error:` line)."""


def window_start(i, n, C, K, overlap=TRANS_OVERLAP):
    """where window i of the K windows of an axis of length n starts: i (C - 256), the last one at max(0, n - C)"""
    return i * (C - overlap) if i < K - 1 else max(0, n - C)


def trans_axis_tiles(n, chunk, overlap=TRANS_OVERLAP):
    """(start[], end[]) of one axis: the reference's cis tiling formula (mustache.py:896-910) with CHUNK = chunk, closed form."""
    n = int(n)
    if n <= chunk:
        return [0], [n]
    if chunk <= overlap:
        raise ValueError("trans tiles of %d bins cannot overlap by %d" % (chunk, overlap))
    K = 1 - (chunk - n) // (chunk - overlap)                      # 1 + ceil((n - chunk) / (chunk - overlap))
    start = [window_start(i, n, chunk, K, overlap) for i in range(K)]
    return start, [s + chunk for s in start[:-1]] + [n]


def trans_tiling(n1, n2, chunk=TRANS_CHUNK):
    """(C, rows, cols): tile size and the (start, end) lists of both axes."""
    C = min(int(chunk), max(int(n1), int(n2)))
    return C, trans_axis_tiles(n1, C), trans_axis_tiles(n2, C)


def zscore_device(v, device=None):
    """v' of rule 2 for a float64 device (or host) vector: (v', mean, std, n).  mean / std come back to the host."""
    import torch
    from . import _lib
    from ._lib import require_gpu
    lib = require_gpu()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    v = torch.as_tensor(v, dtype=torch.float64).to(dev).contiguous()
    out = torch.empty_like(v)
    stats = torch.empty(4, dtype=torch.float64, device=dev)
    ws_bytes = int(lib.mst_trans_zscore_workspace_bytes())
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.mst_trans_zscore(_ptr(v), int(v.numel()), _ptr(out), _ptr(stats), _ptr(ws), ws_bytes, _stream()))
    mean, std, n, _ = (float(a) for a in stats.cpu().numpy())
    return out, mean, std, int(v.numel())


def read_hic_trans(f, norm_method, chr_a, chr_b, res, device=None, slab_bytes=4 << 20, n_slabs=8, threads=0):
    """Every record of the (chr_a, chr_b) matrix of a `.hic` file as DEVICE tensors (x int32, y int32, v float64): the host
    inflates the zlib blocks (mst_hic_rawstream_open_trans), mst_trans_decode_hic_rows decodes the rows, divides by both
    normalisation vectors (KR by default) and transposes a pair the file stores as (chr_b, chr_a)."""
    import torch
    from . import _lib
    from ._lib import require_gpu
    from .hicfile import HicTransRawStream
    from .readers import _HIC_LOCK, _hic_handle
    lib = require_gpu()
    norm = "KR" if not norm_method else str(norm_method)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    pool = torch.empty(n_slabs * slab_bytes, dtype=torch.uint8, pin_memory=True)
    xs, ys, vs = [], [], []
    with _HIC_LOCK, torch.cuda.device(dev):
        h = _hic_handle(f)
        st = HicTransRawStream(h, chr_a, chr_b, res, norm, pool.data_ptr(), n_slabs, slab_bytes, threads=threads)
        try:
            na, nb, _, _ = st.info()
            d_na = None if na is None else torch.from_numpy(na).to(dev)
            d_nb = None if nb is None else torch.from_numpy(nb).to(dev)
            count = torch.zeros(1, dtype=torch.int64, device=dev)
            while True:
                got = st.next(-1)
                if got is False:
                    break
                if got is None:
                    continue
                slab, nbytes, rows = got
                base = slab * slab_bytes
                pay = pool[base:base + max(nbytes, 2)].to(dev)
                dr = pool[base + slab_bytes - 16 * rows:base + slab_bytes].to(dev)
                torch.cuda.current_stream().synchronize()           # the slab is free once its bytes are on the device
                st.release(slab)
                cap = nbytes // 2 + rows
                x = torch.empty(cap, dtype=torch.int32, device=dev)
                y = torch.empty(cap, dtype=torch.int32, device=dev)
                v = torch.empty(cap, dtype=torch.float64, device=dev)
                count.zero_()
                _lib.check(lib.mst_trans_decode_hic_rows(_ptr(pay), _ptr(dr), int(rows), _ptr(d_na), -1 if na is None else len(na),
                                                         _ptr(d_nb), -1 if nb is None else len(nb), 1 if st.transposed else 0,
                                                         _ptr(x), _ptr(y), _ptr(v), cap, _ptr(count), _stream()))
                k = int(count.item())
                if k > cap:
                    raise RuntimeError("mst_trans_decode_hic_rows: %d records in a slab of capacity %d" % (k, cap))
                xs.append(x[:k])
                ys.append(y[:k])
                vs.append(v[:k])
        finally:
            st.close()
    if not xs:
        z = torch.zeros(0, dtype=torch.int32, device=dev)
        return z, z.clone(), torch.zeros(0, dtype=torch.float64, device=dev)
    return torch.cat(xs), torch.cat(ys), torch.cat(vs)


def read_trans_contacts(f, norm_method, chr_a, chr_b, res, device=None):
    """(x, y, v, res) of the pair: `.hic` through read_hic_trans (device tensors), `.cool` / `.mcool` through cooler (host
    arrays); None when the pair has no record."""
    if f.endswith(".hic"):
        x, y, v = read_hic_trans(f, norm_method, chr_a, chr_b, res, device=device)
    elif f.endswith(".cool") or f.endswith(".mcool"):
        from .readers import read_cooler_trans
        x, y, v, res = read_cooler_trans(f, chr_a, chr_b, res, norm_method)
    else:
        from .request import TEXT_ON_TRANS
        raise TransError(TEXT_ON_TRANS)
    if len(v) == 0:
        return None
    return x, y, v, res


def tiles_per_launch_of(tiles_per_launch=None):
    """the tiles of one launch: the caller's number, else MUSTACHE_TRANS_TILES, else 64"""
    return int(tiles_per_launch or os.environ.get("MUSTACHE_TRANS_TILES", "64"))


def prepared_tiles(eng, dev, B, C, fill):
    """(c, nz, nzc) of B tiles of C on `dev`: c [B, C, C] float64 as `fill(c)`, the caller's scatter, leaves it; nz = c != 0
    and its count per tile (mst_trans_prologue: rule 4's first clause)"""
    import torch
    from . import _lib
    c = torch.empty((B, C, C), dtype=torch.float64, device=dev)
    nz = torch.empty((B, C, C), dtype=torch.uint8, device=dev)
    nzc = torch.empty(B, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        fill(c)
        _lib.check(eng.lib.mst_trans_prologue(_ptr(c), _ptr(nz), _ptr(nzc), B, C, _stream()))
    return c, nz, nzc


def tile_loops(eng, dev, B, C, fill, st, pt):
    """Rules 4-5 on the B tiles of one launch: one scatter (`fill`), one prologue, one fused scale-space launch
    (mst_scale_space over dense tiles) and one batched tail.  Per tile its loops [x, y, fdr, sigma] in TILE coordinates."""
    import torch
    from .batches import BlockBatch
    from .tail import batch_tail
    c, nz, nzc = prepared_tiles(eng, dev, B, C, fill)
    with torch.cuda.device(dev):
        found, fits = eng.sigma_loop(c, nz, nzc, with_value=False, select_below=pt)
    batch = BlockBatch(eng, c, nz, C, B, nzc, found, fits)
    return batch_tail(batch, list(range(B)), [0] * B, pt, st, intra=False)


def owned_rows(loops, tiling, i, j):
    """the map rows [x, y, fdr, sigma] of tile (i, j)'s loops (tile coordinates) that the tile owns (rule 3; end_{-1} = 0)"""
    _, (rs, re), (cs, ce) = tiling
    rlo, clo = (re[i - 1] if i else 0), (ce[j - 1] if j else 0)
    out = []
    for lx, ly, q, sg in loops:
        gx, gy = int(lx) + rs[i], int(ly) + cs[j]
        if rlo <= gx < re[i] and clo <= gy < ce[j]:
            out.append([np.int64(gx), np.int64(gy), q, sg])
    return out


def call_trans_coo(x, y, v, octave_values, st, pt, verbose=False, label="", tiles_per_launch=None, chunk=TRANS_CHUNK):
    """Loops of one chromosome pair from its records (x = bins of A, y = bins of B, v > 0; host arrays or device tensors, which
    are not written): rules 2-6 of this module, as a batch of one pair (trans_genome.PairBatcher.run_pair).
    Returns [[x, y, fdr, sigma], ...] sorted by (x, y)."""
    from .trans_genome import TransGenomeCaller
    caller = TransGenomeCaller(octave_values, st, pt, None, chunk=chunk, tiles_per_launch=tiles_per_launch, verbose=verbose)
    return caller.run_pair([(x, y, v)], label)
