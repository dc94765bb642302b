"""Test infrastructure: `.hic` files (versions 8 and 9) with inter-chromosomal matrices, built on tests/hic_writer.py's block
encoders.  A matrix is keyed by the pair of chromosome indices in the order the file stores it; the published layout keys a
pair by the lower index first, and `swap=True` writes it the other way round as well (the reader must then transpose).

write_hic_pairs(path, chroms, matrices, norms, version)
    chroms   : [(name, length)], index 0 = ("All", ...)
    matrices : {(c1, c2): {resolution: (x, y, counts)}} -- x = bins of chromosome c1, y = bins of chromosome c2 (c1 == c2:
               an intra matrix, x <= y)
    norms    : {(type, chrom_index, resolution): vector}
"""
import struct
import zlib

import numpy as np

from hic_writer import _block_v8, _block_v9, _s


def write_hic_pairs(path, chroms, matrices, norms=None, version=8, block_bin_count=64, float_counts=True, dense_blocks=False,
                    short_coords=True):
    assert version in (8, 9)
    norms = norms or {}
    v9 = version == 9
    body = bytearray()
    body += _s("HIC") + struct.pack("<i", version) + struct.pack("<q", 0) + _s("synthetic")
    nvi_at = None
    if v9:
        nvi_at = len(body)
        body += struct.pack("<qq", 0, 0)
    body += struct.pack("<i", 1) + _s("software") + _s("tests/hic_trans_writer.py")
    body += struct.pack("<i", len(chroms))
    for name, length in chroms:
        body += _s(name) + (struct.pack("<q", length) if v9 else struct.pack("<i", length))
    all_res = sorted({r for m in matrices.values() for r in m}, reverse=True)
    body += struct.pack("<i", len(all_res)) + b"".join(struct.pack("<i", r) for r in all_res)
    body += struct.pack("<i", 0)

    master = {}
    for (c1, c2), per_res in matrices.items():
        zooms = []
        for zi, res in enumerate(sorted(per_res, reverse=True)):
            x, y, cnt = (np.asarray(a) for a in per_res[res])
            nbins = max(chroms[c1][1], chroms[c2][1]) // res + 1
            bcc = nbins // block_bin_count + 1
            groups = {}
            for xi, yi, c in zip(x.tolist(), y.tolist(), cnt.tolist()):
                bn = (yi // block_bin_count) * bcc + (xi // block_bin_count)      # the grid numbering of trans matrices
                groups.setdefault(bn, []).append((xi, yi, c))
            blocks = []
            for bn in sorted(groups):
                recs = groups[bn]
                x_off, y_off = min(r[0] for r in recs), min(r[1] for r in recs)
                raw = (_block_v9(recs, x_off, y_off, float_counts, short_coords, short_coords) if v9
                       else _block_v8(recs, x_off, y_off, float_counts, dense_blocks))
                comp = zlib.compress(raw)
                blocks.append((bn, len(body), len(comp)))
                body += comp
            zooms.append((res, zi, bcc, blocks))
        pos = len(body)
        body += struct.pack("<iii", c1, c2, len(zooms))
        for res, zi, bcc, blocks in zooms:
            body += _s("BP") + struct.pack("<i", zi) + struct.pack("<ffff", 0, 0, 0, 0)
            body += struct.pack("<iiii", res, block_bin_count, bcc, len(blocks))
            for bn, bpos, bsize in blocks:
                body += struct.pack("<iqi", bn, bpos, bsize)
        master["%d_%d" % (c1, c2)] = (pos, len(body) - pos)

    norm_pos = {}
    for key, vec in norms.items():
        vec = np.asarray(vec, dtype=np.float64)
        p = len(body)
        if v9:
            body += struct.pack("<q", len(vec)) + vec.astype("<f4").tobytes()
        else:
            body += struct.pack("<i", len(vec)) + vec.astype("<f8").tobytes()
        norm_pos[key] = (p, len(body) - p)

    master_at = len(body)
    foot = bytearray()
    foot += struct.pack("<i", len(master))
    for k, (p, sz) in master.items():
        foot += _s(k) + struct.pack("<qi", p, sz)
    foot += struct.pack("<i", 0) + struct.pack("<i", 0)                  # no expected-value vectors
    nbytes_field = 8 if v9 else 4
    nvi_pos = master_at + nbytes_field + len(foot)
    nvi = bytearray(struct.pack("<i", len(norm_pos)))
    for (typ, ci, res), (p, sz) in norm_pos.items():
        nvi += _s(typ) + struct.pack("<i", ci) + _s("BP") + struct.pack("<i", res) + struct.pack("<q", p)
        nvi += struct.pack("<q", sz) if v9 else struct.pack("<i", sz)
    foot += nvi
    body += (struct.pack("<q", len(foot)) if v9 else struct.pack("<i", len(foot))) + foot
    struct.pack_into("<q", body, 8, master_at)
    if v9:
        struct.pack_into("<qq", body, nvi_at, nvi_pos, len(nvi))
    with open(path, "wb") as fh:
        fh.write(bytes(body))


def expected_trans(x, y, counts, norm_a=None, norm_b=None):
    """What a trans read of the pair (A, B) must return, restated: straw's value (float32 of count / (normA[x] * normB[y]) in
    double), records with a NaN, inf or non-positive value dropped.  x = bins of A, y = bins of B.  Sorted by (x, y)."""
    x = np.asarray(x, np.int64)
    y = np.asarray(y, np.int64)
    c = np.asarray(counts, np.float32).astype(np.float64)
    if norm_a is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            c = (c / (np.asarray(norm_a, np.float64)[x] * np.asarray(norm_b, np.float64)[y])).astype(np.float32).astype(np.float64)
    keep = np.isfinite(c) & (c > 0)
    x, y, c = x[keep], y[keep], c[keep]
    o = np.lexsort((y, x))
    return x[o], y[o], c[o]
