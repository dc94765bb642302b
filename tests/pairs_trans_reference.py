"""The trans half of the rule of mustache_amd/pairs.py restated in plain Python and NumPy: a 4DN pairs file -> the stored trans
rows per chromosome pair and their counters, rows -> per-pair pixels with exact counts; and the way back, a genome of integer
counts -> pairs text.  Shares no code with the package (the line grammar is tests/pairs_reference.py's)."""
import gzip

import numpy as np

import pairs_reference as pr


def pair_list(n):
    return [(a, b) for a in range(n) for b in range(a + 1, n)]


def side_in_range(pos, length, zero_based):
    pos = np.asarray(pos, np.int64)
    lo = 0 if zero_based else 1
    keep = pos >= lo
    if length is not None and length >= 0:
        keep &= pos <= (length - 1 if zero_based else length)
    return keep


def parse_trans(path, zero_based=False):
    """-> {"chromosomes": [(name, length)], "rows": {(a, b): (posA, posB) int32 arrays in file order} for EVERY pair of the table,
    "seg_off": int64 [P + 1], "out_of_range": int64 [P], "counters": {"stored", "out_of_range", "unknown"}, "trans": all trans
    rows of the file}.  A file without `#chromsize` lines raises ValueError."""
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rb") as fh:
        lines = fh.read().decode("utf-8", "surrogateescape").split("\n")
    names, lengths, cols = [], {}, {"chr1": 1, "pos1": 2, "chr2": 3, "pos2": 4}
    in_header, body = True, []
    for line in lines:
        if line.endswith("\r"):
            line = line[:-1]
        f = pr._fields(line)
        if line.startswith("#"):
            if in_header and f[0] == "#chromsize:" and f[1] not in lengths:
                names.append(f[1])
                lengths[f[1]] = int(f[2])
            elif in_header and f[0] == "#columns:":
                cols = {c: f[1:].index(c) for c in cols}
            continue
        if f:
            in_header = False
            body.append(f)
    if not names:
        raise ValueError("no #chromsize line")
    index = {n: i for i, n in enumerate(names)}
    pairs = pair_list(len(names))
    rows = {p: ([], []) for p in pairs}
    trans = unknown = 0
    for f in body:
        c1, c2 = f[cols["chr1"]], f[cols["chr2"]]
        if c1 == c2:
            continue
        trans += 1
        if c1 not in index or c2 not in index:
            unknown += 1
            continue
        a, b = pr._position(f[cols["pos1"]]), pr._position(f[cols["pos2"]])
        i, j = index[c1], index[c2]
        if i > j:
            i, j, a, b = j, i, b, a
        rows[(i, j)][0].append(a)
        rows[(i, j)][1].append(b)
    out, seg, oor = {}, [0], []
    for (i, j) in pairs:
        pa, pb = (np.array(r, dtype=np.int64).astype(np.int32) for r in rows[(i, j)])
        out[(i, j)] = (pa, pb)
        seg.append(seg[-1] + len(pa))
        keep = side_in_range(pa, lengths[names[i]], zero_based) & side_in_range(pb, lengths[names[j]], zero_based)
        oor.append(int((~keep).sum()))
    return {"chromosomes": [(n, lengths[n]) for n in names], "rows": out, "seg_off": np.array(seg, np.int64),
            "out_of_range": np.array(oor, np.int64).reshape(-1),
            "counters": {"stored": seg[-1], "out_of_range": int(sum(oor)), "unknown": unknown}, "trans": trans}


def pair_pixels(posA, posB, res, zero_based, lim_a, lim_b, n_a, n_b):
    """one pair's rows -> ({(x, y): count}, dropped): each side judged by its own limit (negative or None: none), then by its
    bin count"""
    pa, pb = np.asarray(posA, np.int64), np.asarray(posB, np.int64)
    keep = side_in_range(pa, lim_a, zero_based) & side_in_range(pb, lim_b, zero_based)
    lo = 0 if zero_based else 1
    x, y = (pa - lo) // res, (pb - lo) // res
    keep &= (x < n_a) & (y < n_b)
    out = {}
    for k in zip(x[keep].tolist(), y[keep].tolist()):
        out[k] = out.get(k, 0) + 1
    return out, int((~keep).sum())


def pair_keys(posA, posB, res, zero_based, lim_a, lim_b, n_a, n_b):
    """pair_pixels for millions of rows, NumPy only: one pair's rows -> (the ascending unique local cells x * n_b + y int64,
    their counts int64, dropped).  The rule of mustache_amd/pairs.py once more: each side in [lo, limit] (0-based: [0, limit)),
    bin = (pos - lo) // res, a bin >= its side's bin count drops the row."""
    pa, pb = np.asarray(posA, np.int64), np.asarray(posB, np.int64)
    lo = 0 if zero_based else 1
    keep = np.ones(len(pa), bool)
    for pos, lim, n in ((pa, lim_a, n_a), (pb, lim_b, n_b)):
        keep &= pos >= lo
        if lim is not None and lim >= 0:
            keep &= pos < lim + lo
        keep &= (pos - lo) // res < n
    cells, counts = np.unique((pa[keep] - lo) // res * n_b + (pb[keep] - lo) // res, return_counts=True)
    return cells.astype(np.int64), counts.astype(np.int64), int(len(pa) - keep.sum())


def genome_pixels(parsed, res, zero_based=False):
    """parse_trans's result -> ({(a, b): {(x, y): count}} of the pairs that have a pixel, dropped int64 [P]); a chromosome has
    length // res + 1 bins"""
    lengths = [length for _, length in parsed["chromosomes"]]
    out, dropped = {}, []
    for (a, b), (pa, pb) in parsed["rows"].items():
        px, d = pair_pixels(pa, pb, res, zero_based, lengths[a], lengths[b], lengths[a] // res + 1, lengths[b] // res + 1)
        dropped.append(d)
        if px:
            out[(a, b)] = px
    return out, np.array(dropped, np.int64).reshape(-1)


def records_to_pixels(x, y, v):
    """(x, y, v) arrays -> {(x, y): count}; the records must be unique and their counts integers"""
    x, y, v = (np.asarray(t) for t in (x, y, v))
    assert np.all(v == np.round(v)) and np.all(v > 0)
    out = dict(zip(zip(x.tolist(), y.tolist()), v.astype(np.int64).tolist()))
    assert len(out) == len(x), "a pixel appears twice"
    return out


def pairs_text(names, lengths, res, cis, trans, seed, extras=True):
    """A genome of integer counts -> pairs text: one row per contact with a random 1-based position inside its bin (within the
    chromosome's length), either row orientation, all rows shuffled.  cis: {c: (x, y, count)}, trans: {(a, b): (x, y, count)}
    (indices into names).  extras: rows that change no pixel are mixed in -- `chrM` rows (cis and trans: the header does not name
    it) and out-of-range rows (cis; trans on the a side only and on the b side only).  -> (text, data rows)"""
    rng = np.random.default_rng(seed)
    head = "## pairs format v1.0\n" + "".join("#chromsize: %s %d\n" % (n, l) for n, l in zip(names, lengths)) + \
           "#columns: readID chr1 pos1 chr2 pos2 strand1 strand2\n"
    c1, c2, p1, p2 = [], [], [], []
    blocks = [((c, c), rec) for c, rec in cis.items()] + list(trans.items())
    for (ca, cb), (x, y, v) in blocks:
        reps = np.asarray(v).astype(np.int64)
        assert np.all(reps == np.asarray(v))
        bx, by = np.repeat(np.asarray(x, np.int64), reps), np.repeat(np.asarray(y, np.int64), reps)
        a = rng.integers(bx * res + 1, np.minimum((bx + 1) * res, lengths[ca]) + 1)
        b = rng.integers(by * res + 1, np.minimum((by + 1) * res, lengths[cb]) + 1)
        swap = rng.random(len(a)) < 0.5
        p1.append(np.where(swap, b, a))
        p2.append(np.where(swap, a, b))
        c1.append(np.where(swap, cb, ca))
        c2.append(np.where(swap, ca, cb))
    c1, c2, p1, p2 = (np.concatenate(t) for t in (c1, c2, p1, p2))
    order = rng.permutation(len(p1))
    lines = ["r\t%s\t%d\t%s\t%d\t+\t-\n" % (names[i], a, names[j], b)
             for i, a, j, b in zip(c1[order].tolist(), p1[order].tolist(), c2[order].tolist(), p2[order].tolist())]
    if extras:
        extra = ["m\tchrM\t5\tchrM\t9\t+\t-\n", "m\t%s\t7\tchrM\t9\t+\t-\n" % names[0], "m\tchrM\t7\t%s\t9\t+\t-\n" % names[1],
                 "o\t%s\t0\t%s\t5\t+\t-\n" % (names[0], names[0]),
                 "o\t%s\t%d\t%s\t5\t+\t-\n" % (names[0], lengths[0] + 1, names[1]),        # out of range on the a side only
                 "o\t%s\t5\t%s\t%d\t+\t-\n" % (names[1], names[0], lengths[0] + 1),        # the same, named the other way round
                 "o\t%s\t5\t%s\t%d\t+\t-\n" % (names[0], names[1], lengths[1] + 1),        # on the b side only
                 "o\t%s\t5\t%s\t99999999999\t+\t-\n" % (names[0], names[-1])]              # beyond int32
        for k, e in enumerate(extra):
            lines.insert((k + 1) * len(lines) // (len(extra) + 1), e)
    return head + "".join(lines), len(lines)
