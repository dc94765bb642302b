"""The rule of mustache_amd/pairs.py restated in plain Python and NumPy: a 4DN pairs file -> per-chromosome rows and counters,
rows -> pixels with exact counts.  Shares no code with the package."""
import gzip
import re

import numpy as np

_INT = re.compile(r"[+-]?[0-9]+\Z")
_SPLIT = re.compile(r"[ \t]+")
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


class PairsFormatError(ValueError):
    def __init__(self, line, what):
        super().__init__("line %d: %s" % (line, what))
        self.line = line


def _fields(line):
    return [f for f in _SPLIT.split(line) if f]


def _position(tok):
    if not _INT.match(tok):
        return None
    v = int(tok)
    return v if I32_MIN <= v <= I32_MAX else I32_MIN        # not an int32: out of range by definition


def parse_pairs(path, zero_based=False):
    """-> {"chromosomes": [(name, length or -1)], "rows": {name: (pos1, pos2) int32 arrays in file order},
    "out_of_range": {name: count}, "counters": {"rows", "kept", "trans", "out_of_range", "unknown"}}"""
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rb") as fh:
        lines = fh.read().decode("utf-8", "surrogateescape").split("\n")
    names, lengths, cols = [], {}, {"chr1": 1, "pos1": 2, "chr2": 3, "pos2": 4}
    fixed, in_header = False, True
    rows, counters = {}, {"rows": 0, "kept": 0, "trans": 0, "out_of_range": 0, "unknown": 0}
    lo = 0 if zero_based else 1
    for number, line in enumerate(lines, 1):
        if line.endswith("\r"):
            line = line[:-1]
        if line.startswith("#"):
            f = _fields(line)
            if in_header and f[0] == "#chromsize:":
                if len(f) < 3 or _position(f[2]) is None or _position(f[2]) < 0:
                    raise PairsFormatError(number, "a #chromsize: line without a name and a length")
                fixed = True
                if f[1] not in lengths:
                    names.append(f[1])
                    lengths[f[1]] = int(f[2])
            elif in_header and f[0] == "#columns:":
                for c in cols:
                    if c not in f[1:]:
                        raise PairsFormatError(number, "a #columns: line without %s" % c)
                    cols[c] = f[1:].index(c)
            continue
        f = _fields(line)
        if not f:
            continue
        in_header = False
        need = max(cols.values()) + 1
        if len(f) < need:
            raise PairsFormatError(number, "too few fields")
        a, b = _position(f[cols["pos1"]]), _position(f[cols["pos2"]])
        if a is None or b is None:
            raise PairsFormatError(number, "a position that is not a decimal integer")
        counters["rows"] += 1
        c1, c2 = f[cols["chr1"]], f[cols["chr2"]]
        if not fixed:
            for c in (c1, c2):
                if c not in lengths:
                    names.append(c)
                    lengths[c] = -1
        if c1 != c2:
            counters["trans"] += 1
            continue
        if c1 not in lengths:
            counters["unknown"] += 1
            continue
        rows.setdefault(c1, []).append((a, b))
    out_rows, out_oor = {}, {}
    for name in names:
        r = np.array(rows.get(name, []), dtype=np.int64).reshape(-1, 2)
        p1, p2 = r[:, 0].astype(np.int32), r[:, 1].astype(np.int32)
        keep = in_range(p1, p2, lengths[name], zero_based)
        out_rows[name], out_oor[name] = (p1, p2), int((~keep).sum())
        counters["out_of_range"] += out_oor[name]
        counters["kept"] += int(keep.sum())
    return {"chromosomes": [(n, lengths[n]) for n in names], "rows": out_rows, "out_of_range": out_oor, "counters": counters}


def in_range(pos1, pos2, length, zero_based):
    """the rows that are kept: both positions >= 1 and <= length (zero_based: >= 0 and < length); length < 0 or None: no upper limit"""
    p1, p2 = np.asarray(pos1, np.int64), np.asarray(pos2, np.int64)
    lo = 0 if zero_based else 1
    keep = (p1 >= lo) & (p2 >= lo)
    if length is not None and length >= 0:
        hi = length - 1 if zero_based else length
        keep &= (p1 <= hi) & (p2 <= hi)
    return keep


def pixels(pos1, pos2, res, zero_based=False, length=None):
    """rows -> (x, y, count, dropped): the unique pixels sorted by (x, y) with their exact counts, and the rows out of range"""
    p1, p2 = np.asarray(pos1, np.int64), np.asarray(pos2, np.int64)
    keep = in_range(p1, p2, length, zero_based)
    lo = 0 if zero_based else 1
    b1, b2 = (p1[keep] - lo) // res, (p2[keep] - lo) // res
    x, y = np.minimum(b1, b2), np.maximum(b1, b2)
    if len(x) == 0:
        z = np.zeros(0, np.int64)
        return z, z.copy(), z.copy(), int((~keep).sum())
    width = int(y.max()) + 1
    key, count = np.unique(x * width + y, return_counts=True)
    return key // width, key % width, count.astype(np.int64), int((~keep).sum())
