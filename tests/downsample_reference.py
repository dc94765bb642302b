"""The thinning rule of mustache_amd/downsample.py restated in NumPy: Philox4x32-10 on uint64 arrays masked to 32 bits, the
draws addressed by (x, y, j), and the per-pixel count of kept reads.  Nothing here is shared with the package but zlib."""
import zlib

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """the four output words (uint64 arrays holding 32-bit values) of Philox4x32-10 for counters and keys given as arrays or
    integers, broadcast against each other"""
    c0, c1, c2, c3, k0, k1 = (np.asarray(a, dtype=np.uint64) & MASK for a in np.broadcast_arrays(c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2            # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return c0, c1, c2, c3


def chromosome_tag(chromosome):
    name = str(chromosome)
    return zlib.crc32((name[3:] if name.startswith("chr") else name).encode("utf-8")) & 0xFFFFFFFF


def draws(x, y, n, tag, seed, sample):
    """u_0 .. u_{n-1} of one pixel as a uint64 array"""
    calls = (int(n) + 3) // 4
    if calls == 0:
        return np.zeros(0, np.uint64)
    words = philox4x32_10(x, y, np.arange(calls, dtype=np.uint64), tag, seed, sample)
    return np.stack(words, axis=1).reshape(-1)[:int(n)]


def thin_counts(x, y, counts, tag, T, seed=0, sample=0):
    """k per pixel (int64) for pixels (x, y) with integer counts: one vectorised Philox pass over all reads of all pixels"""
    x, y, counts = np.asarray(x, np.int64), np.asarray(y, np.int64), np.asarray(counts, np.int64)
    assert 0 < int(T) < 1 << 32 and (counts >= 0).all() and (counts < 1 << 32).all()
    calls = (counts + 3) // 4
    owner = np.repeat(np.arange(len(counts)), calls)                 # the pixel of every Philox call
    first = np.cumsum(calls) - calls
    q = np.arange(int(calls.sum())) - first[owner]                   # the call's index within its pixel
    words = philox4x32_10(x[owner], y[owner], q, tag, seed, sample)
    k = np.zeros(len(counts), np.int64)
    for w, u in enumerate(words):
        kept = (u < np.uint64(T)) & (4 * q + w < counts[owner])      # the last call holds n & 3 reads when that is not 0
        k += np.bincount(owner, weights=kept, minlength=len(counts)).astype(np.int64)
    return k


def threshold_of(p):
    return int(float(p) * 4294967296.0)


def match_depth(n1, n2):
    """(T_1, T_2) of --match-depth: None for the sample left alone"""
    if n1 == n2:
        return None, None
    return (None, (n1 << 32) // n2) if n1 < n2 else ((n2 << 32) // n1, None)
