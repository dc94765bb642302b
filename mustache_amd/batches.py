"""What the host tail works on: the records of one group of blocks plus the small device gathers the tail asks for
(candidate features, diagonals, clustering), block-batched."""
import numpy as np
import torch

from . import _lib
from ._lib import off as _off, ptr as _ptr, stream as _stream


def host_counts(nz_count):
    """Tested-pixel counts per block as the batches keep them (int64 host array), from whatever a launch handed out: a
    device or host int32 tensor (the kernels' uint32 counters), a NumPy array, or None (a batch built for its gathers
    only)."""
    if isinstance(nz_count, torch.Tensor):
        return nz_count.cpu().numpy().view(np.uint32).astype(np.int64)
    return nz_count


class _MultiGather:
    """Block-batched forms of the tail's gathers: ONE upload of the concatenated candidates, one launch per block on the
    same stream (pointer offsets into the shared buffers), ONE download -- instead of a host round trip per block."""

    def candidate_features_multi(self, bs, pixels, halfs):
        sizes = [int(len(p)) for p in pixels]
        total = sum(sizes)
        empty = (np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0))
        if total == 0:
            return [empty for _ in bs]
        dev = self._device()
        pix = np.concatenate([np.asarray(p, dtype=np.uint32) for p in pixels])
        half = np.concatenate([np.asarray(h, dtype=np.int32) for h in halfs])
        d_pix = torch.from_numpy(pix.view(np.int32)).to(dev)
        d_half = torch.from_numpy(half).to(dev)
        cnt = torch.empty((2, total), dtype=torch.int32, device=dev)
        cval = torch.empty(total, dtype=torch.float64, device=dev)
        if not self._features_one_launch(bs, sizes, d_pix, d_half, total, cnt, cval):
            off = 0
            for b, m in zip(bs, sizes):
                if m:
                    self._features_launch(b, _off(d_pix, off), _off(d_half, off), m, _off(cnt, off), _off(cnt,
                                          total + off), _off(cval, off))
                off += m
        cnt_h = cnt.cpu().numpy().view(np.uint32)
        cval_h = cval.cpu().numpy()
        out, off = [], 0
        for m in sizes:
            out.append((cnt_h[0, off:off + m], cnt_h[1, off:off + m], cval_h[off:off + m]) if m else empty)
            off += m
        return out

    def diagonals_multi(self, bs, kss):
        sizes = [int(len(k)) for k in kss]
        total = sum(sizes)
        if total == 0:
            return [np.zeros((0, self.CH)) for _ in bs]
        dev = self._device()
        d_k = torch.from_numpy(np.concatenate([np.asarray(k, dtype=np.int32) for k in kss])).to(dev)
        out = torch.empty((total, self.CH), dtype=torch.float64, device=dev)
        off = 0
        for b, m in zip(bs, sizes):
            if m:
                self._diagonals_launch(b, _off(d_k, off), m, _off(out, off * self.CH))
            off += m
        host = self.engine.staging.pinned("diags", (total, self.CH), torch.float64)
        host.copy_(out, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        host = host.numpy()
        res, off = [], 0
        for m in sizes:
            res.append(host[off:off + m])
            off += m
        return res

    def diagonal_means_multi(self, bs, kss):
        """Per block the mean of the non-zero entries of its diagonals kss[i] (np.mean(dg[dg != 0]),
        mustache.py:816-820), computed on the device in NumPy's summation order -- bit-identical, and only one double
        per diagonal comes back."""
        sizes = [int(len(k)) for k in kss]
        total = sum(sizes)
        if total == 0:
            return [np.zeros(0) for _ in bs]
        dev = self._device()
        d_k = torch.from_numpy(np.concatenate([np.asarray(k, dtype=np.int32) for k in kss])).to(dev)
        out = torch.empty(total, dtype=torch.float64, device=dev)
        if not self._diag_means_one_launch(bs, sizes, d_k, out):
            off = 0
            for b, m in zip(bs, sizes):
                if m:
                    self._diag_means_launch(b, _off(d_k, off), m, _off(out, off))
                off += m
        host = out.cpu().numpy()
        res, off = [], 0
        for m in sizes:
            res.append(host[off:off + m])
            off += m
        return res

    def _diag_means_one_launch(self, bs, sizes, d_k, out):
        return False                        # overridden where all blocks share one source buffer

    def _features_one_launch(self, bs, sizes, d_pix, d_half, total, cnt, cval):
        return False                        # overridden where all blocks share one source buffer

    def cluster_representatives_multi(self, bs, qs, idxs, pt):
        """Clustering of the surviving candidates of several blocks (mustache.py:830-848) in ONE launch
        (mst_cluster_representatives): per block the record indices of the components' representatives, in the
        reference's label order.  qs[i]: q per record of block bs[i]; idxs[i]: ascending record indices of its
        candidates.  Only records with q < pt can be a component's arg-min (o >= 1 everywhere else), so those are what
        is uploaded."""
        out = [[] for _ in bs]
        sel_pix, sel_q, sel_off, cand_pos, cand_off, back = [], [], [0], [], [0], []
        for b, q, idx in zip(bs, qs, idxs):
            rec = self.found[b]
            idx = np.asarray(idx, dtype=np.int64)
            below = np.nonzero(q < pt)[0]
            if len(idx) and not np.all(q[idx] < pt):
                raise ValueError("cluster_representatives_multi: a candidate with q >= pt")
            sel_pix.append(rec["pixel"][below].astype(np.uint32))
            sel_q.append(np.ascontiguousarray(q[below], dtype=np.float64))
            sel_off.append(sel_off[-1] + len(below))
            cand_pos.append(np.searchsorted(below, idx).astype(np.uint32))
            cand_off.append(cand_off[-1] + len(idx))
            back.append(below)
        total_c = cand_off[-1]
        if total_c == 0:
            return out
        dev = self._device()
        lib = self.engine.lib
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)
        d_pix = up(np.concatenate(sel_pix) if sel_off[-1] else np.zeros(1, np.uint32), np.int32)
        d_q = up(np.concatenate(sel_q) if sel_off[-1] else np.zeros(1), np.float64)
        d_soff = up(np.asarray(sel_off, dtype=np.uint32), np.int32)
        d_cpos = up(np.concatenate(cand_pos), np.int32)
        d_coff = up(np.asarray(cand_off, dtype=np.uint32), np.int32)
        d_rep = torch.empty(total_c, dtype=torch.int32, device=dev)
        d_cnt = torch.empty(len(bs), dtype=torch.int32, device=dev)
        ws_bytes = int(lib.mst_cluster_workspace_bytes(total_c))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.mst_cluster_representatives(_ptr(d_pix), _ptr(d_q), _ptr(d_soff), _ptr(d_cpos), _ptr(d_coff),
                                                       len(bs), int(self.CH), total_c, _ptr(d_rep), _ptr(d_cnt),
                                                       _ptr(ws), ws_bytes, _stream()))
        rep = d_rep.cpu().numpy().view(np.uint32)
        cnt = d_cnt.cpu().numpy().view(np.uint32)
        for i in range(len(bs)):
            r = rep[cand_off[i]:cand_off[i] + int(cnt[i])]
            out[i] = [int(v) for v in back[i][r]]
        return out

    def candidate_features(self, b, pixel, half):
        """(cnt1, cnt2, cval) for candidate pixels of block b (reference mustache.py:800-807, :824)."""
        return self.candidate_features_multi([b], [pixel], [half])[0]

    def diagonals(self, b, ks):
        """Rows = diagonals c[r, r+k] of block b, zero padded to CH (reference mustache.py:816-820)."""
        return self.diagonals_multi([b], [ks])[0].copy()      # the multi form hands out views of a reused pinned buffer


class BlockBatch(_MultiGather):
    """Results of the sigma loop for B blocks, plus the device buffers the tail needs.

    found[b] = dict(pixel uint32 [m] ascending, level uint32 [m] (1-based tested level), value float64 [m],
                    pval float64 [m])  on the host;  nz_count[b];  fit[b] = (loc[n_tested], scale[n_tested]).
    The tail's gathers are tiny, so dense blocks never leave the device.
    """

    def __init__(self, engine, c, nz, CH, B, nz_count, found, fit):
        self.engine, self.c, self.nz, self.CH, self.B = engine, c, nz, CH, B
        self.nz_count, self.found, self.fit = host_counts(nz_count), found, fit

    def _device(self):
        return self.c.device

    def _features_launch(self, b, pix, half, m, cnt1, cnt2, cval):
        _lib.check(self.engine.lib.mst_candidate_features(_ptr(self.c), _ptr(self.nz), self.CH, b, pix, half, m, cnt1,
                                                          cnt2, cval, _stream()))

    def _diagonals_launch(self, b, ks, m, out):
        _lib.check(self.engine.lib.mst_gather_diagonals(_ptr(self.c), self.CH, b, ks, m, out, _stream()))

    def _diag_means_launch(self, b, ks, m, out):
        _lib.check(self.engine.lib.mst_diag_means(_ptr(self.c), self.CH, b, ks, m, out, _stream()))


class BandBatch(_MultiGather):
    """Same interface as BlockBatch for blocks that exist only as windows of the band (mst_scale_space_band): the tail's
    gathers read the band directly, no dense block is ever built.  Blocks [0, P) read bands[0], blocks [P, B) bands[1]
    (PairBandBatch); the batched gathers make one launch per run of consecutive blocks of the same band."""

    def __init__(self, engine, band, n, dpx, starts, CH, nz_count, found, fit):
        self.engine, self.n, self.dpx, self.starts, self.CH = engine, int(n), int(dpx), list(starts), CH
        self.B = self.P = len(self.starts)
        self.bands = (band,)
        self.nz_count, self.found, self.fit = host_counts(nz_count), found, fit

    def _device(self):
        return self.bands[0].device

    def _band(self, b):
        return self.bands[0] if b < self.P else self.bands[1]

    def _runs(self, bs, sizes):
        """(band, first entry, entries) per run of consecutive blocks of bs on the same band, empty runs left out"""
        off = i = 0
        while i < len(bs):
            j = i
            while j < len(bs) and (bs[j] < self.P) == (bs[i] < self.P):
                j += 1
            m = int(sum(sizes[i:j]))
            if m:
                yield self._band(bs[i]), off, m
            off += m
            i = j

    def _entry_starts(self, bs, sizes):
        starts = np.repeat(np.array([int(self.starts[b]) for b in bs], dtype=np.int64), sizes)
        return torch.from_numpy(starts).to(self._device())

    def _features_one_launch(self, bs, sizes, d_pix, d_half, total, cnt, cval):
        d_s = self._entry_starts(bs, sizes)
        for band, off, m in self._runs(bs, sizes):
            _lib.check(self.engine.lib.mst_candidate_features_band_multi(
                _ptr(band), self.n, self.dpx, _off(d_s, off), self.CH, _off(d_pix, off), _off(d_half, off), m,
                _off(cnt, off), _off(cnt, total + off), _off(cval, off), _stream()))
        return True

    def _diag_means_one_launch(self, bs, sizes, d_k, out):
        d_s = self._entry_starts(bs, sizes)
        for band, off, m in self._runs(bs, sizes):
            _lib.check(self.engine.lib.mst_diag_means_band_multi(_ptr(band), self.n, self.dpx, _off(d_s, off), self.CH,
                                                                 _off(d_k, off), m, _off(out, off), _stream()))
        return True

    def _diagonals_launch(self, b, ks, m, out):
        _lib.check(self.engine.lib.mst_gather_diagonals_band(_ptr(self._band(b)), self.n, self.dpx, int(self.starts[b]),
                                                             self.CH, ks, m, out, _stream()))


class PairBandBatch(BandBatch):
    """The two-sample caller's batch: blocks [0, P) are windows of sample 1's band, blocks [P, 2P) the same windows of
    sample 2's band (reference diff_mustache.py:671-674 builds the two dense blocks; here neither exists)."""

    def __init__(self, engine, bands, n, dpx, starts, CH, nz_count, found, fit):
        super().__init__(engine, bands[0], n, dpx, list(starts) + list(starts), CH, nz_count, found, fit)
        self.bands, self.P = tuple(bands), len(starts)
