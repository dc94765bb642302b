"""Found records -> host: the page-locked staging sets and their lifetime rule, the download of whole found sets, the
device selection (BH + q < pt) that brings back only what the tail looks at, and the ONE function that cuts host columns
into per-block record dicts and fits."""
import numpy as np
import torch

from . import _lib, launch
from ._lib import ptr as _ptr, stream as _stream


class Staging:
    """Page-locked host staging buffers (D2H at PCIe rate) in two alternating sets."""

    def __init__(self):
        self._pin, self._set = {}, 0

    def next_set(self):
        """THE lifetime rule of host results, and the only place the sets are switched.  The record arrays a download
        hands out (download_found with sort=False, the unselected forms) are views of the current set; every download
        calls this exactly ONCE, first thing, so those views stay valid until the download AFTER NEXT -- in the
        overlapped generators (engine.sigma_loop_band_overlapped): until the group after next is fetched.  Consume each
        group as it is yielded (the pipeline's tail does) and copy what has to outlive that; `list(...)` over three or
        more groups leaves the first group's views showing the third group's bytes (scripts/staged_stress.py checks the
        path that way).  A finish that prefetches records for the download behind it writes into the set that download
        will switch to (pinned(upcoming=True)) and does not switch itself."""
        self._set ^= 1

    def pinned(self, key, shape, dtype, upcoming=False):
        """[shape] page-locked array `key` of the current set (upcoming=True: of the set the next download switches
        to)"""
        need = int(np.prod(shape))
        slot = (key, self._set ^ 1 if upcoming else self._set)
        buf = self._pin.get(slot)
        if buf is None or buf.numel() < need or buf.dtype != dtype:
            buf = self._pin[slot] = torch.empty(max(need, 1), dtype=dtype, pin_memory=True)
        return buf[:need].view(*shape)


def cut_records(cols, counts, fit_h, nt, sort=False):
    """Host columns -> (recs, fits), the form every download hands out.  cols: {name: [B, W] array}; the records of
    block b are the first counts[b] slots of row b.  sort=False: the columns are in the order to hand out and
    recs[b][name] is the view cols[name][b, :counts[b]].  sort=True: the slots are in arbitrary order (the selection
    kernel appends) and every block comes out ascending by cols["pixel"] (unique inside a block; row-major = the
    reference's nz order, which the tail's look-ups rely on) -- ONE sort by (block, pixel) over the live slots, then
    every block's arrays are slices of the sorted copies.  fits[b] = (loc[:nt], scale[:nt]), views of fit_h [B, >= nt,
    2], which must be the caller's to give away."""
    counts = np.asarray(counts, dtype=np.int64)
    fits = [(fit_h[b, :nt, 0], fit_h[b, :nt, 1]) for b in range(len(counts))]
    if not sort:
        return [{k: v[b, :m] for k, v in cols.items()} for b, m in enumerate(counts.tolist())], fits
    W = cols["pixel"].shape[1]
    live = np.flatnonzero(np.arange(W, dtype=np.int64)[None, :] < counts[:, None])      # ascending: by block, then slot
    flat = live[np.argsort(((live // max(W, 1)) << 32) | cols["pixel"].reshape(-1)[live], kind="stable")]
    cols = {k: v.reshape(-1)[flat] for k, v in cols.items()}
    ends = np.cumsum(counts).tolist()
    return [{k: v[e - m:e] for k, v in cols.items()} for e, m in zip(ends, counts.tolist())], fits


def fdr(eng, pval, count, found_cap):
    """Benjamini-Hochberg q-values per block on the device (reference mustache.py:778); same record order as pval."""
    B = pval.shape[0]
    q = torch.empty_like(pval)
    ws_bytes = _bh_workspace_bytes(eng, B, found_cap)
    with torch.cuda.device(eng.device):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=eng.device)
        _lib.check(eng.lib.mst_bh_fdr(_ptr(pval), _ptr(count), B, found_cap, _ptr(q), _ptr(ws), ws_bytes, _stream()))
    return q


def _bh_workspace_bytes(eng, B, found_cap):
    ws_bytes = int(eng.lib.mst_bh_workspace_bytes(B, found_cap))
    if ws_bytes == 0:
        raise ValueError("too many found records for one BH launch (B * capacity must fit in int32)")
    return ws_bytes


def results(eng, L, download, sort, with_value, with_q, select_below):
    """What a finished launch returns to the caller: the device buffers, the whole found sets, or the selected
    records."""
    nt = eng.levels.n_tested
    if not download:
        return L.found, L.pval, L.count, L.fit, L.cap
    host = (L.count_h, L.fit_h)
    if select_below is not None:
        return download_selected(eng, L.found, L.pval, L.count, L.fit, nt, L.cap, float(select_below), host=host)
    extra = {"q": fdr(eng, L.pval, L.count, L.cap)} if with_q else None
    return download_found(eng, L.found, L.pval, L.count, L.fit, nt, sort=sort, with_value=with_value, extra=extra,
                          host=host, prefetched=L.prefetched)


def download_found(eng, found, pval, count, fit, nt, sort=True, extra=None, with_value=True, host=None,
                   prefetched=None):
    """Whole found sets -> host: per block dict(pixel u32, level u8, pval f64[, value f64][, extras f64]).  The kernel
    appends records per workgroup, so their order inside a block is arbitrary; with sort=True they are ordered by pixel
    index on the device first.  The returned arrays are views into pinned staging memory (Staging.next_set);
    with_value=False leaves the winning DoG values on the device (only the two-sample path needs them).  host = (counts,
    fits) when they came back with mst_found_finish's round trip; prefetched = the (pixel, level, pval) arrays that call
    already copied."""
    eng.staging.next_set()
    if host is not None and host[0] is not None:
        cnt, fit_h = host
        cnt_d = count.to(torch.int64) if sort else None
    else:
        cnt_d = count.to(torch.int64)
        cnt = cnt_d.cpu().numpy()
        fit_h = fit.cpu().numpy()
    B = len(cnt)
    mx = int(cnt.max()) if B else 0
    cols = {"pixel": np.zeros((B, 0), np.uint32), "level": np.zeros((B, 0), np.uint8), "pval": np.zeros((B, 0))}
    for name in (["value"] if with_value else []) + list(extra or {}):
        cols[name] = np.zeros((B, 0))
    if prefetched is not None and not sort and not extra and not with_value:
        pix_h, lvl_h, pv_h = prefetched             # nothing left to fetch
        cols = {"pixel": pix_h.numpy().view(np.uint32), "level": lvl_h.numpy(), "pval": pv_h.numpy()}
    elif mx > 0:
        rec = found[:, :mx]
        word = rec[..., 0]
        pv = pval[:, :mx]
        if sort:
            pix = word & 0xFFFFFFFF
            valid = torch.arange(mx, device=found.device)[None, :] < cnt_d[:, None]
            order = torch.argsort(torch.where(valid, pix, torch.full_like(pix, 1 << 40)), dim=1)
            rec = torch.gather(rec, 1, order[..., None].expand(-1, -1, 2))
            word = rec[..., 0]
            pv = torch.gather(pv, 1, order)
        for name, t in (extra or {}).items():      # further per-record float64 arrays, same order as the records
            t = t[:, :mx]
            cols[name] = (torch.gather(t, 1, order) if sort else t).cpu().numpy()
        pin = eng.staging.pinned
        pix_h, lvl_h = pin("pix", (B, mx), torch.int32), pin("lvl", (B, mx), torch.uint8)
        pv_h = pin("pv", (B, mx), torch.float64)
        pix_h.copy_((word & 0xFFFFFFFF).to(torch.int32), non_blocking=True)
        lvl_h.copy_((word >> 32).to(torch.uint8), non_blocking=True)
        pv_h.copy_(pv, non_blocking=True)
        if with_value:
            val_h = pin("val", (B, mx), torch.int64)
            val_h.copy_(rec[..., 1], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        cols.update(pixel=pix_h.numpy().view(np.uint32), level=lvl_h.numpy(), pval=pv_h.numpy())
        if with_value:
            cols["value"] = val_h.numpy().view(np.float64)
    return cut_records(cols, cnt, fit_h, nt)


def _selected_layout(B, sel, n_pair, tails):
    """(float64 words, int32 words) of the selection's one buffer, see _selected_parts"""
    return B * sel * (1 + n_pair) + sum(int(t.numel()) for t in tails), 2 * B * sel + B


def _selected_parts(buf, B, sel, n_pair, tails):
    """The selection's one buffer (on the device, or its page-locked twin) by part: q [B, sel], the look-ups [n_pair, B,
    sel], one array per tensor of `tails` (float64) | pixel [B, sel], level [B, sel], selected counts [B] (int32)"""
    n8, _ = _selected_layout(B, sel, n_pair, tails)
    f8, i4 = buf[:8 * n8].view(torch.float64), buf[8 * n8:].view(torch.int32)
    cut, extra = B * sel * (1 + n_pair), []
    for t in tails:
        extra.append(f8[cut:cut + t.numel()].view(t.shape))
        cut += t.numel()
    return (f8[:B * sel].view(B, sel), f8[B * sel:B * sel * (1 + n_pair)].view(n_pair, B, sel), extra,
            i4[:B * sel].view(B, sel), i4[B * sel:2 * B * sel].view(B, sel), i4[2 * B * sel:])


def download_selected(eng, found, pval, count, fit, nt, found_cap, pt, pair=None, host=None, also=None, reuse=None):
    """BH-FDR and the selection q < pt on the device (mustache.py:778-797); only the selected records come back, per
    block dict(pixel u32, level u32, q f64) ascending by pixel.  mst_bh_select_nowait sorts only the records that can be
    selected (same selected set and bit-identical q as mst_bh_fdr over all records followed by mst_select_below), in
    LDS.  pair = (ppair [2P, found_cap], P), two-sample path: the records also carry `pair`, `value` and `v_other`, the
    differential test's look-ups (mst_pair_gather).  host = (counts, fits) when they came back with mst_found_finish
    already -- or, when the caller queued that finish in front with wait=False, the function that checks it and returns
    them (launch.finish_landed), called behind the wait; None: the fits are fetched here.  also: a float64 device tensor
    to bring back in the same copy (the two-sample path's norm.fit), returned as third element.  Everything is queued
    back to back -- selection, look-ups, ONE copy of one device buffer to its page-locked twin (six small copies were 45
    us of device time and 0.4 ms of host time) -- and waited for ONCE; the checks that would cost a round trip each come
    after the wait, the finish's own first (a call on six block pairs of 2000 x 2000 is 1.4 ms of kernels: three more
    waits of ~45 us each were 10 % of it).  Two things send the selection round again, both rare and both learned by the
    engine: a block whose candidate subset exceeds the LDS sort size (MST_BH_RETRY: eng._bh_lds_records doubles, up to
    4096, and this call goes through the synchronising forms mst_bh_select / mst_bh_select_records), and more selected
    records in a block than eng._select_cap (twice the need from then on).  reuse: carve key under which the device
    buffers are kept between calls (small, latency-bound calls)."""
    B, lib, n_pair = count.shape[0], eng.lib, 0 if pair is None else 3
    ws_bytes = _bh_workspace_bytes(eng, B, found_cap)
    tails = ([] if also is None else [also]) + ([fit] if host is None else [])
    eng.staging.next_set()
    with torch.cuda.device(eng.device):
        while True:
            sel = eng._select_cap
            n8, n4 = _selected_layout(B, sel, n_pair, tails)
            bufs = [(ws_bytes, torch.uint8, (ws_bytes,)), (8 * n8 + 4 * n4, torch.uint8, (8 * n8 + 4 * n4,))]
            if pair is not None:
                bufs.append((B * sel * 4, torch.int32, (B, sel)))
            ws, blob, *idx = launch.carve(eng, *bufs, reuse=reuse)
            idx = idx[0] if idx else None
            hblob = eng.staging.pinned("selected", (int(blob.numel()),), torch.uint8)
            qs, g, d_tails, pix, lvl, n_sel = _selected_parts(blob, B, sel, n_pair, tails)
            args = (_ptr(found), _ptr(pval), _ptr(count), B, found_cap, pt, sel, _ptr(pix), _ptr(lvl), _ptr(qs),
                    _ptr(idx), _ptr(n_sel), _ptr(ws), ws_bytes, _stream())
            # the sort's LDS request: 1024 records (14 KB) until a launch of this engine needed more -- this kernel runs
            # next to the following group's fused kernel, which leaves little LDS free
            _lib.check(lib.mst_bh_select_nowait(*(args[:12] + (eng._bh_lds_records,) + args[12:])))
            for synchronising_form in (False, True):
                if synchronising_form:
                    eng._bh_lds_records = min(4096, eng._bh_lds_records * 2)
                    _lib.check(lib.mst_bh_select_records(*args) if pair is not None
                               else lib.mst_bh_select(*(args[:10] + args[11:])))
                if pair is not None:
                    _lib.check(lib.mst_pair_gather(_ptr(found), found_cap, _ptr(count), _ptr(pair[0]), int(pair[1]),
                                                   _ptr(idx), _ptr(pix), _ptr(n_sel), sel, sel, _ptr(g[0]), _ptr(g[1]),
                                                   _ptr(g[2]), _stream()))
                for d, t in zip(d_tails, tails):
                    d.copy_(t)
                hblob.copy_(blob, non_blocking=True)
                torch.cuda.current_stream().synchronize()
                if callable(host):
                    host = host()
                q_h, g_h, h_tails, pix_h, lvl_h, n_h = _selected_parts(hblob, B, sel, n_pair, tails)
                n_h = n_h.numpy().view(np.uint32).astype(np.int64)
                if not (n_h == _lib.MST_BH_RETRY).any():
                    break
            mx = int(n_h.max(initial=0))
            if mx <= sel:
                break
            eng._select_cap = mx * 2           # the round again with room for every selected record
    cols = {"pixel": pix_h.numpy().view(np.uint32), "level": lvl_h.numpy().view(np.uint32), "q": q_h.numpy()}
    if pair is not None:
        cols.update(zip(("pair", "value", "v_other"), g_h.numpy()))
    fit_h = host[1] if host is not None else h_tails[-1].numpy().copy()
    out = cut_records(cols, n_h, fit_h, nt, sort=True)
    return out + (h_tails[0].numpy().copy(),) if also is not None else out
