"""The fused scale-space launch in its five forms (dense blocks, windows of a band, windows of two bands, one launch in
stages, a launch replayed as a hipGraph): its state record, buffers, enqueue, overflow rule and finish.  Plain functions
over the engine, which owns what launches learn (record capacities, workspace sizes, kept buffers)."""
import ctypes
import itertools
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import ptr as _ptr, stream as _stream


def default_found_cap(CH):
    """Record capacity per block of CH x CH before any launch overflowed: one record per 32 pixels, at least 4096."""
    return max(4096, (CH * CH) // 32)


def _event_pair(timing):
    """(start, end) timing events around a launch, the start recorded on the current stream; None without a timing
    list."""
    if timing is None:
        return None
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    return ev


@dataclass(slots=True, eq=False)
class _Launch:
    """One fused scale-space launch -- or one group's stage of a staged launch (a view) -- as ss_launch enqueued it, and
    what its finish brought back.  An overflow re-enqueues the same record (grow)."""
    B: int
    CH: int
    cap: int                    # record capacity per block
    flags: int                  # MST_FLAG_* word of the launch
    nzc: object = None          # tested-pixel counts [B] int32 (device): input of the dense, output of the band kernels
    own_nzc: bool = False       # nzc is one of the launch's buffers (allocated with them)
    blocks: tuple = None        # (c, nz): dense blocks and their masks
    band_src: tuple = None      # (band, n, dpx, ctypes array of the B block origins): windows of a band
    band2: tuple = None         # (second band, split): blocks [split, B) are windows of the second band
    stages: list = None         # staged launch: block counts of its groups, one stage each
    views: list = None          # staged launch: one record per group (views of the buffers), set by enqueue
    timing: list = None         # receives `ev` once the finish has synchronised
    ev: tuple = None            # (start, end) events around the launch
    reuse: object = None        # carve slot of the launch's buffers and of its finish's staging; None = not kept
    graph: bool = False         # the finish is replayed as a hipGraph (MST_FLAG_GRAPH)
    done: object = None         # event behind the launch (a staged group: behind its stage)
    ws: object = None           # the launch's buffers
    stats: object = None
    fit: object = None
    count: object = None
    found: object = None
    pval: object = None
    count_h: object = None      # set by the finish: record counts, tested-pixel counts, fits (host), prefetched records
    nz_h: object = None
    fit_h: object = None
    prefetched: object = None


def flags(eng, skip_empty, fma, graph=False):
    """The launch's flag word.  MST_FLAG_NO_SHARE: every tile once per block (default: tiles inside two consecutive
    blocks computed once); MST_FLAG_GRAPH: a launch that repeats with identical arguments is replayed as one
    hipGraph."""
    return ((_lib.MST_FLAG_SKIP_EMPTY if skip_empty else 0) | (_lib.MST_FLAG_FMA if fma else 0)
            | (0 if eng.share_tiles else _lib.MST_FLAG_NO_SHARE) | (_lib.MST_FLAG_GRAPH if graph else 0))


def found_cap_for(eng, CH):
    """record capacity per block of the next launch of CH x CH blocks: the default, or what an overflow taught (grow)"""
    return eng._found_cap.get(CH, default_found_cap(CH))


def workspace_bytes(eng, B, CH):
    ws_bytes = eng._ws_bytes.get((B, CH))
    if ws_bytes is None:
        ws_bytes = eng._ws_bytes[(B, CH)] = int(
            eng.lib.mst_scale_space_workspace_bytes(B, CH, ctypes.byref(eng._lv_struct)))
    return ws_bytes


def carve(eng, *parts, reuse=None):
    """Device buffers for one launch: parts = (bytes, dtype, shape).  `reuse` (a hashable key, or None): SMALL sets
    (< 256 MB) are kept and handed out again for the same key -- a launch of six 2000 x 2000 blocks is 1.75 ms of
    kernel, and a dozen allocator calls per step are 2 % of it; callers pass a key only when the buffers do not outlive
    the call (the results are host copies) and alternate the key's slot between launches in flight."""
    total = sum(int(p[0]) for p in parts)
    key = None
    if reuse is not None and total < (256 << 20):
        key = (reuse,) + tuple((int(p[0]), p[1]) for p in parts)
        hit = eng._buffers.get(key)
        if hit is not None:
            return hit
    out = tuple(torch.empty(shape, dtype=dt, device=eng.device) for _, dt, shape in parts)
    if key is not None:
        if len(eng._buffers) > 16:
            eng._buffers.clear()
        eng._buffers[key] = out
    return out


def _launch_buffers(eng, B, CH, cap, reuse, nzc=False):
    """ws, stats, fit, count, found (16-byte records), pval -- and with nzc=True the tested-pixel counts -- of one
    launch (kept between calls for small launches when `reuse` names a slot, see carve)"""
    T = _lib.MST_MAX_TESTED
    ws_bytes = workspace_bytes(eng, B, CH)
    parts = [(ws_bytes, torch.uint8, (ws_bytes,)), (B * T * 16, torch.float64, (B, T, 2)),
             (B * T * 16, torch.float64, (B, T, 2)), (B * 4, torch.int32, (B,)),
             (B * cap * 16, torch.int64, (B, cap, 2)), (B * cap * 8, torch.float64, (B, cap))]
    if nzc:
        parts.append((B * 4, torch.int32, (B,)))
    return carve(eng, *parts, reuse=None if reuse is None else ("launch", reuse))


def _starts_array(eng, starts):
    key = tuple(starts)
    arr = eng._starts_arrays.get(key)          # repeated launches of the same blocks: no re-marshalling
    if arr is None:
        if len(eng._starts_arrays) > 64:
            eng._starts_arrays.clear()
        arr = eng._starts_arrays[key] = (ctypes.c_int64 * len(key))(*key)
    return arr


def ss_launch(eng, flag_word, nzc=None, blocks=None, band_src=None, band2=None, stages=None, found_cap=None,
              timing=None, reuse=None, graph=False):
    """Record one fused launch and enqueue it on the current stream (no synchronisation).  Source: `blocks` = (c, nz),
    dense blocks and their masks, or `band_src` = (band, n, dpx, starts, CH), windows of a band; `band2` = (second band,
    split): ONE launch over the blocks of two bands (the two samples of a two-sample call; blocks [split, B) read the
    second band).  `nzc`: the tested-pixel counts (input of the dense kernel, output of the band kernel); None = one of
    the launch's own buffers.  `stages`: block counts of the groups of a staged launch (enqueue).  `reuse`: the carve
    slot of the launch's buffers and its finish's staging.  `graph`: the finish is replayed as a hipGraph too."""
    if band_src is not None:
        band, n, dpx, starts, CH = band_src
        B, src = len(starts), (band, n, dpx, _starts_array(eng, starts))
    else:
        (B, CH, _), src = blocks[0].shape, None
    L = _Launch(B, CH, found_cap_for(eng, CH) if found_cap is None else found_cap, flag_word, nzc=nzc,
                own_nzc=nzc is None, blocks=blocks, band_src=src, band2=band2, stages=stages, timing=timing,
                reuse=reuse, graph=graph)
    return enqueue(eng, L)


def enqueue(eng, L):
    """(Re)allocate L's buffers at capacity L.cap and enqueue its fused launch on the current stream.
    A staged launch (L.stages) is enqueued in one stage per group (mst_scale_space_band_stage): the work list is the
    whole launch's, so tiles shared by the last block of a group and the first block of the next are still computed once
    -- separate launches per group recompute them (0.4 ms per cut on 4000 x 4000 blocks) -- and after stage i the blocks
    of groups 0 .. i are final.  L.views then holds one record per group in the form finish takes: views of the launch's
    buffers for the group's blocks, with `done` = the event behind the group's stage."""
    B, CH, cap, lib = L.B, L.CH, L.cap, eng.lib
    lv = ctypes.byref(eng._lv_struct)
    ws_bytes = workspace_bytes(eng, B, CH)
    with torch.cuda.device(eng.device):
        bufs = _launch_buffers(eng, B, CH, cap, L.reuse, nzc=L.own_nzc)
        L.ws, L.stats, L.fit, L.count, L.found, L.pval = bufs[:6]
        if L.own_nzc:
            L.nzc = bufs[6]
        tail = (_ptr(L.found), cap, _ptr(L.count), _ptr(L.stats))
        if L.stages is not None:
            band, n, dpx, st_arr = L.band_src
            cuts = list(itertools.accumulate(L.stages))[:-1]
            cut_arr = (ctypes.c_int32 * max(1, len(cuts)))(*cuts)
            cur = torch.cuda.current_stream(eng.device)
            L.views, b0 = [], 0
            for gi, nb in enumerate(L.stages):
                ev = _event_pair(L.timing)
                _lib.check(lib.mst_scale_space_band_stage(_ptr(band), n, dpx, st_arr, B, CH, lv, *tail, _ptr(L.nzc),
                                                          L.flags, _ptr(L.ws), ws_bytes, cut_arr, len(cuts), gi,
                                                          _stream()))
                if ev is not None:
                    ev[1].record()
                b1 = b0 + nb
                L.views.append(_Launch(nb, CH, cap, L.flags, nzc=L.nzc[b0:b1], timing=L.timing, ev=ev, reuse=1 + gi % 2,
                                       done=cur.record_event(), stats=L.stats[b0:b1], fit=L.fit[b0:b1],
                                       count=L.count[b0:b1], found=L.found[b0:b1], pval=L.pval[b0:b1]))
                b0 = b1
            return L
        L.ev = _event_pair(L.timing)
        if L.blocks is not None:
            c, nz = L.blocks
            _lib.check(lib.mst_scale_space(_ptr(c), _ptr(nz), B, CH, lv, *tail, L.flags, _ptr(L.ws), ws_bytes,
                                           _stream()))
        elif L.band2 is not None:
            band, n, dpx, st_arr = L.band_src
            _lib.check(lib.mst_scale_space_band_pair(_ptr(band), _ptr(L.band2[0]), int(L.band2[1]), n, dpx, st_arr, B,
                                                     CH, lv, *tail, _ptr(L.nzc), L.flags, _ptr(L.ws), ws_bytes,
                                                     _stream()))
        else:
            band, n, dpx, st_arr = L.band_src
            _lib.check(lib.mst_scale_space_band(_ptr(band), n, dpx, st_arr, B, CH, lv, *tail, _ptr(L.nzc), L.flags,
                                                _ptr(L.ws), ws_bytes, _stream()))
        if L.ev is not None:
            L.ev[1].record()
    return L


def grow(eng, L, relaunch=True):
    """THE record-capacity overflow rule (rare: a block with an unusually dense set of local maxima): four times the
    capacity, kept for every later launch of blocks of this size, and the same launch again on the current stream --
    unless the caller redoes the work another way (relaunch=False)."""
    L.cap = eng._found_cap[L.CH] = L.cap * 4
    return enqueue(eng, L) if relaunch else L


def summary_pin(eng, B):
    """Page-locked landing area of mst_found_finish's one round trip (flags, counts, tested-pixel counts, fits)."""
    need = int(eng.lib.mst_found_summary_bytes(B))
    buf = eng._summary_pins.get(B)
    if buf is None or buf.numel() < need:
        buf = eng._summary_pins[B] = torch.empty(need, dtype=torch.uint8, pin_memory=True)
    return buf


def parse_summary(h, B):
    """mst_found_finish's summary block (include/mustache_hip.h; h: its bytes as a uint8 array) -> (found counts,
    tested-pixel counts, fits) as host arrays of their own"""
    T, cw = _lib.MST_MAX_TESTED, 8 * ((B + 1) // 2)
    return (h[16:16 + 4 * B].view(np.uint32).astype(np.int64),
            h[16 + cw:16 + cw + 4 * B].view(np.uint32).astype(np.int64),
            h[16 + 2 * cw:16 + 2 * cw + 16 * T * B].view(np.float64).reshape(B, T, 2).copy())


def finish(eng, L, packed=False, relaunch=True, wait=True, scratch=None):
    """p-values of the found pixels (ONE synchronisation of the launch stream: mst_found_finish brings the overflow
    flag, the record counts, the tested-pixel counts and the fits back in the same round trip); a record-capacity
    overflow re-runs the launch (grow), or with relaunch=False is the caller's to handle.  packed=True: for a caller
    that downloads whole found sets, the records may come back inside the same call (L.prefetched: the three host
    arrays, when the guess of the largest count held).  wait=False (MST_FLAG_NO_WAIT): enqueue only -- the caller queues
    more work behind it on the same stream, waits once, and then calls finish_landed for the status and the summary."""
    nt, none3 = eng.levels.n_tested, (None, None, None)
    with torch.cuda.device(eng.device):
        while True:
            B, cap = L.B, L.cap
            # whole-found-set downloads: the first `pitch` records of every block also come out as narrow, densely
            # pitched arrays and are copied to the host inside the same call; pitch = the largest count the last launch
            # of this block size saw + 5 % (the first launch of a size has no guess and takes the two-step download)
            pitch = min(cap, eng._prefetch_guess.get(L.CH, 0)) if packed and wait else 0
            summ = summary_pin(eng, B)
            dev3 = host3 = none3
            if pitch > 0:
                scratch, *dev3 = carve(eng, (summ.numel(), torch.uint8, (summ.numel(),)),
                                       (B * pitch * 4, torch.int32, (B, pitch)), (B * pitch, torch.uint8, (B, pitch)),
                                       (B * pitch * 8, torch.float64, (B, pitch)),
                                       reuse=None if L.reuse is None else ("finish", L.reuse))
                # lands in the staging set that the download behind this finish switches to (records.Staging)
                host3 = tuple(eng.staging.pinned(k, (B, pitch), dt, upcoming=True)
                              for k, dt in (("pix", torch.int32), ("lvl", torch.uint8), ("pv", torch.float64)))
            elif scratch is None:
                scratch = torch.empty(summ.numel(), dtype=torch.uint8, device=eng.device)
            how = (_lib.MST_FLAG_GRAPH if L.graph else 0) if wait else _lib.MST_FLAG_NO_WAIT
            try:
                _lib.check(eng.lib.mst_found_finish(_ptr(L.found), cap, _ptr(L.count), _ptr(L.nzc), _ptr(L.stats), B,
                                                    nt, _ptr(L.pval), _ptr(L.fit), pitch, *(_ptr(t) for t in dev3),
                                                    _ptr(scratch), _ptr(summ), *(_ptr(t) for t in host3), how,
                                                    _stream()))
                break
            except _lib.MstOverflow:
                if not relaunch:            # the caller owns the launches (several of them behind this one finish)
                    raise
                grow(eng, L)
    if not wait:
        return L
    _read_summary(eng, L)
    L.prefetched = None
    if packed:
        mx = int(L.count_h.max(initial=0))
        if pitch > 0 and mx <= pitch:
            L.prefetched = host3        # the guess held: the records are on the host already
        # next guess: 10 % above this launch's largest count, but never much below the last guess -- the launches of a
        # run differ (a genome's chromosomes, a chromosome's ends), and a guess that fails costs a second download
        eng._prefetch_guess[L.CH] = max(mx + mx // 10 + 64, int(0.995 * eng._prefetch_guess.get(L.CH, 0)))
    return L


def _read_summary(eng, L):
    if L.ev is not None:
        L.timing.append(L.ev)      # the stream has been synchronised: the events are complete
    L.count_h, L.nz_h, L.fit_h = parse_summary(summary_pin(eng, L.B).numpy(), L.B)


def finish_landed(eng, L):
    """Behind the caller's wait for a finish queued with wait=False: the status that call could not return (MstOverflow:
    relaunch with larger lists -- the library words the error) and the summary.  Returns (record counts, fits)."""
    summ = summary_pin(eng, L.B)
    if int(summ.numpy()[:4].view(np.int32)[0]):       # overflow / non-finite flags
        _lib.check(eng.lib.mst_found_summary_status(_ptr(summ), L.cap))
    _read_summary(eng, L)
    return L.count_h, L.fit_h
