"""Device-side driver of the scale-space hot path: torch tensors for HBM + streams, HIP kernels through the C ABI.

PyTorch is plumbing here (device memory, streams); every number is produced by libmustache_hip.so.  A missing
library or a missing GPU is an error -- there is no CPU path in this package.

The engine owns the level table, the streams' use and what launches learn; the launch forms are in launch.py, the way
from found records to host arrays in records.py, the batches the host tail works on in batches.py.
"""
import contextlib
import ctypes
import functools
import os

import numpy as np
import torch

from . import _lib, launch, records
from ._lib import ptr as _ptr, require_gpu, stream as _stream
from .batches import BandBatch, BlockBatch, PairBandBatch, _MultiGather      # noqa: F401  (this module's interface)
from .launch import default_found_cap                          # noqa: F401
from .levels import LevelTable

_STREAMS = {}


def device_streams(device):
    """The package's three side streams of `device`, created ONCE per process: two for the fused kernel's launches
    (alternating, so that the post-processing of one launch runs under the kernel of the next) and one for
    host-to-device copies of the streaming `.hic` read.  HIP maps streams to a handful of hardware queues in creation
    order; a stream per engine or per call makes that mapping depend on what else the process has created, and two
    streams that land on one queue serialise -- the host tail's small kernels then wait behind the next launch's fused
    kernel (measured: a whole-genome run 0.032 -> 0.053 s after another engine had created two streams).  One fixed set
    keeps the mapping the same in every run."""
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    got = _STREAMS.get(key)
    if got is None:
        got = _STREAMS[key] = tuple(torch.cuda.Stream(device) for _ in range(3))
    return got


_GC_SETTLED = False


def settle_gc():
    """Once per process: move everything alive now (the modules of torch, numpy, this package: ~10^6 objects that never
    die) out of the cyclic collector's reach (`gc.freeze()`).  A chromosome's host tail makes ~2 * 10^4 short-lived
    containers (one 4-element list per loop, as the reference returns them), so CPython ran a full collection every
    third chromosome and each one walked all of those objects: +27-38 ms on a 55-75 ms step, exactly periodic
    (scripts/pair_genome_jitter.py, scripts/file_leg_cpu.py; LABBOOK R5.8).  Results do not depend on it.  A
    process-global, irreversible change, so the LIBRARY never makes it on its own: the command-line entry points
    (mustache.main, diff_mustache.main) and bench.py call this; a host application that imports mustache() / regulator()
    keeps its collector untouched unless it calls settle_gc() itself or exports MUSTACHE_GC_FREEZE=1 (then the first
    engine does).  MUSTACHE_GC_FREEZE=0 leaves the collector alone everywhere."""
    global _GC_SETTLED
    if _GC_SETTLED or os.environ.get("MUSTACHE_GC_FREEZE", "1") == "0":
        return
    import gc
    # (no gc.collect() first: that full collection is the 0.1 s this is here to avoid; whatever cyclic garbage exists at
    # this moment stays allocated, a few objects)
    gc.freeze()
    _GC_SETTLED = True


class ScaleSpaceEngine:
    """Owns the level table and runs rows 2-7 of SURVEY.md section 8a on the GPU."""

    def __init__(self, octave_values=(1.6, 3.2), s=10, device=None):
        self.lib = require_gpu()
        # band source: compute the tiles two consecutive blocks have in common once (identical records)
        self.share_tiles = True
        # several groups of blocks with host results: one launch in stages (mst_scale_space_band_stage) instead of a
        # launch per group; MUSTACHE_STAGED=0 keeps the launch-per-group form (the cross-check of
        # tests/test_gpu_pipeline.py)
        self.staged_launches = os.environ.get("MUSTACHE_STAGED", "1") != "0"
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self.levels = LevelTable(octave_values, s)
        self._lv_struct = self.levels.as_struct()
        # ---- what launches learn (launch.py, records.py) ----
        self._found_cap = {}            # CH -> record capacity per block after an overflow (launch.grow)
        self._select_cap = 256          # selected records per block records.download_selected has room for
        self._bh_lds_records = 1024     # LDS sort size of mst_bh_select_nowait (doubles on MST_BH_RETRY)
        self._prefetch_guess = {}       # CH -> record columns mst_found_finish copies to the host speculatively
        # ---- kept between calls ----
        self._buffers = {}              # small device buffer sets (launch.carve)
        self._starts_arrays, self._ws_bytes = {}, {}
        self._summary_pins = {}         # B -> page-locked landing area of mst_found_finish's summary
        self.staging = records.Staging()
        if os.environ.get("MUSTACHE_GC_FREEZE") == "1":      # library use: opt-in only (settle_gc's docstring)
            settle_gc()

    # ---- host queries of the launch geometry (no GPU work) --------------------------------------------------------
    def band_tile_fraction(self, CH, dpx):
        """Share of a block's tiles launched with empty tiles skipped: those whose owned pixels can reach the tested
        band 4 <= col - row <= dpx + 1 (mst_scale_space_band_tiles)."""
        total = ctypes.c_int32(0)
        m = self.lib.mst_scale_space_band_tiles(int(CH), int(dpx), ctypes.byref(self._lv_struct), ctypes.byref(total))
        if m < 0:
            _lib.check(m)
        return m / float(total.value)

    def band_items(self, starts, CH, dpx, skip_empty=False, share=True):
        """(workgroups one launch over the blocks at `starts` runs, tiles the blocks would run one by one, tiles
        computed once for two blocks) -- mst_scale_space_band_items, the work list the band-direct kernel is launched
        with."""
        st = (ctypes.c_int64 * len(starts))(*[int(a) for a in starts])
        tiles, shared = ctypes.c_int64(), ctypes.c_int64()
        flag_word = (_lib.MST_FLAG_SKIP_EMPTY if skip_empty else 0) | (0 if share else _lib.MST_FLAG_NO_SHARE)
        m = self.lib.mst_scale_space_band_items(st, len(starts), int(CH), int(dpx), ctypes.byref(self._lv_struct),
                                                flag_word, ctypes.byref(tiles), ctypes.byref(shared))
        if m < 0:
            _lib.check(m)
        return int(m), int(tiles.value), int(shared.value)

    # ---- row 2: COO -> dense blocks ---------------------------------------------------------------------------
    def scatter_blocks(self, x, y, v, starts, CH):
        """x, y int64 / v float64 device tensors (upper-triangular COO, bin units) -> [B, CH, CH] float64."""
        B = len(starts)
        c = torch.empty((B, CH, CH), dtype=torch.float64, device=self.device)
        st = (ctypes.c_int64 * B)(*[int(s) for s in starts])
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mst_scatter_blocks(_ptr(x), _ptr(y), _ptr(v), int(v.numel()), st, B, CH, _ptr(c),
                                                   _stream()))
        return c

    # ---- row 4 bring-up: one Gaussian level ----------------------------------------------------------------------
    def gauss_blur(self, img, taps):
        """img [B, H, W] float64 device tensor; taps = centre-first half kernel (radius = len-1)."""
        img = img.contiguous()
        B, H, W = img.shape
        out = torch.empty_like(img)
        tmp = torch.empty_like(img)
        arr = (ctypes.c_double * len(taps))(*[float(t) for t in taps])
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mst_gauss_blur(_ptr(img), _ptr(out), _ptr(tmp), B, H, W, arr, len(taps) - 1, _stream()))
        return out

    # ---- rows 3-7 -------------------------------------------------------------------------------------------------
    def prologue(self, c, dpx, intra=True):
        B, CH, _ = c.shape
        nz = torch.empty((B, CH, CH), dtype=torch.uint8, device=self.device)
        nz_count = torch.empty(B, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mst_block_prologue(_ptr(c), _ptr(nz), _ptr(nz_count), B, CH, int(dpx),
                                                   1 if intra else 0, _stream()))
        return nz, nz_count

    def sigma_loop_band(self, band, n, dpx, starts, CH, **kw):
        """Rows 2-7 straight from the normalised band: blocks are cut, filled and masked inside the fused kernel.
        Returns what sigma_loop returns plus the per-block tested-pixel counts (device int32 tensor) as last element."""
        nz_count = torch.empty(len(starts), dtype=torch.int32, device=self.device)
        res = self.sigma_loop(None, None, nz_count, band_src=(band, int(n), int(dpx), [int(s) for s in starts],
                              int(CH)), **kw)
        return res + (nz_count,)       # (a record-capacity overflow re-ran the kernel into this same tensor)

    def sigma_loop(self, c, nz, nz_count, skip_empty=True, found_cap=None, download=True, timing=None, sort=True,
                   with_value=True, with_q=True, fma=False, band_src=None, select_below=None):
        """The fused kernel + p-values.  Returns host records (download=True) or the device buffers.
        `select_below=pt`: BH and the selection q < pt (mustache.py:778-797) run on the device and only those records
        come back, as dict(pixel, level, q) sorted by pixel -- all the tail ever looks at; the full found set stays in
        HBM.  `timing`: optional list; receives a (start, end) torch.cuda.Event pair bracketing the mst_scale_space
        launch on the launch stream.  `band_src` = (band, n, dpx, starts, CH) selects the band-direct kernel (c, nz
        unused; nz_count is then an OUTPUT)."""
        L = launch.ss_launch(self, launch.flags(self, skip_empty, fma), nzc=nz_count,
                             blocks=None if band_src is not None else (c, nz), band_src=band_src, found_cap=found_cap,
                             timing=timing)
        return self._finish_results(L, (download, sort, with_value, with_q, select_below))

    def _finish_results(self, L, form, relaunch=True):
        """The finish of launch L and its results in the caller's form = (download, sort, with_value, with_q,
        select_below); a caller that takes whole found sets as they lie (unsorted) lets the finish bring the records
        along (packed)."""
        download, sort, _, _, select_below = form
        packed = download and select_below is None and not sort
        return records.results(self, launch.finish(self, L, packed=packed, relaunch=relaunch), *form)

    # ---- streams ------------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def _capturable_stream(self, wanted=True):
        """The stream a launch that may be replayed as a hipGraph (MST_FLAG_GRAPH) runs on: the caller's -- but a graph
        cannot be captured on the legacy default stream, so from there the work goes to the first side stream, ordered
        behind what the caller's stream produced, and the caller's stream is ordered behind it afterwards (explicitly,
        whatever synchronisation the work did)."""
        cur = torch.cuda.current_stream(self.device)
        side = device_streams(self.device)[0] if wanted and cur.cuda_stream == 0 else None
        if side is None:
            yield
            return
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            yield
        cur.wait_stream(side)

    def _ping_pong(self, groups, queue, collect):
        """The two-stream overlap of both overlapped generators: `queue(gi, group)` enqueues a group's device work on
        one of two alternating side streams (behind what the caller's stream produced, and behind the previous group's
        work: one group's kernels at a time), and group i + 1 is queued BEFORE `collect(group, work)` fetches the
        results of group i on that group's stream -- so the finish, selection and download of one group, and the
        caller's host tail, run under the kernels of the next.  Yields what collect returns."""
        cur = torch.cuda.current_stream(self.device)
        ready = cur.record_event()
        streams = device_streams(self.device)[:2]
        pending = done = None

        def fetch(s, group, work):
            with torch.cuda.stream(s), torch.cuda.device(self.device):
                return collect(group, work)

        for gi, group in enumerate(groups):
            s = streams[gi % 2]
            s.wait_event(ready)
            if done is not None:
                s.wait_event(done)
            with torch.cuda.stream(s):
                work = queue(gi, group)
                done = s.record_event()
            if pending is not None:
                yield fetch(*pending)
            pending = (s, group, work)
        if pending is not None:
            yield fetch(*pending)
        cur.wait_stream(streams[0])
        cur.wait_stream(streams[1])

    def sigma_loop_band_overlapped(self, band, n, dpx, groups, CH, skip_empty=True, timing=None, fma=False,
                                   download=True, sort=True, with_value=True, with_q=True, select_below=None):
        """sigma_loop_band over several groups of blocks with copy/compute overlap: the groups' fused kernels run back
        to back, and the p-values / BH / selection / download of group i run while the kernel of group i + 1 is
        executing.  Yields, per group, what sigma_loop_band returns -- with host results the tested-pixel counts as a
        HOST tensor (they came back with the finish's round trip; callers' .cpu() is then free).  LIFETIME of the host
        results: records.Staging.next_set -- consume each group as it is yielded."""
        form = (download, sort, with_value, with_q, select_below)
        src = lambda starts: (band, int(n), int(dpx), [int(v) for v in starts], int(CH))
        flag_word = launch.flags(self, skip_empty, fma)

        def result(L, relaunch=True):
            res = self._finish_results(L, form, relaunch)
            return res + ((torch.from_numpy(L.nz_h.astype(np.uint32).view(np.int32)) if download else L.nzc),)

        if len(groups) == 1:
            # nothing to overlap: run on the caller's stream, without the side streams' events (a small launch -- six
            # blocks of 2000 x 2000 are 1.75 ms of kernel -- pays for every host-side call).  With host results
            # (download) the launch buffers are kept between calls, so a caller that repeats the launch -- a benchmark
            # step, the same chromosome again -- presents identical arguments and the library replays it as ONE hipGraph
            # launch.
            with self._capturable_stream(download):
                L = launch.ss_launch(self, launch.flags(self, skip_empty, fma, graph=download), band_src=src(groups[0]),
                                     timing=timing, reuse=0 if download else None, graph=download)
                res = result(L)
            yield res
            return
        if not (self.staged_launches and download):
            # a launch per group; two launches in flight: two buffer sets
            yield from self._ping_pong(
                groups,
                lambda gi, starts: launch.ss_launch(self, flag_word, band_src=src(starts), timing=timing,
                                                    reuse=(1 + gi % 2) if download else None),
                lambda starts, L: result(L))
            return
        # ONE launch in one stage per group on the first side stream; the p-values / selection / download of group i run
        # on the second one behind stage i's event, while stage i + 1 executes.  Same records as separate launches.
        cur = torch.cuda.current_stream(self.device)
        ready = cur.record_event()              # the band was produced on the caller's stream
        ks, fs = device_streams(self.device)[:2]
        ks.wait_event(ready)
        # (a launch's record lists, p-values and per-tile statistics are allocated for all of its blocks at once: 24 B x
        # CH^2 / 32 per block and ~2.6 MB of statistics per 4000 x 4000 block -- 1.9 GB for chr1 at 1 kb.  Whole genomes
        # at fine resolutions go through several staged launches of at most MUSTACHE_STAGED_GB, default 32, of such
        # buffers.)
        per_block = 24 * launch.found_cap_for(self, int(CH)) + \
            (int(CH) // 30 + 2) * (int(CH) // 62 + 2) * (20 + 16 * self.levels.n_tested)
        budget = float(os.environ.get("MUSTACHE_STAGED_GB", "32")) * (1 << 30)
        chunks, acc = [[]], 0
        for g in groups:
            if chunks[-1] and (acc + len(g)) * per_block > budget:
                chunks.append([])
                acc = 0
            chunks[-1].append(g)
            acc += len(g)
        for chunk in chunks:
            with torch.cuda.stream(ks), _lib.stage("scale-space launch"):
                L = launch.ss_launch(self, flag_word, band_src=src([v for g in chunk for v in g]),
                                     stages=[len(g) for g in chunk], timing=timing, reuse="staged")
            gi = 0
            while gi < len(chunk):
                view = L.views[gi]
                fs.wait_event(view.done)
                try:
                    with torch.cuda.stream(fs), _lib.stage("scale-space finish"):
                        res = result(view, relaunch=False)
                except _lib.MstOverflow:
                    # the whole launch again with more room; the groups already handed out stay as they are (their
                    # records were complete)
                    ks.synchronize()
                    with torch.cuda.stream(ks), _lib.stage("scale-space launch"):
                        launch.grow(self, L)
                    continue
                yield res
                gi += 1
        cur.wait_stream(ks)
        cur.wait_stream(fs)

    # ---- two-sample additions (reference diff_mustache.py:262-276, :371-385)
    # --------------------------------------------
    def pair_pvalues(self, c, nz, found, found_cap, count):
        """c / nz: [2P, CH, CH] filled blocks and masks, sample 1 in [0, P), sample 2 in [P, 2P); found / count: the
        device records of the 2P-block sigma loop.  Returns ppair [2P, found_cap] (device)."""
        P2, CH, _ = c.shape
        P = P2 // 2
        lt = self.levels
        n_oct, lpo, tpo = len(lt.octave_values), lt.levels_per_octave, lt.s - 1
        dev = self.device
        with torch.cuda.device(dev):
            cd = torch.empty((P, CH, CH), dtype=torch.float64, device=dev)
            nzb = torch.empty((P, CH, CH), dtype=torch.uint8, device=dev)
            nzbc = torch.empty(P, dtype=torch.int32, device=dev)
            _lib.check(self.lib.mst_diff_image(_ptr(c[:P]), _ptr(c[P:]), _ptr(nz[:P]), _ptr(nz[P:]), P, CH, _ptr(cd),
                                               _ptr(nzb), _ptr(nzbc), _stream()))
            g2 = torch.empty((n_oct, P, CH, CH), dtype=torch.float64, device=dev)
            g3 = torch.empty((n_oct, P, CH, CH), dtype=torch.float64, device=dev)
            fit = torch.empty((n_oct, P, 2), dtype=torch.float64, device=dev)
            ws = torch.empty(2048 * P, dtype=torch.uint8, device=dev)
            for o in range(n_oct):
                # the reference's Lc of the difference image: G(sigma_2) - G(sigma_3) of the octave
                # (diff_mustache.py:315-336)
                g2[o] = self.gauss_blur(cd, lt.taps[o * lpo + 1])
                g3[o] = self.gauss_blur(cd, lt.taps[o * lpo + 2])
                _lib.check(self.lib.mst_masked_normfit(_ptr(g2[o]), _ptr(g3[o]), _ptr(nzb), _ptr(nzbc), P, CH * CH,
                                                       _ptr(fit[o]), _ptr(ws), ws.numel(), _stream()))
            ppair = torch.empty((P2, found_cap), dtype=torch.float64, device=dev)
            for off in (0, P):
                _lib.check(self.lib.mst_pair_pvalues(_ptr(found), found_cap, _ptr(count), _ptr(g2), _ptr(g3), _ptr(fit),
                                                     P, CH, n_oct, tpo, off, _ptr(ppair), _stream()))
        return ppair, fit

    def pair_pvalues_tiles(self, c, found, found_cap, count):
        """pair_pvalues for tile pairs whose difference image needs no mask beyond c != 0 (inter-chromosomal tiles,
        diff_trans.py): mst_diff_dog_tiles stages c[:P] - c[P:] in LDS and writes only D_2 per octave and norm.fit; no
        difference image, G_2 or G_3 reaches HBM.  Returns (ppair [2P, found_cap], fit) like pair_pvalues."""
        P2, CH, _ = c.shape
        P = P2 // 2
        n_oct, tpo = len(self.levels.octave_values), self.levels.s - 1
        lv = ctypes.byref(self._lv_struct)
        dev = self.device
        with torch.cuda.device(dev):
            dog = torch.empty((n_oct, P, CH, CH), dtype=torch.float64, device=dev)
            fit = torch.empty((n_oct, P, 2), dtype=torch.float64, device=dev)
            mcount = torch.empty(P, dtype=torch.int32, device=dev)
            ws_bytes = int(self.lib.mst_diff_dog_tiles_workspace_bytes(P, CH, lv))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(self.lib.mst_diff_dog_tiles(_ptr(c[:P]), _ptr(c[P:]), P, CH, lv, _ptr(dog), _ptr(fit), _ptr(mcount),
                                                   _ptr(ws), ws_bytes, _stream()))
            ppair = torch.empty((P2, found_cap), dtype=torch.float64, device=dev)
            for off in (0, P):
                _lib.check(self.lib.mst_pair_pvalues_dog(_ptr(found), found_cap, _ptr(count), _ptr(dog), _ptr(fit), P, CH,
                                                         n_oct, tpo, off, _ptr(ppair), _stream()))
        return ppair, fit

    def _pair_launch(self, bands, n, dpx, starts, CH, skip_empty, reuse=None, graph=False):
        """Enqueue a two-sample call's device work on the current stream: both samples' sigma loops in ONE fused launch
        over 2P blocks (mst_scale_space_band_pair: rows [0, P) sample 1, [P, 2P) the same windows of sample 2's band --
        one set of record buffers, so ONE mst_found_finish serves both) and, right behind it, the difference kernel
        (mst_diff_dog_band: it needs the bands only).  `graph`: the fused launch is replayed as a hipGraph.  Returns
        (launch, dog, norm.fit, keep); `keep` holds the difference kernel's other buffers until the caller is done."""
        P = len(starts)
        starts = [int(v) for v in starts]
        L = launch.ss_launch(self, launch.flags(self, skip_empty, False, graph=graph), band_src=(bands[0], int(n),
                             int(dpx), starts + starts, int(CH)), band2=(bands[1], P), reuse=reuse)
        lv = ctypes.byref(self._lv_struct)
        dev = self.device
        with torch.cuda.device(dev):
            st_arr = (ctypes.c_int64 * P)(*starts)
            dog = torch.empty((len(self.levels.octave_values), P, CH, CH), dtype=torch.float64, device=dev)
            nfit = torch.empty((len(self.levels.octave_values), P, 2), dtype=torch.float64, device=dev)
            mcount = torch.empty(P, dtype=torch.int32, device=dev)
            ws_bytes = int(self.lib.mst_diff_dog_workspace_bytes(P, CH, lv))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(self.lib.mst_diff_dog_band(_ptr(bands[0]), _ptr(bands[1]), int(n), int(dpx), st_arr, P, CH, lv,
                                                  _ptr(dog), _ptr(nfit), _ptr(mcount), _ptr(ws), ws_bytes, _stream()))
        return L, dog, nfit, (ws, mcount, st_arr)

    def _pair_pvalues(self, L, P, dog, nfit, ppair=None):
        """Differential p-values of a two-sample launch's records (mst_pair_pvalues_dog over rows [0, P), then [P, 2P))
        -> ppair [2P, cap] (device; allocated here unless given)."""
        if ppair is None:
            ppair = torch.empty((2 * P, L.cap), dtype=torch.float64, device=self.device)
        n_oct, tpo = len(self.levels.octave_values), self.levels.s - 1
        for off in (0, P):
            _lib.check(self.lib.mst_pair_pvalues_dog(_ptr(L.found), L.cap, _ptr(L.count), _ptr(dog), _ptr(nfit), P,
                                                     L.CH, n_oct, tpo, off, _ptr(ppair), _stream()))
        return ppair

    def _pair_selected(self, L, P, dog, nfit, pt, reuse=None):
        """Behind the kernels of a two-sample launch (_pair_launch), the per-chromosome driver's form: the selection
        (records.download_selected) with a finish that does not wait and the pair p-values queued in front of it, so
        that everything behind the kernels is waited for ONCE; the finish's status is checked after that wait
        (MstOverflow: the caller relaunches with larger lists).  Returns the PairBandBatch's (records, fits,
        norm.fit)."""
        nbytes = launch.summary_pin(self, L.B).numel()
        scratch, ppair = launch.carve(self, (nbytes, torch.uint8, (nbytes,)),
                                      (L.B * L.cap * 8, torch.float64, (L.B, L.cap)), reuse=reuse)
        launch.finish(self, L, wait=False, scratch=scratch)
        self._pair_pvalues(L, P, dog, nfit, ppair)
        return records.download_selected(self, L.found, L.pval, L.count, L.fit, self.levels.n_tested, L.cap, pt,
                                         pair=(ppair, P), host=functools.partial(launch.finish_landed, self, L),
                                         also=nfit, reuse=reuse)

    def run_band_pairs(self, bands, n, dpx, starts, CH, skip_empty=True, select_below=None):
        """Both samples' sigma loops straight from their bands + the pair p-values: PairBandBatch over 2P blocks whose
        records carry `pair` and `q`.  select_below = pt (what the per-chromosome driver passes): BH, the selection q <
        pt and the differential test's look-ups happen on the device and only the selected records come back, each with
        `pair`, `value` and `v_other` (the partner sample's winning value at that pixel, NaN if it did not find it);
        without it the whole found sets are downloaded, sorted by pixel (the cross-check form)."""
        P = len(starts)
        # A SMALL call (its buffers are kept between calls, launch.carve) repeats with identical arguments when the
        # caller repeats it: the two fused launches are then replayed as hipGraphs (MST_FLAG_GRAPH: uploads, counter
        # zeroing, kernel, reduction in one launch each, no dispatch gaps -- ~40 us of idle device before each kernel
        # otherwise).
        small = 2 * P * launch.found_cap_for(self, CH) * 24 + launch.workspace_bytes(self, 2 * P, CH) < (200 << 20)
        with torch.cuda.device(self.device), self._capturable_stream(small):
            L, dog, nfit, _keep = self._pair_launch(bands, n, dpx, starts, CH, skip_empty, reuse="pairs", graph=small)
            while True:
                try:
                    if select_below is not None:
                        recs, fits, norm_fit = self._pair_selected(L, P, dog, nfit, float(select_below),
                                                                   reuse="pairs-tail")
                    else:
                        launch.finish(self, L, relaunch=False)
                    break
                except _lib.MstOverflow:        # both samples again (the difference kernel's results stay valid)
                    launch.grow(self, L)
            if select_below is None:
                ppair = self._pair_pvalues(L, P, dog, nfit)
                recs, fits = records.download_found(
                    self, L.found, L.pval, L.count, L.fit, self.levels.n_tested, sort=True, host=(L.count_h, L.fit_h),
                    extra={"pair": ppair, "q": records.fdr(self, L.pval, L.count, L.cap)})
                norm_fit = nfit.cpu().numpy()
        batch = PairBandBatch(self, bands, n, dpx, starts, CH, L.nz_h, recs, fits)
        batch.norm_fit = norm_fit
        return batch

    def run_band_pairs_overlapped(self, bands, n, dpx, groups, CH, skip_empty=True, select_below=None):
        """run_band_pairs over several groups of block pairs with the device work of group i + 1 queued BEFORE the
        results of group i are collected (_ping_pong): the groups' kernels (both samples' sigma loops + the difference
        kernel) run back to back while the caller's host tail of the previous group -- and its small gathers on the
        caller's stream -- proceed.  Yields one PairBandBatch per group, identical to run_band_pairs(group)."""
        if len(groups) <= 1 or select_below is None:
            for starts in groups:
                yield self.run_band_pairs(bands, n, dpx, starts, CH, skip_empty=skip_empty, select_below=select_below)
            return

        def collect(starts, work):
            L, dog, nfit, _keep = work
            try:
                recs, fits, norm_fit = self._pair_selected(L, len(starts), dog, nfit, float(select_below))
            except _lib.MstOverflow:
                # more room from now on, and this group redone the plain way
                launch.grow(self, L, relaunch=False)
                return self.run_band_pairs(bands, n, dpx, starts, CH, skip_empty=skip_empty, select_below=select_below)
            batch = PairBandBatch(self, bands, n, dpx, starts, CH, L.nz_h, recs, fits)
            batch.norm_fit = norm_fit
            return batch

        yield from self._ping_pong(
            groups, lambda gi, starts: self._pair_launch(bands, n, dpx, starts, CH, skip_empty), collect)

    def run_filled_pairs(self, c, nz, nz_count, skip_empty=True, tiles=False):
        """The reference's dense two-sample data flow (the cross-check of run_band_pairs): c [2P, CH, CH] filled blocks
        (sample 1 first, then sample 2), nz their masks, nz_count their tested-pixel counts (device).  BlockBatch over
        all 2P blocks whose records also carry `pair` (the differential p-value) and `q`.  tiles=True: nz is c != 0
        (inter-chromosomal tiles) and the pair p-values come from the fused kernel (pair_pvalues_tiles)."""
        found, pval, count, fit, cap = self.sigma_loop(c, nz, nz_count, skip_empty=skip_empty, download=False)
        ppair, nfit = self.pair_pvalues_tiles(c, found, cap, count) if tiles else self.pair_pvalues(c, nz, found, cap, count)
        recs, fits = records.download_found(self, found, pval, count, fit, self.levels.n_tested, sort=True,
                                            extra={"pair": ppair, "q": records.fdr(self, pval, count, cap)})
        B, CH, _ = c.shape
        batch = BlockBatch(self, c, nz, CH, B, nz_count, recs, fits)
        batch.norm_fit = nfit.cpu().numpy()
        return batch

    def run_block_pairs(self, c, dpx, intra=True, skip_empty=True):
        """c: [2P, CH, CH] raw blocks (sample 1 first, then sample 2), mutated in place -> run_filled_pairs."""
        return self.run_filled_pairs(c, *self.prologue(c, dpx, intra), skip_empty=skip_empty)

    def run_blocks(self, c, dpx, intra=True, skip_empty=True):
        """c: [B, CH, CH] float64 device tensor holding raw (normalised, un-filled) blocks; mutated in place
        like the reference mutates its block (mustache.py:703-706)."""
        nz, nz_count = self.prologue(c, dpx, intra)
        found, fits = self.sigma_loop(c, nz, nz_count, skip_empty=skip_empty)
        B, CH, _ = c.shape
        return BlockBatch(self, c, nz, CH, B, nz_count, found, fits)
