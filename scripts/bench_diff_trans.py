#!/usr/bin/env python3
"""The difference image's D_2 and norm.fit for inter-chromosomal tile pairs, two ways on the same tiles (default: 64 pairs of
2000 x 2000, octaves 1.6 / 3.2):

  fused   mst_diff_dog_tiles: the difference image and its blurs live in LDS; per pair 2 images read, n_oct written
  dense   mst_diff_image, two mst_gauss_blur per octave, mst_masked_normfit (engine.pair_pvalues without its p-value
          kernel): the difference image, every blur's intermediate, G_2 and G_3 go through HBM; per pair about 1 + 6 n_oct
          images moved beyond the two it reads

Both give the same D_2 (checked bit for bit here) and the same fit.  Timed with device events around each form, the two forms
alternating, after a warm-up of both; then the whole two-sample call (call_diff_trans_coo) on the 2 x 2 production case of
tests/diff_trans_reference.py, in Gpix-pairs/s (tile pairs x C^2 over the call's wall time, device synchronised).

Prints one JSON line.  Needs the GPU: there is no other path.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--size", type=int, default=2000)
    ap.add_argument("--octaves", type=float, nargs="+", default=[1.6, 3.2])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--density", type=float, default=0.3)
    ap.add_argument("--no-call", action="store_true", help="skip the whole-call timing")
    args = ap.parse_args()

    import torch
    from mustache_amd import _lib
    from mustache_amd._lib import ptr as _ptr, stream as _stream
    from mustache_amd.engine import ScaleSpaceEngine
    if not torch.cuda.is_available():
        raise SystemExit("bench_diff_trans.py needs the GPU")
    eng = ScaleSpaceEngine(args.octaves)
    lib, lt = eng.lib, eng.levels
    P, C, n_oct, lpo = args.pairs, args.size, len(args.octaves), eng.levels.levels_per_octave
    dev = eng.device
    gen = torch.Generator(device=dev).manual_seed(1)
    c = torch.empty((2 * P, C, C), dtype=torch.float64, device=dev)
    for p in range(P):                                       # pair by pair: no stack-sized temporaries
        a = torch.randn((C, C), generator=gen, dtype=torch.float64, device=dev)
        keep = torch.rand((C, C), generator=gen, device=dev) < args.density
        c[p] = torch.where(keep, a, torch.zeros_like(a))
        b = a + 0.3 * torch.randn((C, C), generator=gen, dtype=torch.float64, device=dev)
        keep = torch.rand((C, C), generator=gen, device=dev) < args.density
        c[P + p] = torch.where(keep, b, torch.zeros_like(b))
    del a, b, keep
    nz = torch.empty((2 * P, C, C), dtype=torch.uint8, device=dev)
    nzc = torch.empty(2 * P, dtype=torch.int32, device=dev)
    _lib.check(lib.mst_trans_prologue(_ptr(c), _ptr(nz), _ptr(nzc), 2 * P, C, _stream()))
    lv = ctypes.byref(eng._lv_struct)

    dog = torch.empty((n_oct, P, C, C), dtype=torch.float64, device=dev)
    fit_f = torch.empty((n_oct, P, 2), dtype=torch.float64, device=dev)
    mcount = torch.empty(P, dtype=torch.int32, device=dev)
    wsb = int(lib.mst_diff_dog_tiles_workspace_bytes(P, C, lv))
    ws_f = torch.empty(wsb, dtype=torch.uint8, device=dev)

    def fused():
        _lib.check(lib.mst_diff_dog_tiles(_ptr(c[:P]), _ptr(c[P:]), P, C, lv, _ptr(dog), _ptr(fit_f), _ptr(mcount), _ptr(ws_f),
                                          wsb, _stream()))

    cd = torch.empty((P, C, C), dtype=torch.float64, device=dev)
    nzb = torch.empty((P, C, C), dtype=torch.uint8, device=dev)
    nzbc = torch.empty(P, dtype=torch.int32, device=dev)
    g2 = torch.empty((n_oct, P, C, C), dtype=torch.float64, device=dev)
    g3 = torch.empty((n_oct, P, C, C), dtype=torch.float64, device=dev)
    tmp = torch.empty((P, C, C), dtype=torch.float64, device=dev)
    fit_d = torch.empty((n_oct, P, 2), dtype=torch.float64, device=dev)
    ws_d = torch.empty(2048 * P, dtype=torch.uint8, device=dev)
    taps = [[(ctypes.c_double * len(t))(*[float(v) for v in t]) for t in (lt.taps[o * lpo + 1], lt.taps[o * lpo + 2])]
            for o in range(n_oct)]

    def dense():
        _lib.check(lib.mst_diff_image(_ptr(c[:P]), _ptr(c[P:]), _ptr(nz[:P]), _ptr(nz[P:]), P, C, _ptr(cd), _ptr(nzb), _ptr(nzbc),
                                      _stream()))
        for o in range(n_oct):
            for g, t in ((g2[o], taps[o][0]), (g3[o], taps[o][1])):
                _lib.check(lib.mst_gauss_blur(_ptr(cd), _ptr(g), _ptr(tmp), P, C, C, t, len(t) - 1, _stream()))
            _lib.check(lib.mst_masked_normfit(_ptr(g2[o]), _ptr(g3[o]), _ptr(nzb), _ptr(nzbc), P, C * C, _ptr(fit_d[o]), _ptr(ws_d),
                                              ws_d.numel(), _stream()))

    for _ in range(args.warmup):
        fused()
        dense()
    torch.cuda.synchronize()
    same = all(bool(torch.equal(g2[o] - g3[o], dog[o])) for o in range(n_oct))
    fit_gap = float(((fit_f - fit_d).abs() / fit_d[..., 1:].abs()).max())
    times = {"fused": [], "dense": []}
    for _ in range(args.reps):
        for name, fn in (("fused", fused), ("dense", dense)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e-3)
    image = 8.0 * P * C * C
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    model = {"fused": (2 + n_oct) * image, "dense": (2 + 1 + 6 * n_oct) * image}
    out = {
        "pairs": P, "size": C, "octaves": args.octaves, "d2_bit_identical": same, "fit_max_gap_over_scale": fit_gap,
        "fused_s": med["fused"], "dense_s": med["dense"], "fused_s_all": times["fused"], "dense_s_all": times["dense"],
        "dense_over_fused": med["dense"] / med["fused"],
        "fused_model_GBps": model["fused"] / med["fused"] / 1e9, "dense_model_GBps": model["dense"] / med["dense"] / 1e9,
        "fused_Gpix_pairs_per_s": P * C * C / med["fused"] / 1e9,
    }
    del cd, nzb, g2, g3, tmp, dog, c, nz
    torch.cuda.empty_cache()

    if not args.no_call:
        import diff_trans_reference as dr
        from mustache_amd.diff_trans import call_diff_trans_coo
        from mustache_amd.trans import trans_tiling
        case = dr.CASES["production_2x2"]
        rec1, rec2 = dr.case_records("production_2x2")
        Cc, (rs, _), (cs, _) = trans_tiling(case["n1"], case["n2"], case["chunk"])
        call_t, rows = [], None
        for i in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = call_diff_trans_coo(rec1, rec2, case["oct"], dr.ST, dr.PT, dr.PT2, chunk=case["chunk"])
            torch.cuda.synchronize()
            if i >= args.warmup:
                call_t.append(time.perf_counter() - t0)
        m = sorted(call_t)[len(call_t) // 2]
        out.update({"call_case": "production_2x2", "call_tile_pairs": len(rs) * len(cs), "call_rows": len(rows), "call_s": m,
                    "call_s_all": call_t, "call_Gpix_pairs_per_s": len(rs) * len(cs) * Cc * Cc / m / 1e9})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
