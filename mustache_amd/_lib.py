"""ctypes binding of libmustache_hip.so (include/mustache_hip.h).  There is no CPU fallback: if the HIP library is
missing or stale the import fails loudly."""
import ctypes
import os

MST_MAX_LEVELS = 64
MST_MAX_RADIUS = 32
MST_MAX_TESTED = 48
MST_ABI_VERSION = 3
MST_ABI_REVISION = 1         # include/mustache_hip.h: entry points added since the version last changed

MST_OK, MST_E_ARG, MST_E_HIP, MST_E_OVERFLOW, MST_E_NONFINITE = 0, -1, -2, -3, -4

# flag words of the launches and of mst_found_finish (include/mustache_hip.h: same names, same values)
MST_FLAG_SKIP_EMPTY, MST_FLAG_FMA, MST_FLAG_NO_SHARE, MST_FLAG_GRAPH, MST_FLAG_NO_WAIT = 1, 2, 4, 8, 16
MST_BH_RETRY = 0xFFFFFFFF      # mst_bh_select_nowait: out_count of a block whose candidate subset exceeds lds_records

_HERE = os.path.dirname(os.path.abspath(__file__))
# MUSTACHE_HIP_LIB: developer override to A/B alternative builds of the same ABI (still an in-tree HIP library)
LIB_PATH = os.environ.get("MUSTACHE_HIP_LIB") or os.path.join(_HERE, "libmustache_hip.so")


class MstLevels(ctypes.Structure):
    _fields_ = [
        ("n_octaves", ctypes.c_int32),
        ("levels_per_octave", ctypes.c_int32),
        ("radius", ctypes.c_int32 * MST_MAX_LEVELS),
        ("_pad", ctypes.c_int32),
        ("sigma", ctypes.c_double * MST_MAX_LEVELS),
        ("taps", (ctypes.c_double * (MST_MAX_RADIUS + 1)) * MST_MAX_LEVELS),
    ]


class MstError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libmustache_hip error %d: %s" % (code, msg))
        self.code = code


class MstOverflow(MstError):
    pass


_p = ctypes.c_void_p
_i32 = ctypes.c_int32
_u32 = ctypes.c_uint32
_i64 = ctypes.c_int64
_u64 = ctypes.c_uint64

_SIGNATURES = {
    "mst_abi_version": (ctypes.c_int, []),
    "mst_abi_revision": (ctypes.c_int, []),
    "mst_last_error": (ctypes.c_char_p, []),
    "mst_scatter_blocks": (ctypes.c_int, [_p, _p, _p, _i64, ctypes.POINTER(_i64), _i32, _i32, _p, _p]),
    "mst_block_prologue": (ctypes.c_int, [_p, _p, _p, _i32, _i32, _i32, _i32, _p]),
    "mst_gauss_blur": (ctypes.c_int, [_p, _p, _p, _i32, _i32, _i32, ctypes.POINTER(ctypes.c_double), _i32, _p]),
    "mst_scale_space": (ctypes.c_int, [_p, _p, _i32, _i32, ctypes.POINTER(MstLevels), _p, _u32, _p, _p, _i32, _p,
                                       _u64, _p]),
    "mst_scale_space_workspace_bytes": (_u64, [_i32, _i32, ctypes.POINTER(MstLevels)]),
    "mst_found_pvalues": (ctypes.c_int, [_p, _u32, _p, _p, _p, _i32, _i32, _p, _p, _p]),
    "mst_found_summary_bytes": (_u64, [_i32]),
    "mst_found_finish": (ctypes.c_int, [_p, _u32, _p, _p, _p, _i32, _i32, _p, _p, _u32, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _p]),
    "mst_bh_workspace_bytes": (_u64, [_i32, _u32]),
    "mst_bh_fdr": (ctypes.c_int, [_p, _p, _i32, _u32, _p, _p, _u64, _p]),
    "mst_bh_select": (ctypes.c_int, [_p, _p, _p, _i32, _u32, ctypes.c_double, _u32, _p, _p, _p, _p, _p, _u64, _p]),
    "mst_scale_space_band_tiles": (ctypes.c_int, [_i32, _i32, _p, _p]),
    "mst_scale_space_band_items": (ctypes.c_int, [ctypes.POINTER(_i64), _i32, _i32, _i32, _p, _i32, _p, _p]),
    "mst_bh_select_records": (ctypes.c_int, [_p, _p, _p, _i32, _u32, ctypes.c_double, _u32, _p, _p, _p, _p, _p, _p, _u64, _p]),
    "mst_bh_select_nowait": (ctypes.c_int, [_p, _p, _p, _i32, _u32, ctypes.c_double, _u32, _p, _p, _p, _p, _p, _u32, _p, _u64, _p]),
    "mst_found_summary_status": (ctypes.c_int, [_p, _u32]),
    "mst_select_below": (ctypes.c_int, [_p, _p, _p, _i32, _u32, ctypes.c_double, _u32, _p, _p, _p, _p, _p]),
    "mst_candidate_features": (ctypes.c_int, [_p, _p, _i32, _i32, _p, _p, _i32, _p, _p, _p, _p]),
    "mst_gather_diagonals": (ctypes.c_int, [_p, _i32, _i32, _p, _i32, _p, _p]),
    "mst_band_from_coo": (ctypes.c_int, [_p, _p, _p, _i64, _i64, _i32, _p, _p]),
    "mst_band_from_packed": (ctypes.c_int, [_p, _p, _p, _i64, _i64, _i32, _p, _p]),
    "mst_band_scatter_packed": (ctypes.c_int, [_p, _p, _i32, _p, _i64, _i64, _i32, _p, _p]),
    "mst_band_verify_packed": (ctypes.c_int, [_p, _p, _i32, _p, _i64, _i64, _i32, _p, _p, _p]),
    "mst_band_scatter_hic_rows": (ctypes.c_int, [_p, _p, _i32, _p, _i64, _i64, _i64, _i64, _i32, _p, _p, _i32, _p]),
    "mst_band_to_coo": (ctypes.c_int, [_p, _p, _p, _i64, _i64, _i32, _p, _p]),
    "mst_normalize_band": (ctypes.c_int, [_p, _p, _i64, _i32, _i32, _i32, _p, _p]),
    "mst_blocks_from_band": (ctypes.c_int, [_p, _i64, _i32, ctypes.POINTER(_i64), _i32, _i32, _p, _p, _p, _p]),
    "mst_scale_space_band": (ctypes.c_int, [_p, _i64, _i32, ctypes.POINTER(_i64), _i32, _i32, ctypes.POINTER(MstLevels), _p,
                                            _u32, _p, _p, _p, _i32, _p, _u64, _p]),
    "mst_scale_space_band_stage": (ctypes.c_int, [_p, _i64, _i32, ctypes.POINTER(_i64), _i32, _i32, ctypes.POINTER(MstLevels), _p,
                                                  _u32, _p, _p, _p, _i32, _p, _u64, ctypes.POINTER(_i32), _i32, _i32, _p]),
    "mst_scale_space_band_pair": (ctypes.c_int, [_p, _p, _i32, _i64, _i32, ctypes.POINTER(_i64), _i32, _i32, ctypes.POINTER(MstLevels),
                                                 _p, _u32, _p, _p, _p, _i32, _p, _u64, _p]),
    "mst_candidate_features_band": (ctypes.c_int, [_p, _i64, _i32, _i64, _i32, _p, _p, _i32, _p, _p, _p, _p]),
    "mst_candidate_features_band_multi": (ctypes.c_int, [_p, _i64, _i32, _p, _i32, _p, _p, _i32, _p, _p, _p, _p]),
    "mst_gather_diagonals_band": (ctypes.c_int, [_p, _i64, _i32, _i64, _i32, _p, _i32, _p, _p]),
    "mst_diag_means": (ctypes.c_int, [_p, _i32, _i32, _p, _i32, _p, _p]),
    "mst_diag_means_band": (ctypes.c_int, [_p, _i64, _i32, _i64, _i32, _p, _i32, _p, _p]),
    "mst_diag_means_band_multi": (ctypes.c_int, [_p, _i64, _i32, _p, _i32, _p, _i32, _p, _p]),
    "mst_cluster_workspace_bytes": (_u64, [_u32]),
    "mst_cluster_representatives": (ctypes.c_int, [_p, _p, _p, _p, _p, _i32, _i32, _u32, _p, _p, _p, _u64, _p]),
    "mst_diff_image": (ctypes.c_int, [_p, _p, _p, _p, _i32, _i32, _p, _p, _p, _p]),
    "mst_masked_normfit": (ctypes.c_int, [_p, _p, _p, _p, _i32, _i64, _p, _p, _u64, _p]),
    "mst_diff_dog_workspace_bytes": (_u64, [_i32, _i32, ctypes.POINTER(MstLevels)]),
    "mst_diff_dog_band": (ctypes.c_int, [_p, _p, _i64, _i32, ctypes.POINTER(_i64), _i32, _i32, ctypes.POINTER(MstLevels),
                                         _p, _p, _p, _p, _u64, _p]),
    "mst_diff_dog_tiles_workspace_bytes": (_u64, [_i32, _i32, ctypes.POINTER(MstLevels)]),
    "mst_diff_dog_tiles": (ctypes.c_int, [_p, _p, _i32, _i32, ctypes.POINTER(MstLevels), _p, _p, _p, _p, _u64, _p]),
    "mst_pair_pvalues_dog": (ctypes.c_int, [_p, _u32, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _p, _p]),
    "mst_pair_gather": (ctypes.c_int, [_p, _u32, _p, _p, _i32, _p, _p, _p, _u32, _u32, _p, _p, _p, _p]),
    "mst_pair_pvalues": (ctypes.c_int, [_p, _u32, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _p, _p]),
    "mst_balance_workspace_bytes": (_u64, [_i64, _i64]),
    "mst_balance_marginals": (ctypes.c_int, [_p, _p, _p, _p, _p, _i64, _i64, _p, _p, _p, _p, _u64, _p]),
    "mst_balance_iterate": (ctypes.c_int, [_p, _p, _p, _p, _p, _i64, _i64, _p, _i32, _i32, ctypes.c_double, _p, _p, _u64, _p]),
    "mst_balance_newton_workspace_bytes": (_u64, [_i64, _i64]),
    "mst_balance_newton": (ctypes.c_int, [_p, _p, _p, _p, _p, _i64, _i64, _p, _i32, _i32, ctypes.c_double, _p, _p, _i32, _p, _u64,
                                          _p]),
    "mst_balance_bias": (ctypes.c_int, [_p, _p, _p, _p, _p, _i64, _i64, _p, _p, _p, _p, _u64, _p]),
    "mst_balance_apply_packed": (ctypes.c_int, [_p, _p, _p, _i64, _p, _i64, _p, _p]),
    "mst_balance_apply_pairs": (ctypes.c_int, [_p, _p, _p, _i64, _p, _p, _p, _i32, _p, _i64, _p, _p]),
    "mst_trans_decode_hic_rows": (ctypes.c_int, [_p, _p, _i32, _p, _i64, _p, _i64, _i32, _p, _p, _p, _i64, _p, _p]),
    "mst_trans_zscore_workspace_bytes": (_u64, []),
    "mst_trans_zscore": (ctypes.c_int, [_p, _i64, _p, _p, _p, _u64, _p]),
    "mst_trans_scatter_tiles": (ctypes.c_int, [_p, _p, _p, _i64, _p, _p, _i32, _i32, _p, _p]),
    "mst_trans_prologue": (ctypes.c_int, [_p, _p, _p, _i32, _i32, _p]),
    "mst_trans_zscore_segmented_workspace_bytes": (_u64, [_i32]),
    "mst_trans_zscore_segmented": (ctypes.c_int, [_p, _p, _p, _i64, _p, _i32, _p, _p, _p, _p, _u64, _p]),
    "mst_trans_count_tiles": (ctypes.c_int, [_p, _p, _p, _i64, _p, _p, _i32, _i64, _p, _p]),
    "mst_trans_scatter_worklist": (ctypes.c_int, [_p, _p, _p, _p, _p, _i32, _i32, _i64, _i64, _p, _i32, _i32, _p, _p]),
    "mst_pileup_workspace_bytes": (_u64, [_i64, _i32, _i64, _i32]),
    "mst_pileup_expected": (ctypes.c_int, [_p, _i64, _i32, _i32, _p, _p, _p, _u64, _p]),
    "mst_pileup_windows": (ctypes.c_int, [_p, _i64, _i32, _i32, _p, _p, _p, _i64, _i32, _i32, _p, _p, _p, _p]),
    "mst_pileup_reduce": (ctypes.c_int, [_p, _p, _p, _i64, _i32, _p, _p, _u64, _p]),
    "mst_pileup_trans_workspace_bytes": (_u64, [_i64, _i64, _i64, _i32]),
    "mst_pileup_trans_windows": (ctypes.c_int, [_p, _p, _p, _i64, _i64, _i64, _p, _p, _i64, _i32, _i32, _p, _p, _p, _p, _p, _p, _p,
                                                _u64, _p]),
    "mst_pileup_trans_batch_workspace_bytes": (_u64, [_p, _p, _p, _i32, _i32]),
    "mst_pileup_trans_batch": (ctypes.c_int, [_p, _p, _p, _i64, _p, _p, _p, _p, _p, _i64, _p, _i32, _i32, _i32, _p, _p, _p, _p, _p,
                                              _p, _p, _p, _u64, _p]),
    "mst_pileup_reduce_segmented_workspace_bytes": (_u64, [_p, _i32, _i32]),
    "mst_pileup_reduce_segmented": (ctypes.c_int, [_p, _p, _p, _i64, _p, _i32, _i32, _p, _p, _u64, _p]),
    "mst_pileup_enrich": (ctypes.c_int, [_p, _i64, _i32, _i32, _p, _i32, _p, _p, _p, _p, _p]),
    "mst_pileup_centre_counts": (ctypes.c_int, [_p, _p, _p, _i32, _i64, _p, _i64, _i32, _i32, _p, _p, _p]),
    "mst_pileup_poisson": (ctypes.c_int, [_p, _p, _p, _p, _p, _i64, _p, _p, _i64, _p, _p, _p, _p, _p, _p]),
    "mst_pileup_compare": (ctypes.c_int, [_p, _p, _i64, _i32, _i32, _p, _p]),
    "mst_pileup_reduce_pair": (ctypes.c_int, [_p, _p, _p, _i64, _i32, _p, _p, _u64, _p]),
    "mst_pairs_bin": (ctypes.c_int, [_p, _p, _i64, _i32, _i32, _i64, _i64, _i32, _p, _p, _p, _i64, _p, _p]),
    "mst_pairs_compact_workspace_bytes": (_u64, [_i32, _i64]),
    "mst_pairs_compact": (ctypes.c_int, [_p, _i32, _i64, _p, _p, _p, _i64, _p, _p, _u64, _p]),
    "mst_pairs_bin_trans": (ctypes.c_int, [_p, _p, _i64, _p, _i32, _p, _p, _p, _p, _p, _i32, _i32, _i64, _p, _p, _p, _i64, _p, _p, _p]),
    "mst_pairs_trans_compact_workspace_bytes": (_u64, [_i64]),
    "mst_pairs_trans_compact": (ctypes.c_int, [_p, _i64, _p, _p, _i64, _p, _p, _u64, _p]),
    "mst_pairs_trans_decode": (ctypes.c_int, [_p, _p, _i64, _p, _p, _i32, _p, _p, _p, _p]),
    "mst_thin_counts": (ctypes.c_int, [_p, _p, _p, _i32, _i64, _u32, _u32, _u32, _u64, _p, _p, _p]),
    "mst_thin_pairs": (ctypes.c_int, [_p, _p, _p, _i32, _i64, _p, _p, _i32, _u32, _u32, _u64, _p, _p, _i32, _p]),
    "mst_coarsen_records": (ctypes.c_int, [_p, _p, _p, _i32, _i64, _i32, _i64, _i32, _p, _p, _p, _i64, _p, _p]),
    "mst_coarsen_compact_workspace_bytes": (_u64, [_i32, _i64]),
    "mst_coarsen_compact": (ctypes.c_int, [_p, _i32, _i64, _p, _p, _p, _i64, _p, _p, _u64, _p]),
    "mst_coarsen_pairs": (ctypes.c_int, [_p, _p, _p, _i32, _i64, _p, _p, _p, _p, _i32, _i32, _i64, _p, _p, _p, _i64, _p, _i32, _p]),
    "mst_coarsen_pairs_compact_workspace_bytes": (_u64, [_i64]),
    "mst_coarsen_pairs_compact": (ctypes.c_int, [_p, _i64, _p, _p, _i64, _p, _p, _u64, _p]),
}

_lib = None


def load():
    """Load the shared library once; raise if it is absent (build it with `python -c 'import __graft_entry__ as g;
    g.build()'` or `make -C mustache_amd/csrc`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "mustache_amd: %s not found -- the HIP extension is required (no CPU fallback). "
            "Build it with `make -C mustache_amd/csrc` (hipcc, --offload-arch=gfx950)." % LIB_PATH)
    # PyTorch-ROCm ships its own libamdhip64.so.7; it must be in the process BEFORE our library is opened so that
    # the dynamic linker binds us to that same runtime instance (one HIP runtime per process, shared streams and
    # allocations).  Opening ours first would pull in /opt/rocm's copy and leave two runtimes fighting over the GPU.
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    # the version first: a stale library names itself before any symbol it lacks is looked up (a library from before
    # mst_abi_revision existed is revision 0)
    lib.mst_abi_version.restype = ctypes.c_int
    have = (lib.mst_abi_version(), lib.mst_abi_revision() if hasattr(lib, "mst_abi_revision") else 0)
    if have != (MST_ABI_VERSION, MST_ABI_REVISION):
        raise ImportError("mustache_amd: ABI version mismatch (library %d.%d, binding %d.%d): rebuild %s"
                          % (have + (MST_ABI_VERSION, MST_ABI_REVISION, LIB_PATH)))
    missing = []
    for name, (res, args) in _SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            missing.append(name)
            continue
        fn.restype = res
        fn.argtypes = args
    if missing:
        raise ImportError("mustache_amd: %s lacks symbols %s (stale build?)" % (LIB_PATH, missing))
    _lib = lib
    return lib


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("mustache_amd needs a ROCm GPU (MI355X/gfx950); no CPU fallback exists")
    return load()


def ptr(t):
    """Pointer of tensor t (device or page-locked host memory) as the C ABI takes it; None stays None."""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def off(t, n):
    """Device pointer of element n of tensor t."""
    return ctypes.c_void_p(t.data_ptr() + n * t.element_size())


def stream():
    """The current torch stream as the C ABI takes it."""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def exported_symbols():
    return sorted(_SIGNATURES)


def check(rc):
    if rc == MST_OK:
        return
    msg = load().mst_last_error().decode("utf-8", "replace")
    if rc == MST_E_OVERFLOW:
        raise MstOverflow(rc, msg)
    raise MstError(rc, msg)


# ---- stage markers (observability).  MUSTACHE_ROCTX=1: the host stages of a run (read / normalise / scale-space /
# tail) are pushed as roctx ranges through librocprofiler-sdk-roctx, so `rocprofv3 --marker-trace --kernel-trace` shows them above
# the kernels (the PROFILE library marks its entry points the same way).  Off by default: no library is loaded, no call is made.
_ROCTX = None


class stage:
    """with stage("read"): ...   -- a roctx range when MUSTACHE_ROCTX=1, nothing otherwise"""
    __slots__ = ("name", "on")

    def __init__(self, name):
        self.name, self.on = name, False

    def __enter__(self):
        global _ROCTX
        if os.environ.get("MUSTACHE_ROCTX") == "1":
            if _ROCTX is None:
                try:
                    _ROCTX = ctypes.CDLL("librocprofiler-sdk-roctx.so")
                    _ROCTX.roctxRangePushA.argtypes = [ctypes.c_char_p]
                except OSError:
                    _ROCTX = False
            if _ROCTX:
                _ROCTX.roctxRangePushA(("mustache: " + self.name).encode())
                self.on = True
        return self

    def __exit__(self, *exc):
        if self.on:
            _ROCTX.roctxRangePop()
        return False
