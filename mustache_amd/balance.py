"""Balancing of one chromosome's intra-chromosomal map on the GPU, for maps that come without a bias vector: `--balance ICE`
(iterative correction) or `--balance NEWTON` (Knight & Ruiz's Newton iteration) on the command lines, `ice()` and `newton()`
in Python.  Both solve x_i (A x)_i = const, which has one solution up to the scale that kappa fixes; ICE converges linearly,
NEWTON quadratically.

The algorithm (modelled on the defaults of `cooler balance --cis-only`; tests/balance_reference.py restates it in NumPy):

Input: the chromosome's whole upper-triangular pixel set (i <= j; entries with v <= 0 or a non-finite v are dropped) and the
bin count n.  A repeated pixel (same (min, max) in either orientation) counts once, the last entry in input order wins.
Every step runs on the full symmetric matrix A (an off-diagonal pixel is in row i and in row j).
  1. drop the pixels with j - i < ignore_diags;
  2. mask the bins whose row has fewer than min_nnz non-zeros;
  3. m = the row sums with the masked rows and columns removed;
  4. over the bins with m > 0: l = log m, med = median(l), mad = median(|l - med|); mask the bins with
     m < exp(med - mad_max * mad) and the bins with m = 0;
  5. (ICE) w = 1 on unmasked bins, 0 on masked; for k = 1 .. max_iter: s = w * (A w); mu = mean(s[s != 0]); r = s / mu where
     s != 0, 1 elsewhere; w /= r; var = population variance of r[s != 0] (0 when no s is non-zero); stop when var < tol;
  6. b = kappa / w on unmasked bins, NaN on masked, kappa = sqrt(sum A_ij w_i w_j / sum A_ij) over the kept pixels i <= j: the
     balanced total equals the raw total (Juicer's scale, so read_bias' 0.2 cut-off means what it means for a KR vector).
The bias is applied exactly as a `-b` vector (mustache.read_pd): v' = (v / b[bin of pos1]) / b[bin of pos2], NaN or b < 0.2
count as +inf, v' > 0 kept.

NEWTON replaces step 5 (tests/newton_reference.py restates it in NumPy).  K: the unmasked bins.  Act = {i in K :
(A 1_K)_i != 0}; the bins of K outside Act ("isolated": every partner is masked) keep x = 1, as ICE leaves w = 1 there, and
take part in nothing.  Every vector lives on Act; A is the kept symmetric matrix restricted to K.  delta = 0.1, Delta = 3,
g = 0.9, etamax = 0.1; tol = 1e-6 and max_matvecs = 2000 are keywords.
    x = 1; v = x * (A x); r = 1 - v; rho = rout = r.r; eta = etamax; rold = rout
    while rout > tol^2 and matvecs < max_matvecs:                       # outer (Newton) iteration
        y = 1; k = 0; innertol = max(eta^2 * rout, tol^2)
        while rho > innertol and matvecs < max_matvecs:                 # inner (CG) iteration, Jacobi-preconditioned by v
            k += 1
            if k == 1: z = r / v; p = z; rho = r.z
            else:      p = z + (rho / rho_prev) * p
            w = x * (A (x * p)) + v * p; matvecs += 1
            if p.w is not positive and finite: stop, converged = False
            alpha = rho / (p.w); ap = alpha * p; ynew = y + ap
            if min(ynew) <= delta: y += min over {ap_i < 0} of (delta - y_i) / ap_i * ap; leave the inner loop (a capped step)
            if max(ynew) >= Delta: y += min over {ynew_i > Delta} of (Delta - y_i) / ap_i * ap; leave the inner loop (capped;
                                   the factor is 1 when the set is empty, that is when max(ynew) = Delta exactly)
            y = ynew; r -= alpha * w; rho_prev = rho; z = r / v; rho = r.z
        x = x * y; v = x * (A x); matvecs += 1; r = 1 - v; rho = rout = r.r
        rat = rout / rold; rold = rout; eta_o = eta; eta = g * rat
        if g * eta_o^2 > 0.1: eta = max(eta, g * eta_o^2)
        eta = max(min(eta, etamax), 0.5 * tol / sqrt(rout))
    converged = rout <= tol^2;  w = x on Act, 1 on isolated bins, 0 on masked bins; step 6 follows unchanged.

Device work (mustache_amd/csrc/mst_balance.hip): the filter-stage row sums and non-zero counts, either iteration with its
scalars and its stop test (ICE: mean, variance; NEWTON: every dot product, min/max, cap factor, forcing term and the
inner/outer control flow, in a state record the host only reads between batches of STEPS_PER_READ steps), kappa and the bias,
and the application to `.hic` records.  Every sum has a fixed order that
depends only on absolute bin and pixel positions, so the bias is bit-identical from run to run, under any permutation of the
records, for any n, and whichever reader the pixels came from.  torch does the one-off sort and the CSR offsets; the median
of step 4 runs on the host (NumPy).
"""
import ctypes
import math

import numpy as np

METHODS = ("ICE", "NEWTON")
CHUNK = 1024                 # entries per chunk of a CSR row (kChunk in mst_balance.hip)
STEPS_PER_READ = 8           # iterations (NEWTON: steps) enqueued between two reads of the device's state record


class BalanceError(ValueError):
    """A --balance request that conflicts with another option."""


def check_request(method, path=None, bias=None, norm_method=None, world=1, bias_flag="-b"):
    """Raise BalanceError naming the conflict when `--balance method` cannot be honoured; return the method (upper case)."""
    m = str(method).upper()
    if m not in METHODS:
        raise BalanceError("--balance %s: unknown method (supported: %s)" % (method, ", ".join(METHODS)))
    if bias:
        raise BalanceError("--balance %s and %s: give either a bias file or --balance, not both" % (m, bias_flag))
    if norm_method and str(norm_method).upper() != "NONE":
        raise BalanceError("--balance %s and -norm %s: --balance reads raw counts; leave -norm unset or NONE"
                           % (m, norm_method))
    for p in ([path] if isinstance(path, str) else list(path or [])):
        if str(p).endswith((".cool", ".mcool")):
            raise BalanceError("--balance %s and %s: .cool/.mcool files carry their own `weight` column; "
                               "--balance is for text and .hic input" % (m, p))
    if world > 1:
        raise BalanceError("--balance %s in a multi-rank run (world size %d): balancing runs on one GPU; "
                           "start a single process" % (m, world))
    return m


def method_of(balance):
    """The method a reader's `balance=` argument names: the string itself, ICE for any other true value."""
    return balance.upper() if isinstance(balance, str) else "ICE"


# ----------------------------------------------------------------------------------------------------------------------
# bias vectors as files and as read_pd's lookup
# ----------------------------------------------------------------------------------------------------------------------
def write_bias(path, chrom, res, bias):
    """The 3-column bias file read_bias reads: `chrom<TAB>start_bp<TAB>repr(value)`, one line per bin, `nan` on masked bins.
    repr() round-trips every float64, so read_bias reads back exactly these values."""
    res = int(res)
    with open(path, "w") as f:
        f.write("".join("%s\t%d\t%r\n" % (chrom, i * res, float(b)) for i, b in enumerate(np.asarray(bias, np.float64))))


def bias_lookup(bias):
    """bin -> factor exactly as read_bias builds it from a file holding `bias` (NaN or < 0.2 -> +inf, other bins 1.0)."""
    from collections import defaultdict
    d = defaultdict(lambda: 1.0)
    for i, val in enumerate(np.asarray(bias, np.float64).tolist()):
        d[float(i)] = val if (not np.isnan(val) and val >= 0.2) else np.inf
    return d


# ----------------------------------------------------------------------------------------------------------------------
# the device balancing
# ----------------------------------------------------------------------------------------------------------------------
class _State(ctypes.Structure):            # mst_balance_state
    _fields_ = [("variance", ctypes.c_double), ("mean", ctypes.c_double), ("iterations", ctypes.c_int32),
                ("converged", ctypes.c_int32), ("done", ctypes.c_int32), ("_pad", ctypes.c_int32)]


class _NewtonState(ctypes.Structure):      # mst_newton_state
    _fields_ = [(k, ctypes.c_double) for k in ("rho", "rho_prev", "rout", "rold", "eta", "innertol", "alpha", "gamma",
                                               "variance")] + \
               [(k, ctypes.c_int32) for k in ("phase", "k", "matvecs", "iterations", "capped_steps", "capped_upper",
                                              "isolated", "active", "cg_step", "capped", "converged", "done")]


def _as_tensor(a, dtype, device):
    import torch
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=dtype)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a))).to(device=device, dtype=dtype)


class BalanceCSR:
    """The kept pixels of one map as the full symmetric CSR the kernels take (see include/mustache_hip.h)."""

    def __init__(self, x, y, v, n, ignore_diags=2, device=None):
        import torch
        from ._lib import require_gpu
        require_gpu()
        if device is None:
            device = v.device if isinstance(v, torch.Tensor) and v.is_cuda else \
                torch.device("cuda", torch.cuda.current_device())
        self.device, self.n = torch.device(device), int(n)
        n = self.n
        with torch.cuda.device(self.device):
            xd, yd = _as_tensor(x, torch.int64, device), _as_tensor(y, torch.int64, device)
            vd = _as_tensor(v, torch.float64, device)
            ok = (vd > 0) & torch.isfinite(vd)
            lo, hi = torch.minimum(xd, yd), torch.maximum(xd, yd)
            ok &= (lo >= 0) & (hi < n)
            lo, hi, vd = lo[ok], hi[ok], vd[ok]
            # a repeated pixel counts once: the last entry in input order wins (stable sort, last of each run of equal keys)
            key = lo * n + hi
            key, order = torch.sort(key, stable=True)
            last = torch.ones_like(key, dtype=torch.bool)
            if key.numel() > 1:
                last[:-1] = key[1:] != key[:-1]
            sel = order[last]
            lo, hi, vd = lo[sel], hi[sel], vd[sel]        # sorted by (lo, hi)
            del key, order, last, sel, xd, yd, ok
            far = (hi - lo) >= int(ignore_diags)
            lo, hi, vd = lo[far], hi[far], vd[far]
            self.kept = int(vd.numel())
            off = hi != lo
            rows = torch.cat([lo, hi[off]])
            cols = torch.cat([hi, lo[off]])
            vals = torch.cat([vd, vd[off]])
            del lo, hi, vd, off
            _, order = torch.sort(rows * n + cols)        # unique keys
            self.col = cols[order].to(torch.int32)
            self.val = vals[order]
            counts = torch.bincount(rows, minlength=n)
            del rows, cols, vals, order
            zero = torch.zeros(1, dtype=torch.int64, device=device)
            self.row_ptr = torch.cat([zero, torch.cumsum(counts, 0)])
            nch = (counts + (CHUNK - 1)) // CHUNK
            self.chunk_ptr = torch.cat([zero, torch.cumsum(nch, 0)])
            self.n_chunks = int(self.chunk_ptr[-1].item())
            self.chunk_row = torch.repeat_interleave(torch.arange(n, dtype=torch.int32, device=device), nch)
            self.nnz = int(self.val.numel())
            from . import _lib
            lib = _lib.load()
            self.ws = torch.empty(int(lib.mst_balance_workspace_bytes(n, self.n_chunks)), dtype=torch.uint8, device=device)

    def _args(self):
        from ._lib import ptr as _ptr
        return (_ptr(self.row_ptr), _ptr(self.col), _ptr(self.val), _ptr(self.chunk_row), _ptr(self.chunk_ptr), self.n,
                self.n_chunks)

    def marginals(self, w, with_nnz=False):
        """(m = w * (A w), row non-zero counts or None) as device tensors."""
        import torch
        from . import _lib
        from ._lib import ptr as _ptr, stream as _stream
        lib = _lib.load()
        m = torch.empty(self.n, dtype=torch.float64, device=self.device)
        nnz = torch.empty(self.n, dtype=torch.int32, device=self.device) if with_nnz else None
        _lib.check(lib.mst_balance_marginals(*self._args(), _ptr(w), _ptr(m), _ptr(nnz), _ptr(self.ws), self.ws.numel(),
                                             _stream()))
        return m, nnz

    def iterate(self, w, max_iter, tol):
        """Run the ICE iteration on w (in place) -> (iterations, variance, converged)."""
        import torch
        from . import _lib
        from ._lib import ptr as _ptr, stream as _stream
        lib = _lib.load()
        state = torch.zeros(ctypes.sizeof(_State), dtype=torch.uint8, device=self.device)
        launched = 0
        st = _State()
        while launched < max_iter:
            k = min(STEPS_PER_READ, max_iter - launched)
            _lib.check(lib.mst_balance_iterate(*self._args(), _ptr(w), int(k), int(max_iter), float(tol), _ptr(state),
                                               _ptr(self.ws), self.ws.numel(), _stream()))
            launched += k
            host = state.cpu().numpy()
            ctypes.memmove(ctypes.addressof(st), host.ctypes.data, ctypes.sizeof(_State))
            if st.done:
                break
        return int(st.iterations), float(st.variance), bool(st.converged)

    def newton(self, w, max_matvecs, tol):
        """Run the Newton iteration on w (in place: 1 / 0 in, x out) -> the final state record and the trace (a list)."""
        import torch
        from . import _lib
        from ._lib import ptr as _ptr, stream as _stream
        lib = _lib.load()
        need = int(lib.mst_balance_newton_workspace_bytes(self.n, self.n_chunks))
        if self.ws.numel() < need:
            self.ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        state = torch.zeros(ctypes.sizeof(_NewtonState), dtype=torch.uint8, device=self.device)
        cap = int(max_matvecs) + 2                  # one outer update costs a mat-vec; the count may pass the limit by one
        trace = torch.zeros(cap, dtype=torch.float64, device=self.device)
        st = _NewtonState()
        launched = 0
        while launched < cap + 1:                   # the start step and at most max_matvecs + 1 counted ones
            _lib.check(lib.mst_balance_newton(*self._args(), _ptr(w), int(STEPS_PER_READ), int(max_matvecs), float(tol),
                                              _ptr(state), _ptr(trace), cap, _ptr(self.ws), self.ws.numel(), _stream()))
            launched += STEPS_PER_READ
            host = state.cpu().numpy()
            ctypes.memmove(ctypes.addressof(st), host.ctypes.data, ctypes.sizeof(_NewtonState))
            if st.done:
                break
        if not st.done:
            raise RuntimeError("balance.newton: the device did not stop within %d steps" % launched)
        return st, trace[:st.iterations].cpu().numpy().tolist()

    def bias(self, w):
        """(bias device tensor [n], kappa)"""
        import torch
        from . import _lib
        from ._lib import ptr as _ptr, stream as _stream
        lib = _lib.load()
        b = torch.empty(self.n, dtype=torch.float64, device=self.device)
        kappa = torch.empty(1, dtype=torch.float64, device=self.device)
        _lib.check(lib.mst_balance_bias(*self._args(), _ptr(w), _ptr(b), _ptr(kappa), _ptr(self.ws), self.ws.numel(),
                                        _stream()))
        return b, float(kappa.item())


def mad_mask(m, mad_max):
    """Step 4 on host values m (float64 [n]): True where the bin is masked."""
    m = np.asarray(m, np.float64)
    pos = m > 0
    if not pos.any():
        return np.ones(len(m), bool)
    logm = np.log(m[pos])
    med = np.median(logm)
    mad = np.median(np.abs(logm - med))
    return (m < np.exp(med - mad_max * mad)) | (m == 0)


def _balance(step5, empty, x, y, v, n, ignore_diags, min_nnz, mad_max, device, timings):
    """Steps 1-4, then step5(csr, w) -> info entries (w: 1 / 0 in, the weights out), then step 6.  `empty`: the entries of an
    all-masked map."""
    import time
    import torch
    n = int(n)
    t0 = time.perf_counter()
    csr = BalanceCSR(x, y, v, n, ignore_diags=ignore_diags, device=device)
    with torch.cuda.device(csr.device):
        w = torch.ones(n, dtype=torch.float64, device=csr.device)
        _, nnz = csr.marginals(w, with_nnz=True)
        w = (nnz >= int(min_nnz)).to(torch.float64)
        m, _ = csr.marginals(w)
        masked = mad_mask(m.cpu().numpy(), float(mad_max))
        w = torch.from_numpy((~masked).astype(np.float64)).to(csr.device)
        torch.cuda.synchronize(csr.device)
        t1 = time.perf_counter()
        if masked.all():
            info, kappa = dict(empty), math.nan
            bias = np.full(n, np.nan)
        else:
            info = step5(csr, w)
            b, kappa = csr.bias(w)
            bias = b.cpu().numpy()
        t2 = time.perf_counter()
    if timings is not None:
        timings["prepare_s"], timings["iterate_s"], timings["kept"], timings["nnz"] = t1 - t0, t2 - t1, csr.kept, csr.nnz
    del csr
    info.update(masked=masked, kappa=kappa)
    return bias, info


def ice(x, y, v, n, *, ignore_diags=2, min_nnz=10, mad_max=5.0, tol=1e-5, max_iter=200, device=None, timings=None):
    """ICE bias of one chromosome's map.  x, y: bin indices (host arrays or device tensors, either orientation); v: raw
    counts; n: bin count.  Returns (bias float64[n] on the host, info) with info = {"iterations", "variance", "converged",
    "masked" (bool[n]), "kappa"}.  `timings` (a dict) receives "prepare_s" and "iterate_s" when given."""
    if int(max_iter) < 1:
        raise ValueError("ice(): max_iter must be >= 1")

    def step5(csr, w):
        iterations, variance, converged = csr.iterate(w, int(max_iter), float(tol))
        return {"iterations": iterations, "variance": variance, "converged": converged}
    return _balance(step5, {"iterations": 0, "variance": math.nan, "converged": True}, x, y, v, n, ignore_diags, min_nnz,
                    mad_max, device, timings)


_NEWTON_EMPTY = {"iterations": 0, "variance": math.nan, "converged": True, "matvecs": 0, "residual": math.nan,
                 "capped_steps": 0, "capped_upper": 0, "isolated": 0, "trace": []}


def newton(x, y, v, n, *, ignore_diags=2, min_nnz=10, mad_max=5.0, tol=1e-6, max_matvecs=2000, device=None, timings=None):
    """Newton (Knight & Ruiz) bias of one chromosome's map; arguments and result as ice().  info has ice()'s keys
    ("iterations": outer iterations, "variance": of x * (A x) over the active bins) and "matvecs", "residual" (the 2-norm of
    1 - x * (A x)), "capped_steps" ("capped_upper" of them at the upper cap), "isolated" (unmasked bins whose partners are all
    masked) and "trace" (the residual after every outer iteration)."""
    if int(max_matvecs) < 0 or not float(tol) > 0:
        raise ValueError("newton(): max_matvecs must be >= 0 and tol > 0")

    def step5(csr, w):
        st, trace = csr.newton(w, int(max_matvecs), float(tol))
        return {"iterations": int(st.iterations), "variance": float(st.variance), "converged": bool(st.converged),
                "matvecs": int(st.matvecs), "residual": math.sqrt(st.rout), "capped_steps": int(st.capped_steps),
                "capped_upper": int(st.capped_upper), "isolated": int(st.isolated), "trace": trace}
    empty = dict(_NEWTON_EMPTY, trace=[])
    return _balance(step5, empty, x, y, v, n, ignore_diags, min_nnz, mad_max, device, timings)


def solve(method, x, y, v, n, **kw):
    """ice() or newton(), by the method name check_request returned; info["method"] names it."""
    m = str(method).upper()
    if m not in METHODS:
        raise BalanceError("--balance %s: unknown method (supported: %s)" % (method, ", ".join(METHODS)))
    bias, info = (newton if m == "NEWTON" else ice)(x, y, v, n, **kw)
    info["method"] = m
    return bias, info


def _empty_info(method):
    """info of a map without a bin"""
    info = dict(_NEWTON_EMPTY, trace=[]) if method == "NEWTON" else {"iterations": 0, "variance": math.nan, "converged": True}
    info.update(masked=np.zeros(0, bool), kappa=math.nan, method=method)
    return info


def report(info, label):
    """The CLI's line about one balancing; a warning when the iteration limit was reached."""
    masked = (int(info["masked"].sum()), len(info["masked"]))
    if "matvecs" in info:
        if not info["converged"]:
            print("Warning: NEWTON balancing of %s did not converge in %d mat-vecs (%d outer iterations, residual %r)"
                  % (label, info["matvecs"], info["iterations"], info["residual"]))
        else:
            print("NEWTON balancing of %s: %d outer iterations, %d mat-vecs, %d of %d bins masked"
                  % ((label, info["iterations"], info["matvecs"]) + masked))
    elif not info["converged"]:
        print("Warning: ICE balancing of %s did not converge in %d iterations (variance %r)"
              % (label, info["iterations"], info["variance"]))
    else:
        print("ICE balancing of %s: %d iterations, %d of %d bins masked" % ((label, info["iterations"]) + masked))


# ----------------------------------------------------------------------------------------------------------------------
# readers under --balance
# ----------------------------------------------------------------------------------------------------------------------
def balance_text(p1, p2, cnt, res, method="ICE", **kw):
    """Raw text records (positions in bp, counts) -> (bias, info) over bins 0 .. max bin, by `method` (solve())."""
    a = np.floor_divide(np.asarray(p1, np.float64), res)
    b = np.floor_divide(np.asarray(p2, np.float64), res)
    cnt = np.asarray(cnt, np.float64)
    ok = np.isfinite(a) & np.isfinite(b) & (a >= 0) & (b >= 0)
    a, b, cnt = a[ok].astype(np.int64), b[ok].astype(np.int64), cnt[ok]
    n = int(max(a.max(), b.max())) + 1 if len(a) else 0
    if n == 0:
        return np.zeros(0), _empty_info(str(method).upper())
    return solve(method, a, b, cnt, n, **kw)


def read_hic_balanced(f, CHRM_SIZE, distance_in_bp, chromosome, res, device=None, method="ICE", **kw):
    """`.hic` under --balance: every raw record of the chromosome (norm NONE, no distance limit), `method` on the device, the
    bias applied on the device, then the reader's distance rule -> (x, y, v) host arrays, None when nothing is left."""
    raw = read_hic_raw(f, CHRM_SIZE, chromosome, res, device=device, method=method)
    if raw is None:
        return None
    xd, dd, vd, dev = raw
    return balance_records_device(xd, dd, vd, distance_in_bp, chromosome, res, dev, method=method, **kw)


def read_hic_raw(f, CHRM_SIZE, chromosome, res, device=None, method="ICE"):
    """The first half of read_hic_balanced, the raw pixel set on the device: -> (x int32, dist int32, v float32, device), None
    when the chromosome has no record."""
    import torch
    from ._lib import require_gpu
    from .hicfile import read_intra_packed
    from .readers import _HIC_LOCK, _hic_handle
    require_gpu()
    with _HIC_LOCK:
        h = _hic_handle(f)
        if not CHRM_SIZE:
            sizes = {"chr" + name.replace("chr", ''): length for name, length in h.chromosomes()[1:]}
            key = "chr" + str(chromosome).replace("chr", '')
            if key not in sizes:
                raise NameError('wrong chromosome name!')
            CHRM_SIZE = sizes[key]
        print("reading %s through the native .hic reader, raw counts for %s balancing" % (str(f).rsplit("/", 1)[-1], str(method).upper()))
        pc = read_intra_packed(h, chromosome, res, "NONE", -1, int(CHRM_SIZE))
    if len(pc) == 0:
        print(f'There is no contact in chrmosome {chromosome} to work on.')
        return None
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(dev):
        xd = torch.from_numpy(pc.x[:pc.count]).to(dev)
        dd = torch.from_numpy(pc.dist[:pc.count]).to(dev)
        vd = torch.from_numpy(pc.v[:pc.count]).to(dev)
    return xd, dd, vd, dev


def balance_records_device(xd, dd, vd, distance_in_bp, chromosome, res, dev, method="ICE", **kw):
    """The half of a --balance read that follows the pixel set, shared by `.hic` input (read_hic_balanced) and read pairs
    (pairs.read_pairs_balanced): device records (xd = bin, dd = distance: int32; vd = raw counts, float32 as a `.hic` file
    stores them or float64) -> n = max bin + 1, `method` on the device, the bias applied on the device as
    v' = (v / b[x]) / b[y] (NaN or < 0.2 count as +inf), then v' > 0 and the reader's distance rule -> (x, y, v) host arrays,
    None when nothing is left."""
    return balance_records_with_bias(xd, dd, vd, distance_in_bp, chromosome, res, dev, method=method, **kw)[0]


def balance_records_with_bias(xd, dd, vd, distance_in_bp, chromosome, res, dev, method="ICE", **kw):
    """balance_records_device for a caller that goes on with the bias (pileup.py, "Significance"): -> (that function's result,
    the bias vector solve() returned as a device float64 [n] tensor)."""
    import torch
    from ._lib import ptr as _ptr, stream as _stream, require_gpu
    from . import _lib
    lib = require_gpu()
    count = int(vd.numel())
    with torch.cuda.device(dev):
        yd = xd.to(torch.int64) + dd.to(torch.int64)
        n = int(yd.max().item()) + 1
        bias, info = solve(method, xd, yd, vd.to(torch.float64), n, device=dev, **kw)
        report(info, "chromosome %s" % chromosome)
        bd = torch.from_numpy(bias).to(dev)
        out = torch.empty(count, dtype=torch.float64, device=dev)
        if vd.dtype == torch.float32:
            _lib.check(lib.mst_balance_apply_packed(_ptr(xd), _ptr(dd), _ptr(vd), count, _ptr(bd), int(n), _ptr(out), _stream()))
        else:                                   # float64 counts: the pair form with one segment that starts at bin 0
            seg = torch.tensor([0, count], dtype=torch.int64, device=dev)
            zero = torch.zeros(1, dtype=torch.int64, device=dev)
            y32 = yd.to(torch.int32)
            _lib.check(lib.mst_balance_apply_pairs(_ptr(xd), _ptr(y32), _ptr(vd), count, _ptr(seg), _ptr(zero), _ptr(zero), 1,
                                                   _ptr(bd), int(n), _ptr(out), _stream()))
        keep = (out > 0) & (dd <= int(distance_in_bp // res))
        x, y, v = xd[keep].to(torch.int64).cpu().numpy(), yd[keep].cpu().numpy(), out[keep].cpu().numpy()
    if len(v) == 0:
        print(f'There is no contact in chrmosome {chromosome} to work on.')
        return None, bd
    return (x, y, v), bd
