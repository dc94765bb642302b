"""NumPy restatement of the Newton balancing of mustache_amd/balance.py (`--balance NEWTON`): Knight & Ruiz's inexact Newton
iteration with Jacobi-preconditioned conjugate gradients on x_i (A x)_i = 1.  Steps 1-4 (kept pixels, min_nnz, MAD mask) and
step 6 (kappa, b = kappa / w, NaN on masked bins) are those of the ICE restatement (tests/balance_reference.py) and are taken
from it; step 5 is restated here.  Plain float64 NumPy; no GPU.

K: the unmasked bins.  Act = {i in K : (A 1_K)_i != 0}; the bins of K outside Act ("isolated") keep x = 1 and take part in
nothing.  Every vector lives on Act, A is the kept symmetric matrix restricted to K.

    x = 1; v = x * (A x); r = 1 - v; rho = rout = r.r; eta = etamax; rold = rout
    while rout > tol^2 and matvecs < max_matvecs:
        y = 1; k = 0; innertol = max(eta^2 * rout, tol^2)
        while rho > innertol and matvecs < max_matvecs:
            k += 1
            if k == 1: z = r / v; p = z; rho = r.z
            else:      p = z + (rho / rho_prev) * p
            w = x * (A (x * p)) + v * p; matvecs += 1
            if not (p.w > 0 and finite): stop, converged = False
            alpha = rho / (p.w); ap = alpha * p; ynew = y + ap
            if min(ynew) <= delta: y += min over {ap_i < 0} of (delta - y_i) / ap_i * ap; capped step, leave the inner loop
            if max(ynew) >= Delta: y += min over {ynew_i > Delta} of (Delta - y_i) / ap_i * ap; capped step, leave
            y = ynew; r -= alpha * w; rho_prev = rho; z = r / v; rho = r.z
        x = x * y; v = x * (A x); matvecs += 1; r = 1 - v; rho = rout = r.r
        rat = rout / rold; rold = rout; eta_o = eta; eta = g * rat
        if g * eta_o^2 > 0.1: eta = max(eta, g * eta_o^2)
        eta = max(min(eta, etamax), 0.5 * tol / sqrt(rout))
    converged = rout <= tol^2

(The upper-cap set {ynew_i > Delta} is empty only when max(ynew) == Delta exactly; the factor is then 1.)
"""
import numpy as np

import balance_reference as br

DELTA_LO, DELTA_HI, G, ETAMAX = 0.1, 3.0, 0.9, 0.1


def solve(rows, cols, vals, w0, n, tol=1e-6, max_matvecs=2000):
    """Step 5 on the symmetric entries; w0: 1 on unmasked bins, 0 on masked.  -> (w [n], stats) with w = x on Act, 1 on
    isolated bins, 0 on masked bins."""
    w0 = np.asarray(w0, np.float64)

    def A(u):
        return np.bincount(rows, weights=vals * u[cols], minlength=n)

    a1 = A(w0)
    act = (w0 != 0) & (a1 != 0)
    isolated = int(((w0 != 0) & ~act).sum())
    x = act.astype(np.float64)                       # vectors are kept at length n, zero outside Act
    v = x * A(x)
    r = np.where(act, 1.0 - v, 0.0)
    rho = rout = float(r @ r)
    eta, rold = ETAMAX, rout
    matvecs = outer = capped = capped_upper = 0
    trace, failed = [], False
    tol2 = tol * tol
    va = np.where(act, v, 1.0)                       # divisor: 1 outside Act, where r and p are 0
    while rout > tol2 and matvecs < max_matvecs and not failed:
        y = np.ones(n)
        k = 0
        innertol = max(eta * eta * rout, tol2)
        rho_prev, p = np.nan, None
        while rho > innertol and matvecs < max_matvecs:
            k += 1
            if k == 1:
                z = r / va
                p = z.copy()
                rho = float(r @ z)
            else:
                p = z + (rho / rho_prev) * p
            w = x * A(x * p) + v * p
            matvecs += 1
            pw = float(p @ w)
            if not (pw > 0 and np.isfinite(pw)):
                failed = True
                break
            alpha = rho / pw
            ap = alpha * p
            ynew = y + ap
            if ynew[act].min() <= DELTA_LO:
                neg = act & (ap < 0)
                y = y + np.min((DELTA_LO - y[neg]) / ap[neg]) * ap
                capped += 1
                break
            if ynew[act].max() >= DELTA_HI:
                big = act & (ynew > DELTA_HI)
                gamma = np.min((DELTA_HI - y[big]) / ap[big]) if big.any() else 1.0
                y = y + gamma * ap
                capped += 1
                capped_upper += 1
                break
            y = ynew
            r = r - alpha * w
            rho_prev = rho
            z = r / va
            rho = float(r @ z)
        if failed:
            break
        x = x * y
        v = x * A(x)
        matvecs += 1
        va = np.where(act, v, 1.0)
        r = np.where(act, 1.0 - v, 0.0)
        rho = rout = float(r @ r)
        outer += 1
        trace.append(np.sqrt(rout))
        rat = rout / rold
        rold = rout
        eta_o = eta
        eta = G * rat
        if G * eta_o * eta_o > 0.1:
            eta = max(eta, G * eta_o * eta_o)
        eta = max(min(eta, ETAMAX), 0.5 * tol / np.sqrt(rout)) if rout > 0 else ETAMAX
    wout = np.where(act, x, w0)
    stats = {"iterations": outer, "matvecs": matvecs, "residual": float(np.sqrt(rout)), "capped_steps": capped,
             "capped_upper": capped_upper, "isolated": isolated, "trace": trace, "converged": bool(rout <= tol2) and not failed,
             "variance": float(np.var(v[act])) if act.any() else 0.0, "active": act}
    return wout, stats


def newton(x, y, v, n, ignore_diags=2, min_nnz=10, mad_max=5.0, tol=1e-6, max_matvecs=2000):
    """-> (bias [n], info) like mustache_amd.balance.newton; info also carries "active" (bool [n])."""
    i, j, vv = br.kept_pixels(x, y, v, n, ignore_diags)
    masked = br.filter_mask(i, j, vv, n, min_nnz, mad_max)
    info = {"masked": masked}
    if masked.all():
        info.update(iterations=0, variance=np.nan, converged=True, kappa=np.nan, matvecs=0, residual=np.nan, capped_steps=0,
                    capped_upper=0, isolated=0, trace=[], active=np.zeros(n, bool))
        return np.full(n, np.nan), info
    rows, cols, vals = br._sym(i, j, vv)
    w, stats = solve(rows, cols, vals, (~masked).astype(np.float64), n, tol, max_matvecs)
    kappa = np.sqrt(np.sum(vv * w[i] * w[j]) / np.sum(vv))
    bias = np.full(n, np.nan)
    bias[~masked] = kappa / w[~masked]
    info.update(stats, kappa=kappa)
    return bias, info


def condition(x, y, v, n, bias, info, ignore_diags=2):
    """From a result alone: (1 - x * (A x) on Act with x = kappa / bias, kappa recomputed from its definition)."""
    i, j, vv = br.kept_pixels(x, y, v, n, ignore_diags)
    rows, cols, vals = br._sym(i, j, vv)
    w = np.where(info["masked"], 0.0, info["kappa"] / np.where(info["masked"], 1.0, bias))
    av = np.bincount(rows, weights=vals * w[cols], minlength=n)
    act = ~info["masked"] & (np.bincount(rows, weights=vals * (~info["masked"])[cols], minlength=n) != 0)
    kappa = np.sqrt(np.sum(vv * w[i] * w[j]) / np.sum(vv))
    return (1.0 - w * av)[act], kappa, act


def isolated_map():
    """A circular band of 60 bins (every bin has the same number of partners), then bin 60 whose only partners are the five
    bins 61 .. 65, which have no other partner: their row sums (6) fall below the MAD cut-off and bin 60's (30) does not.
    -> (x, y, v, n)"""
    rng = np.random.default_rng(11)
    xs, ys = [], []
    for i in range(60):
        for d in range(6):
            xs.append(min(i, (i + d) % 60))
            ys.append(max(i, (i + d) % 60))
    v = rng.uniform(2.0, 4.0, len(xs))
    x = np.concatenate([np.array(xs), np.full(5, 60)])
    y = np.concatenate([np.array(ys), np.arange(61, 66)])
    return x, y, np.concatenate([v, np.full(5, 6.0)]), 66
