"""What the Chebyshev tests share: the estimate's start vector, the Lanczos recurrence, the tridiagonal and its largest
eigenvalue by Sturm bisection, the row bound, the coefficient table and the polynomial, restated in Python floats and numpy
(one IEEE operation each) with the row sums in lane order (amg_numerics) and the dots in the pinned order
(krylov_numerics).  No GPU and no library call in here."""
import math
import sys

import numpy as np

import amg_numerics as AN
import krylov_numerics as KN

DBL_MIN = sys.float_info.min
STEPS, BOOST, RATIO, DEGREE, BISECTIONS = 10, 1.1, 30.0, 4, 64             # the header's defaults, restated on purpose

# the nine non-empty cases of amg_numerics and the indefinite 2 x 2 matrix that stops the recurrence at once
INDEFINITE = dict(name="indefinite2", n=2, rp=np.array([0, 2, 4], np.int32), ci=np.array([0, 1, 0, 1], np.int32),
                  val=np.array([1.0, 2.0, 2.0, 1.0]), symmetric=True, theta=0.0)


def case(name):
    return INDEFINITE if name == "indefinite2" else AN.case(name)


CASES = AN.CASES + ["indefinite2"]


def positive(v):
    return v > 0.0 and math.isfinite(v)


def start(n, seed=0, level=0):
    """b0[i] = (2 h(i) + 1) 2^-32 - 1: exact in a double"""
    return np.array([(2.0 * AN.priority(i, seed, level) + 1.0) * 2.0 ** -32 - 1.0 for i in range(n)], np.float64)


def diagonal(n, rp, ci, val):
    d = np.zeros(n)
    for i in range(n):
        d[i] = val[rp[i]:rp[i + 1]][ci[rp[i]:rp[i + 1]] == i][0]
    return d


def level_of(n, rp, ci, val):
    return dict(n=n, rowptr=rp, colidx=ci, val=val)


def lanczos(n, rp, ci, val, steps=STEPS, seed=0, level=0):
    """-> (alpha, beta, m): k steps of Jacobi-preconditioned CG on A x = b0 from x = 0, x never formed"""
    L = level_of(n, rp, ci, val)
    with np.errstate(all="ignore"):
        dinv = 1.0 / diagonal(n, rp, ci, val)
        r = start(n, seed, level)
        z = dinv * r
        p = z.copy()
        rho = float(KN.dot_np(r, z))
        alpha, beta, m = [], [], 0
        for j in range(steps):
            q = AN.row_sums(L, p)
            pq = float(KN.dot_np(p, q))
            if not positive(pq):
                break
            a = rho / pq
            if not positive(a):
                break
            alpha.append(a)
            m = j + 1
            if j == steps - 1:
                break
            r = r - np.float64(a) * q
            z = dinv * r
            rho_new = float(KN.dot_np(r, z))
            b = rho_new / rho if rho != 0.0 else math.nan
            if not positive(b):
                break
            beta.append(b)
            rho = rho_new
            p = z + np.float64(b) * p
    return alpha, beta[:max(m - 1, 0)], m


def tridiagonal(alpha, beta):
    m = len(alpha)
    t, e2 = [], []
    for j in range(m):
        inv = 1.0 / alpha[j]
        t.append(inv if j == 0 else inv + beta[j - 1] / alpha[j - 1])
        if j < m - 1:
            e2.append(beta[j] / (alpha[j] * alpha[j]))
    return t, e2


def sturm_count(t, e2, x):
    count, q = 0, 0.0
    for j in range(len(t)):
        q = t[j] - x if j == 0 else (t[j] - x) - e2[j - 1] / q
        if q == 0.0:
            q = -DBL_MIN
        if q < 0.0:
            count += 1
    return count


def ritz(t, e2):
    m = len(t)
    lo = max(t)
    hi = max((t[j] + (math.sqrt(e2[j - 1]) if j > 0 else 0.0)) + (math.sqrt(e2[j]) if j < m - 1 else 0.0) for j in range(m))
    for _ in range(BISECTIONS):
        mid = lo + (hi - lo) / 2.0
        if mid <= lo or mid >= hi:
            break
        if sturm_count(t, e2, mid) == m:
            hi = mid
        else:
            lo = mid
    return hi


def rowbound(n, rp, ci, val):
    g = 0.0
    d = diagonal(n, rp, ci, val)
    with np.errstate(all="ignore"):
        for i in range(n):
            s = 0.0
            for a in val[rp[i]:rp[i + 1]]:
                s = s + abs(float(a))
            bound = float(np.float64(s) / np.float64(d[i]))
            if bound > g:
                g = bound
    return g


def lambda_max(m, ritz_value, g, boost=BOOST):
    if m < 1:
        return g
    boosted = boost * ritz_value
    return boosted if boosted < g else g


def coefficients(lmax, degree=DEGREE, ratio=RATIO):
    """-> (table of degree rows (c1_k, c2_k), lambda_min)"""
    with np.errstate(all="ignore"):
        lmax = np.float64(lmax)
        lmin = lmax / np.float64(ratio)
        theta, delta = (lmax + lmin) / np.float64(2.0), (lmax - lmin) / np.float64(2.0)
        sigma = theta / delta
        rho = np.float64(1.0) / sigma
        table = [(0.0, float(np.float64(1.0) / theta))]
        for _ in range(1, degree):
            nxt = np.float64(1.0) / (np.float64(2.0) * sigma - rho)
            table.append((float(nxt * rho), float((np.float64(2.0) * nxt) / delta)))
            rho = nxt
    return np.array(table, np.float64).reshape(degree, 2), float(lmin)


def estimate(c, steps=STEPS, boost=BOOST, seed=0, level=0):
    """the whole estimate of case c -> dict(alpha, beta, m, t, e2, ritz, g, lambda_max)"""
    n, rp, ci, val = c["n"], c["rp"], c["ci"], c["val"]
    alpha, beta, m = lanczos(n, rp, ci, val, steps, seed, level)
    t, e2 = tridiagonal(alpha, beta)
    rv = ritz(t, e2) if m else 0.0
    g = rowbound(n, rp, ci, val)
    return dict(alpha=alpha, beta=beta, m=m, t=t, e2=e2, ritz=rv, g=g, lambda_max=lambda_max(m, rv, g, boost))


def apply(n, rp, ci, val, table, b, x=None):
    """the polynomial of degree len(table) from zero, or from the guess x: numpy rounds every elementwise operation"""
    L = level_of(n, rp, ci, val)
    with np.errstate(all="ignore"):
        dinv = 1.0 / diagonal(n, rp, ci, val)
        b = np.asarray(b, np.float64)
        c2 = np.float64(table[0][1])
        if x is None:
            d = c2 * (dinv * b)
            cur = d.copy()
        else:
            x = np.asarray(x, np.float64)
            d = c2 * (dinv * (b - AN.row_sums(L, x)))
            cur = x + d
        for k in range(1, len(table)):
            t = dinv * (b - AN.row_sums(L, cur))
            d = np.float64(table[k][0]) * d + np.float64(table[k][1]) * t
            cur = cur + d
    return cur


def true_lambda_max(n, rp, ci, val):
    """the largest eigenvalue of D^-1/2 A D^-1/2, dense: small symmetric cases only"""
    A = np.zeros((n, n))
    row = np.repeat(np.arange(n), np.diff(rp.astype(np.int64)))
    A[row, ci] = val
    d = np.diag(A)
    return float(np.linalg.eigvalsh(A / np.sqrt(np.outer(d, d)))[-1])        # a_ii / sqrt(a_ii a_ii) is 1 exactly


# ---- the polynomial as AMG's smoother -----------------------------------------------------------------------------------
def chebyshev_levels(levels, degree=2, coarse_sweeps=8, steps=STEPS, boost=BOOST, ratio=RATIO, seed=0, estimate_of=estimate):
    """A hierarchy (amg_numerics' or amg_sa_numerics') as the Chebyshev smoother sees it: wd = 1 / a_ii and table, the level's
    own, from the level's own estimate of salt seed + level; the coarsest level's table has coarse_sweeps rows.
    estimate_of(case, steps, boost, seed, level) -> dict with lambda_max (the restatement's by default)."""
    out = []
    for l, L in enumerate(levels):
        c = dict(n=L["n"], rp=L["rowptr"], ci=L["colidx"], val=L["val"])
        E = estimate_of(c, steps, boost, seed, l)
        table, _ = coefficients(E["lambda_max"], coarse_sweeps if l + 1 == len(levels) else degree, ratio)
        with np.errstate(all="ignore"):
            wd = 1.0 / diagonal(L["n"], L["rowptr"], L["colidx"], L["val"])
        out.append(dict(L, wd=wd, table=table, eig=E))
    return out


def cycle_py(levels, r, nu=1, degree=2, coarse_sweeps=8, scale=1.0, l=0):
    """z = M^-1 r with every smoothing one polynomial: the pre-smoothing's first from zero, the others from the iterate; the
    coarsest level one polynomial of degree coarse_sweeps from zero.  Plain aggregates or general P and R, by the level's keys."""
    L = levels[l]
    b = np.asarray(r, np.float64)
    poly = lambda x: apply(L["n"], L["rowptr"], L["colidx"], L["val"], L["table"], b, x)
    if l + 1 == len(levels):
        return poly(None)
    x = poly(None)
    for _ in range(nu - 1):
        x = poly(x)
    res = b - AN.row_sums(L, x)
    if "p_rowptr" in L:
        bc = AN.row_sums(dict(n=len(L["r_rowptr"]) - 1, rowptr=L["r_rowptr"], colidx=L["r_colidx"], val=L["r_val"]), res)
    else:
        nc = len(L["aggptr"]) - 1
        bc = np.zeros(nc)
        for a in range(nc):
            s = 0.0
            for k in range(int(L["aggptr"][a]), int(L["aggptr"][a + 1])):
                s = s + float(res[L["members"][k]])
            bc[a] = s
    e = cycle_py(levels, bc, nu, degree, coarse_sweeps, scale, l + 1)
    if "p_rowptr" in L:
        x = x + np.float64(scale) * AN.row_sums(dict(n=L["n"], rowptr=L["p_rowptr"], colidx=L["p_colidx"], val=L["p_val"]), e)
    else:
        x = x + np.float64(scale) * e[L["agg"]]
    for _ in range(nu):
        x = poly(x)
    return x


def launches(levels, nu=1, degree=2, coarse_sweeps=8):
    """a hand count: 2 nu polynomials of `degree` launches, a residual, a restriction and a prolongation on every level
    above the coarsest, one polynomial of coarse_sweeps launches on it"""
    return 0 if levels == 0 else (levels - 1) * (2 * nu * degree + 3) + coarse_sweeps
