"""What the AMG tests share: the cases, the aggregation restated as a scalar loop, the hierarchy built in numpy from a set
of aggregates, the V-cycle restated with the row sums in lane order, and the plain host loops "it solves" is held
against (the loops composed from parts are in solver_compose.py).  No GPU and no library call in here (fma is the C
library's, by ctypes: Python's math.fma where it exists)."""
import ctypes
import ctypes.util
import math
from fractions import Fraction

import numpy as np

import krylov_numerics as KN

G4_MAX, G16_MAX = 4, 32                                                     # the header's group bounds, restated on purpose
MASK = 0xffffffff

if hasattr(math, "fma"):
    fma = math.fma
else:
    try:
        _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm.fma.restype = ctypes.c_double
        _libm.fma.argtypes = [ctypes.c_double] * 3
        fma = _libm.fma
    except (OSError, AttributeError):
        def fma(a, b, c):                                                   # exact: rationals, rounded once
            return float(Fraction(a) * Fraction(b) + Fraction(c))


# ---- the cases ----------------------------------------------------------------------------------------------------------
def csr_from_rows(rows):
    """rows: a list of dicts {col: val} -> (n, rowptr, colidx, val) with ascending columns"""
    rp, ci, val = [0], [], []
    for r in rows:
        for c in sorted(r):
            ci.append(c), val.append(r[c])
        rp.append(len(ci))
    return len(rows), np.array(rp, np.int32), np.array(ci, np.int32), np.array(val, np.float64)


def grid_rows(side, ax=1.0, ay=1.0, base=0):
    rows = []
    for y in range(side):
        for x in range(side):
            r = {base + y * side + x: 2.0 * ax + 2.0 * ay}
            if x > 0:
                r[base + y * side + x - 1] = -ax
            if x + 1 < side:
                r[base + y * side + x + 1] = -ax
            if y > 0:
                r[base + (y - 1) * side + x] = -ay
            if y + 1 < side:
                r[base + (y + 1) * side + x] = -ay
            rows.append(r)
    return rows


def case(name):
    """-> dict(n, rp, ci, val, symmetric, theta)"""
    theta, sym = 0.0, True
    if name == "n0":
        n, rp, ci, val = 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0)
    elif name == "n1":
        n, rp, ci, val = csr_from_rows([{0: 2.0}])
    elif name == "diagonal300":
        n, rp, ci, val = csr_from_rows([{i: 1.0 + (i % 7)} for i in range(300)])
    elif name == "tridiagonal3000":
        n, rp, ci, val = csr_from_rows([{j: (2.0 if j == i else -1.0) for j in (i - 1, i, i + 1) if 0 <= j < 3000} for i in range(3000)])
    elif name in ("grid24", "grid32"):
        n, rp, ci, val = KN.laplacian(int(name[4:]))
        rp, ci = rp.astype(np.int32), ci.astype(np.int32)
    elif name == "clique130":                                               # a 130-clique block next to a 12 x 12 grid
        rows = [{j: (131.0 if j == i else -1.0) for j in range(130)} for i in range(130)] + grid_rows(12, base=130)
        n, rp, ci, val = csr_from_rows(rows)
    elif name == "star5000":
        rows = [{j: (5000.0 if j == 0 else -1.0) for j in range(5000)}] + [{0: -1.0, i: 2.0} for i in range(1, 5000)]
        n, rp, ci, val = csr_from_rows(rows)
    elif name == "random4000":
        rng = np.random.default_rng(4000)
        rows = []
        for i in range(4000):
            cols = set(int(c) for c in rng.integers(0, 4000, 7)) - {i}
            r = {c: float(-rng.random() - 0.1) for c in cols}
            r[i] = float(-sum(r.values()) + 1.0)
            rows.append(r)
        n, rp, ci, val = csr_from_rows(rows)
        sym = False
    elif name == "aniso32":                                                 # strong along x, weak (0.01) along y
        n, rp, ci, val = csr_from_rows(grid_rows(32, ax=1.0, ay=0.01))
        theta = 0.25
    else:
        raise KeyError(name)
    return dict(name=name, n=n, rp=rp, ci=ci, val=val, symmetric=sym, theta=theta)


CASES = ["n0", "n1", "diagonal300", "tridiagonal3000", "grid24", "grid32", "clique130", "star5000", "random4000", "aniso32"]


# ---- aggregation, as a scalar loop -------------------------------------------------------------------------------------
def fmix32(x):
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & MASK
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & MASK
    x ^= x >> 16
    return x


def priority(v, seed, level):
    salt = (0x9E3779B9 * ((seed + level + 1) & MASK)) & MASK
    return fmix32((v + salt) & MASK)


def strong_lists(n, rp, ci, val=None, theta=0.0):
    """every row's strong neighbours in stored order"""
    out = []
    for i in range(n):
        cols = [int(c) for c in ci[rp[i]:rp[i + 1]]]
        if val is not None and theta > 0.0:
            vals = [abs(float(v)) for v in val[rp[i]:rp[i + 1]]]
            m = 0.0
            for c, a in zip(cols, vals):
                if c != i and a > m:
                    m = a
            bound = theta * m
            out.append([c for c, a in zip(cols, vals) if c != i and a >= bound])
        else:
            out.append([c for c in cols if c != i])
    return out


def aggregate_py(n, rp, ci, val=None, theta=0.0, seed=0, level=0):
    """-> (agg, aggptr, members, roots)"""
    strong = strong_lists(n, rp, ci, val, theta)
    order = sorted(range(n), key=lambda v: -priority(v, seed, level))
    root = [False] * n
    for v in order:
        root[v] = not any(root[u] for u in strong[v])
    agg, count = [-1] * n, 0
    for v in range(n):
        if root[v]:
            agg[v], count = count, count + 1
    for v in range(n):
        if not root[v]:
            agg[v] = agg[next(u for u in strong[v] if root[u])]
    members = sorted(range(n), key=lambda v: (agg[v], v))
    aggptr = [0] * (count + 1)
    for v in range(n):
        aggptr[agg[v] + 1] += 1
    for a in range(count):
        aggptr[a + 1] += aggptr[a]
    return np.array(agg, np.int32), np.array(aggptr, np.int32), np.array(members, np.int32), np.array(root, bool)


# ---- the hierarchy, in numpy --------------------------------------------------------------------------------------------
def galerkin(n, rp, ci, agg, n_agg):
    """the coarse pattern of a set of aggregates: the triplets (agg[row], agg[col]) in stored order, sorted by (row, col),
    equal pairs in input order -> (rowptr, colidx, perm, runptr)"""
    row = np.repeat(np.arange(n), np.diff(rp.astype(np.int64)))
    tr, tc = agg[row].astype(np.int64), agg[ci].astype(np.int64)
    perm = np.lexsort((tc, tr))
    sr, sc = tr[perm], tc[perm]
    head = np.ones(len(perm), bool)
    head[1:] = (sr[1:] != sr[:-1]) | (sc[1:] != sc[:-1])
    runptr = np.concatenate([np.flatnonzero(head), [len(perm)]])
    crow, ccol = sr[head], sc[head]
    crp = np.concatenate([[0], np.cumsum(np.bincount(crow, minlength=n_agg))])
    return crp.astype(np.int32), ccol.astype(np.int32), perm, runptr


def assemble(val, perm, runptr):
    """a run's values added left to right in input order, each sum rounded"""
    v = np.asarray(val, np.float64)[perm]
    out = v[runptr[:-1]].copy()
    length = np.diff(runptr)
    for k in range(1, int(length.max()) if len(length) else 0):
        sel = length > k
        out[sel] = out[sel] + v[runptr[:-1][sel] + k]
    return out


def weights(n, rp, ci, val, smoother="jacobi", omega=None):
    if omega is None:
        omega = 1.0 if smoother == "l1" else 2.0 / 3.0
    wd = np.zeros(n)
    for i in range(n):
        c, v = ci[rp[i]:rp[i + 1]], val[rp[i]:rp[i + 1]]
        if smoother == "l1":
            s = 0.0
            for a in v:
                s = s + abs(float(a))
        else:
            s = float(v[c == i][0])
        wd[i] = np.float64(omega) / np.float64(s)
    return wd


def hierarchy(c, aggregate, coarse_max=64, max_levels=20, seed=0, smoother="jacobi", omega=None):
    """The levels of case c by the stopping rule, with `aggregate(n, rp, ci, val, theta, seed, level) -> (agg, aggptr,
    members)`: a list of dicts(n, rowptr, colidx, val, wd[, agg, aggptr, members, perm, runptr])."""
    n, rp, ci, val, theta = c["n"], c["rp"], c["ci"], c["val"], c["theta"]
    levels = []
    if n == 0:
        return levels
    while True:
        L = dict(n=n, rowptr=rp, colidx=ci, val=val, wd=weights(n, rp, ci, val, smoother, omega))
        levels.append(L)
        if not (n > coarse_max and len(levels) < max_levels):
            return levels
        agg, aggptr, members = aggregate(n, rp, ci, val if theta > 0.0 else None, theta, seed, len(levels) - 1)[:3]
        nc = len(aggptr) - 1
        if nc >= n:
            return levels
        crp, cci, perm, runptr = galerkin(n, rp, ci, agg, nc)
        L.update(agg=agg, aggptr=aggptr, members=members, perm=perm, runptr=runptr)
        n, rp, ci, val = nc, crp, cci, assemble(val, perm, runptr)


# ---- the cycle, with the row sums in lane order --------------------------------------------------------------------------
def group(p):
    return 4 if p <= G4_MAX else 16 if p <= G16_MAX else 64


def lane_order_sum(ci, val, x, beg, end, take=None):
    """the sum of one stored row (entries beg .. end - 1; ci, val, x plain lists): G comes from the stored length; lane l
    of G takes the entries l, l + G, ... with one fma each from +0, an entry whose take[e] is false takes none (take: a
    mask over the stored entries, None for the whole row); the butterfly l ^ 1, l ^ 2, ... as written; lane 0"""
    G = group(end - beg)
    v = [0.0] * G
    for l in range(min(G, end - beg)):
        s = 0.0
        for e in range(beg + l, end, G):
            if take is None or take[e]:
                s = fma(val[e], x[ci[e]], s)
        v[l] = s
    m = 1
    while m < G:
        v = [v[l] + v[l ^ m] for l in range(G)]
        m <<= 1
    return v[0]


def row_sums(L, x):
    """s_i for every row, each by lane_order_sum()"""
    rp, ci, val = L["rowptr"], L["colidx"].tolist(), L["val"].tolist()
    x = x.tolist()
    out = np.zeros(L["n"])
    for i in range(L["n"]):
        out[i] = lane_order_sum(ci, val, x, int(rp[i]), int(rp[i + 1]))
    return out


def cycle_py(levels, r, nu=1, coarse_sweeps=8, scale=1.0, l=0):
    """z = M^-1 r: numpy rounds every elementwise operation on its own"""
    L = levels[l]
    b = np.asarray(r, np.float64)
    x = L["wd"] * b
    if l + 1 == len(levels):
        for _ in range(coarse_sweeps - 1):
            x = x + L["wd"] * (b - row_sums(L, x))
        return x
    for _ in range(nu - 1):
        x = x + L["wd"] * (b - row_sums(L, x))
    res = b - row_sums(L, x)
    nc = len(L["aggptr"]) - 1
    bc = np.zeros(nc)
    members, aggptr = L["members"], L["aggptr"]
    for a in range(nc):
        s = 0.0
        for k in range(int(aggptr[a]), int(aggptr[a + 1])):
            s = s + float(res[members[k]])
        bc[a] = s
    e = cycle_py(levels, bc, nu, coarse_sweeps, scale, l + 1)
    x = x + np.float64(scale) * e[L["agg"]]
    for _ in range(nu):
        x = x + L["wd"] * (b - row_sums(L, x))
    return x


def launches(levels, nu=1, coarse_sweeps=8):
    """a hand count: 2 nu sweeps, a residual, a restriction and a prolongation on every level above the coarsest"""
    return 0 if levels == 0 else (levels - 1) * (2 * nu + 3) + coarse_sweeps


# ---- the host loops "it solves" is held against (the loops composed from parts live in solver_compose.py) ------------------
def host_pcg(n, rp, ci, val, b, apply, tol, limit=1000, x0=None):
    """plain float64 PCG with M^-1 = apply -> (iterations until |r| <= tol |b|, x); from x = 0, or from the guess x0, which
    is returned at once when it already meets the test"""
    x, r, stop = np.zeros(n), b.copy(), tol * np.linalg.norm(b)
    if x0 is not None:
        x, r = x0.copy(), b - KN.matvec(n, rp, ci, val, x0)
        if np.linalg.norm(r) <= stop:
            return 0, x
    z = apply(r)
    p, rz = z.copy(), r @ z
    for it in range(1, limit + 1):
        q = KN.matvec(n, rp, ci, val, p)
        alpha = rz / (p @ q)
        x, r = x + alpha * p, r - alpha * q
        if np.linalg.norm(r) <= stop:
            return it, x
        z = apply(r)
        rz, old = r @ z, rz
        p = z + (rz / old) * p
    return limit + 1, x


def host_bicgstab(n, rp, ci, val, b, apply, tol, limit=1000, x0=None):
    """plain float64 BiCGStab with M^-1 = apply, right-preconditioned -> (iterations until |r| <= tol |b|, x)"""
    x = np.zeros(n) if x0 is None else x0.copy()
    r = b - KN.matvec(n, rp, ci, val, x)
    stop = tol * np.linalg.norm(b)
    if np.linalg.norm(r) <= stop:
        return 0, x
    rh, p, v = r.copy(), np.zeros(n), np.zeros(n)
    rho, alpha, omega = r @ r, 1.0, 1.0
    beta = 0.0
    for it in range(1, limit + 1):
        p = r + beta * (p - omega * v)
        ph = apply(p)
        v = KN.matvec(n, rp, ci, val, ph)
        alpha = rho / (rh @ v)
        s = r - alpha * v
        sh = apply(s)
        t = KN.matvec(n, rp, ci, val, sh)
        tt = t @ t
        omega = (t @ s) / tt if tt != 0.0 else 0.0
        x, r = x + alpha * ph + omega * sh, s - omega * t
        if np.linalg.norm(r) <= stop:
            return it, x
        rho, old = rh @ r, rho
        beta = (rho / old) * (alpha / omega)
    return limit + 1, x
