"""What the smoothed-aggregation tests share, restated in numpy on top of amg_numerics and spgemm_numerics,
which are only read: the guard, the prolongator by the pinned rule, the restriction as the stable transpose, the two
products by the SpGEMM contract (V), the row product in lane order and the cycle with general transfer operators.  No GPU
and no library call in here; the aggregation comes in as a function, as in amg_numerics.hierarchy."""
import numpy as np

import amg_numerics as AN
import spgemm_numerics as SN

OMEGA_P = 2.0 / 3.0
MIN_REDUCTION = 0.2                                                         # the Python layer's default for a smoothed plan


def case(name):
    """amg_numerics.case, and random600: the recipe of random4000 at n = 600 with three draws a row"""
    if name != "random600":
        return AN.case(name)
    rng = np.random.default_rng(600)
    rows = []
    for i in range(600):
        cols = set(int(c) for c in rng.integers(0, 600, 3)) - {i}
        r = {c: float(-rng.random() - 0.1) for c in cols}
        r[i] = float(-sum(r.values()) + 1.0)
        rows.append(r)
    n, rp, ci, val = AN.csr_from_rows(rows)
    return dict(name=name, n=n, rp=rp, ci=ci, val=val, symmetric=False, theta=0.0)


CASES = ["n0", "n1", "diagonal300", "tridiagonal3000", "grid24", "grid32", "clique130", "aniso32", "star5000", "random600"]


def keep_level(n, n_next, min_reduction):
    """the coarsening guard: any reduction at all, and at least min_reduction of n; the product is rounded once"""
    return n_next < n and float(n_next) <= (1.0 - float(min_reduction)) * float(n)


def rows_of(n, rp):
    return np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(rp, np.int64)))


def tentative_values(n, rp, ci, val, omega_p=OMEGA_P):
    """t_e for every stored entry: q_i = omega_P / a_ii; -(q_i a_ie) off the diagonal, 1 - q_i a_ii on it.  numpy rounds each
    elementwise operation on its own (no fma)."""
    row = rows_of(n, rp)
    on = row == np.asarray(ci, np.int64)
    val = np.asarray(val, np.float64)
    d = np.zeros(n)
    d[row[on]] = val[on]
    with np.errstate(all="ignore"):
        q = np.float64(omega_p) / d
        prod = q[row] * val
        return np.where(on, np.float64(1.0) - prod, -prod)


def prolongator(n, rp, ci, val, agg, n_agg, omega_p=OMEGA_P):
    """P: the COO sum of the triplets (row(e), agg[col(e)], t_e) in stored order -> (rowptr, colidx, val)"""
    row = rows_of(n, rp).astype(np.int32)
    col = np.asarray(agg, np.int32)[np.asarray(ci, np.int64)]
    return SN.sum_triplets(n, row, col, tentative_values(n, rp, ci, val, omega_p))


def hierarchy(c, aggregate, prolongator_kind="smoothed", omega_p=OMEGA_P, min_reduction=None, coarse_max=64, max_levels=20, seed=0,
              smoother="jacobi", omega=None):
    """The levels of case c: a list of dicts(n, rowptr, colidx, val, wd) with, above the coarsest, agg, aggptr, members and for
    a smoothed hierarchy p_rowptr, p_colidx, p_val, r_rowptr, r_colidx, r_val.  A plain hierarchy is amg_numerics' with the
    guard in front of it."""
    if min_reduction is None:
        min_reduction = MIN_REDUCTION if prolongator_kind == "smoothed" else 0.0
    n, rp, ci, val, theta = c["n"], c["rp"], c["ci"], c["val"], c["theta"]
    levels = []
    if n == 0:
        return levels
    while True:
        L = dict(n=n, rowptr=rp, colidx=ci, val=val, wd=AN.weights(n, rp, ci, val, smoother, omega))
        levels.append(L)
        if not (n > coarse_max and len(levels) < max_levels):
            return levels
        agg, aggptr, members = aggregate(n, rp, ci, val if theta > 0.0 else None, theta, seed, len(levels) - 1)[:3]
        nc = len(aggptr) - 1
        if not keep_level(n, nc, min_reduction):
            return levels
        L.update(agg=agg, aggptr=aggptr, members=members)
        if prolongator_kind == "smoothed":
            prp, pci, pv = prolongator(n, rp, ci, val, agg, nc, omega_p)
            rrp, rci, rv = SN.transpose_csr(n, nc, prp, pci, pv)
            ap = SN.reference(n, nc, rp, ci, val, prp, pci, pv)
            crp, cci, cv = SN.reference(nc, nc, rrp, rci, rv, *ap)
            L.update(p_rowptr=prp, p_colidx=pci, p_val=pv, r_rowptr=rrp, r_colidx=rci, r_val=rv)
        else:
            crp, cci, perm, runptr = AN.galerkin(n, rp, ci, agg, nc)
            L.update(perm=perm, runptr=runptr)
            cv = AN.assemble(val, perm, runptr)
        n, rp, ci, val = nc, crp, cci, cv


def fixed(levels):
    """an `aggregate` for hierarchy() that repeats the aggregates of `levels` (setup with other values keeps them); a level
    that was discarded reduces nothing: singletons, which no guard keeps"""
    def aggregate(n, rp, ci, val, theta, seed, level):
        if "agg" in levels[level]:
            return levels[level]["agg"], levels[level]["aggptr"], levels[level]["members"]
        return np.arange(n, dtype=np.int32), np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)
    return aggregate


def sizes(levels):
    return [L["n"] for L in levels]


def operator_complexity(levels):
    return sum(len(L["colidx"]) for L in levels) / max(len(levels[0]["colidx"]), 1)


def transfer(rowptr, colidx, val, x):
    """s_i over every stored row of M in the sweep's lane order"""
    return AN.row_sums(dict(n=len(rowptr) - 1, rowptr=rowptr, colidx=colidx, val=val), np.asarray(x, np.float64))


def cycle_py(levels, r, nu=1, coarse_sweeps=8, scale=1.0, l=0):
    """amg_numerics.cycle_py with the transfers as row products: b_c = R res, x = x + scale * (P e)"""
    L = levels[l]
    b = np.asarray(r, np.float64)
    x = L["wd"] * b
    if l + 1 == len(levels):
        for _ in range(coarse_sweeps - 1):
            x = x + L["wd"] * (b - AN.row_sums(L, x))
        return x
    for _ in range(nu - 1):
        x = x + L["wd"] * (b - AN.row_sums(L, x))
    res = b - AN.row_sums(L, x)
    bc = transfer(L["r_rowptr"], L["r_colidx"], L["r_val"], res)
    e = cycle_py(levels, bc, nu, coarse_sweeps, scale, l + 1)
    x = x + np.float64(scale) * transfer(L["p_rowptr"], L["p_colidx"], L["p_val"], e)
    for _ in range(nu):
        x = x + L["wd"] * (b - AN.row_sums(L, x))
    return x


_made = {}


def built(name, aggregate):
    """(case, its smoothed hierarchy with the defaults), made once a process and never changed"""
    if name not in _made:
        c = case(name)
        _made[name] = (c, hierarchy(c, aggregate))
    return _made[name]
