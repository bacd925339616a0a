"""The triangular-solve contract of include/sblas_hip.h restated in numpy (a plain helper module; no scipy, and nothing
shared with the kernels): T x = alpha b for the lower or upper triangle T of a square CSR matrix whose rows may be
unsorted and hold off-diagonal duplicates (they add) and entries in the other triangle (ignored); unit=True ignores
stored diagonals and uses 1.

- levels(): level(i) = 0 when row i selects no off-diagonal entry, else 1 + the greatest level among the rows named.
- pack(): the rows by (level, row) and every level's four-lane units, each row aligned to its own unit count.
- reference(): forward / backward substitution in double-double (the error-free pieces of numerics.py).
- residual_bound(): the rounding-error bound on the residual that every correct evaluation order satisfies.
- grid_problem(): integer data on which every order of every sum is exact, so the solve must return x with ==.
- solve_lane_order(): SpSV's results contract restated operation by operation, for equality of bits.
- the generators of the shapes the tests use."""
import numpy as np

import numerics as NM


# ---------------------------------------------------------------------------------------------------------------------
# structure
# ---------------------------------------------------------------------------------------------------------------------
def csr_of_rows(rows):
    """(rowptr, colidx) from a list of column lists"""
    rp = np.zeros(len(rows) + 1, np.int64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.concatenate([np.asarray(r, np.int64) for r in rows]) if len(rows) and rp[-1] else np.zeros(0, np.int64)
    return rp.astype(np.int32), ci.astype(np.int32)


def selected(rowptr, colidx, lower):
    """mask over the stored entries: strictly inside the triangle"""
    row = NM.row_of_entries(rowptr)
    col = np.asarray(colidx, np.int64)
    return col < row if lower else col > row


def on_diagonal(rowptr, colidx):
    return np.asarray(colidx, np.int64) == NM.row_of_entries(rowptr)


def levels(n, rowptr, colidx, lower=True):
    """level of every row and the number of levels, by the rule's own words"""
    rp, ci = np.asarray(rowptr, np.int64), np.asarray(colidx, np.int64)
    lv = np.zeros(n, np.int64)
    for i in (range(n) if lower else range(n - 1, -1, -1)):
        c = ci[rp[i]:rp[i + 1]]
        c = c[c < i] if lower else c[c > i]
        lv[i] = 0 if len(c) == 0 else 1 + lv[c].max()
    return lv, (int(lv.max()) + 1 if n else 0)


def level_widths(lv, n_levels):
    return np.bincount(lv, minlength=n_levels).astype(np.int64)


def units_per_row(p, g4_max, g16_max):
    """four-lane units of a row of p stored entries: G(p) / 4 for G = 4 (p <= g4_max), 16 (p <= g16_max) or 64 lanes"""
    return 1 if p <= g4_max else 4 if p <= g16_max else 16


def pack(n, rowptr, level, n_levels, g4_max, g16_max):
    """-> (perm, level_ptr, level_unit_ptr, unit_row, unit_q) by the rule's own words: the rows sorted stably by level;
    in a level each row takes its units_per_row() units numbered from 0, starting on a multiple of that count from the
    level's start, and (-1, 0) pads the gaps"""
    rp = np.asarray(rowptr, np.int64)
    perm = np.argsort(np.asarray(level, np.int64), kind="stable")
    level_ptr, level_unit_ptr, unit_row, unit_q = [0], [0], [], []
    for l in range(n_levels):
        rows = [int(i) for i in perm if level[i] == l]
        at = 0                                                              # units of this level so far
        for i in rows:
            per = units_per_row(rp[i + 1] - rp[i], g4_max, g16_max)
            pads = -at % per
            unit_row += [-1] * pads + [i] * per
            unit_q += [0] * pads + list(range(per))
            at += pads + per
        level_ptr.append(level_ptr[-1] + len(rows))
        level_unit_ptr.append(level_unit_ptr[-1] + at)
    return (perm.astype(np.int32), np.array(level_ptr, np.int32), np.array(level_unit_ptr, np.int64),
            np.array(unit_row, np.int32), np.array(unit_q, np.int32))


# ---------------------------------------------------------------------------------------------------------------------
# double-double substitution
# ---------------------------------------------------------------------------------------------------------------------
def _dd_sum(hi, lo):
    """double-double sum over axis 0 of (hi, lo)[k, ...]: a pairwise tree"""
    while hi.shape[0] > 1:
        k = hi.shape[0] // 2
        h, l = NM._dd_add(hi[:k], lo[:k], hi[k:2 * k], lo[k:2 * k])
        if hi.shape[0] % 2:
            h, l = np.concatenate([h, hi[-1:]]), np.concatenate([l, lo[-1:]])
        hi, lo = h, l
    return hi[0], lo[0]


def _dd_times(t, xh, xl):
    """t (double) * (xh, xl) as a double-double; t broadcasts over the leading axis"""
    p, e = NM._two_prod(t, xh)
    return NM._fast_two_sum(p, e + t * xl)


def _dd_div(rh, rl, d):
    """(rh, rl) / d for a double d"""
    q1 = rh / d
    p, e = NM._two_prod(q1, d)
    h, l = NM._dd_add(rh, rl, -p, -e)
    q2 = (h + l) / d
    return NM._fast_two_sum(q1, q2)


def reference(n, rowptr, colidx, val, b, lower=True, unit=False, alpha=1.0):
    """x with T x = alpha * b by substitution in double-double, rounded to double at the end.  b: (n,) or (n, k).  Finite
    data that neither overflows nor underflows; its own error is some 2^-100 of the terms' magnitudes a row."""
    rp, ci = np.asarray(rowptr, np.int64), np.asarray(colidx, np.int64)
    val = np.asarray(val, np.float64)
    b2 = np.asarray(b, np.float64).reshape(n, -1)
    k = b2.shape[1]
    xh, xl = np.zeros((n, k)), np.zeros((n, k))
    ah, al = NM._two_prod(np.float64(alpha), b2)
    for i in (range(n) if lower else range(n - 1, -1, -1)):
        c, v = ci[rp[i]:rp[i + 1]], val[rp[i]:rp[i + 1]]
        sel = c < i if lower else c > i
        rh, rl = ah[i], al[i]
        if sel.any():
            th, tl = _dd_times(v[sel][:, None], xh[c[sel]], xl[c[sel]])
            sh, sl = _dd_sum(th, tl)
            rh, rl = NM._dd_add(rh, rl, -sh, -sl)
        if unit:
            xh[i], xl[i] = rh, rl
        else:
            d = v[c == i]
            assert len(d) == 1, "row %d stores %d diagonal entries" % (i, len(d))
            xh[i], xl[i] = _dd_div(rh, rl, d[0])
    return (xh + xl).reshape(np.shape(b))


def solve_lane_order(n, rowptr, colidx, val, b, lower=True, unit=False, alpha=1.0):
    """x with the bits the results contract of sptrsv.hip promises: row i's sum over its selected entries in lane order
    (amg_numerics.lane_order_sum: G from the stored length of the whole row, a rejected entry takes no fma and is not
    read), then three roundings -- alpha * b_i, the subtraction, the division by the stored diagonal (1 under unit).
    One stored diagonal a row unless unit."""
    import amg_numerics as AN                                               # here: amg_numerics' own imports lead back to this module
    rp, ci = np.asarray(rowptr, np.int64), np.asarray(colidx, np.int64)
    take, dg = selected(rp, ci, lower).tolist(), on_diagonal(rp, ci)
    cl, vl, bl = ci.tolist(), np.asarray(val, np.float64).tolist(), np.asarray(b, np.float64).tolist()
    x = [float("nan")] * n                                                  # a row that is read before it is solved shows
    for i in (range(n) if lower else range(n - 1, -1, -1)):
        beg, end = int(rp[i]), int(rp[i + 1])
        s = AN.lane_order_sum(cl, vl, x, beg, end, take)
        pivot = 1.0
        if not unit:
            d = np.flatnonzero(dg[beg:end])
            assert len(d) == 1, "row %d stores %d diagonal entries" % (i, len(d))
            pivot = vl[beg + int(d[0])]
        t = float(alpha) * bl[i]
        x[i] = (t - s) / pivot
    return np.array(x, np.float64)


def residual_bound(n, rowptr, colidx, val, b, x, lower=True, unit=False, alpha=1.0):
    """-> (residual, bound), each shaped like x: residual_i = alpha b_i - sum_j t_ij x_j over row i of T (the diagonal
    included), evaluated in double-double, and

        bound_i = gamma(p_i + 3) * (|alpha b_i| + sum_j |t_ij| |x_j|) + (p_i + 3) * eta,

    p_i = the selected off-diagonal entries of row i (duplicates counted), gamma(m) = m u / (1 - m u), eta = the smallest
    subnormal.  Derivation.  A kernel computes x_i = fl(fl(fl(alpha b_i) - s) / t_ii), s a floating-point sum of the p_i
    products t_ij x_j in some order, fused or not.  Whatever the order, a product enters s through at most p_i roundings:
    unfused, its own and at most p_i - 1 additions; fused, one per multiply-add on its path, and a path that merges q
    partial sums has left at most p_i - q products for the additions before.  Adding an exact zero (an idle lane, the
    start of a sum) rounds nothing.  So s = sum_j t_ij x_j (1 + theta_j), |theta_j| <= gamma(p_i).  One more rounding each
    for alpha b_i (delta_1), the subtraction (delta_2) and the division (delta_3):
        t_ii x_i (1 + delta_3) = (alpha b_i (1 + delta_1) - s) (1 + delta_2),
    hence alpha b_i - s0 - t_ii x_i = -alpha b_i delta_1 + sum_j t_ij x_j theta_j + t_ii x_i ((1 + delta_3) / (1 + delta_2) - 1)
    with s0 the exact sum, which is at most gamma(p_i + 3) (|alpha b_i| + sum_j |t_ij x_j|) in magnitude (the standard
    product-of-(1 + delta) lemma; every factor above is within gamma(p_i + 3)); each rounding may instead be an underflow,
    which costs at most eta.  No measured margin enters."""
    rp, ci = np.asarray(rowptr, np.int64), np.asarray(colidx, np.int64)
    val = np.asarray(val, np.float64)
    shape = np.shape(x)
    x2, b2 = np.asarray(x, np.float64).reshape(n, -1), np.asarray(b, np.float64).reshape(n, -1)
    sel = selected(rp, ci, lower)
    p = NM.row_sums(rp, sel.astype(np.int64))
    keep = sel if unit else (sel | on_diagonal(rp, ci))
    row = NM.row_of_entries(rp)[keep]
    c, v = ci[keep], val[keep]
    if unit:                                                                # the implied diagonal: one more entry a row
        row, c, v = np.concatenate([row, np.arange(n)]), np.concatenate([c, np.arange(n)]), np.concatenate([v, np.ones(n)])
        order = np.argsort(row, kind="stable")
        row, c, v = row[order], c[order], v[order]
    rp_t = np.zeros(n + 1, np.int64)
    rp_t[1:] = np.cumsum(np.bincount(row, minlength=n))
    th, tl = NM._two_prod(v[:, None], x2[c])
    sh, sl = NM._dd_row_sums(rp_t, th, tl)
    ah, al = NM._two_prod(np.float64(alpha), b2)
    rh, rl = NM._dd_add(ah, al, -sh, -sl)
    mag = np.abs(alpha * b2) + NM.row_sums(rp_t, np.abs(v)[:, None] * np.abs(x2[c]))
    m = (p + 3).astype(np.float64)[:, None]
    bound = NM.gamma(m, np.float64) * mag + m * NM.eta(np.float64)
    return (rh + rl).reshape(shape), bound.reshape(shape)


def check_residual(n, rowptr, colidx, val, b, x, lower=True, unit=False, alpha=1.0, what=""):
    res, bnd = residual_bound(n, rowptr, colidx, val, b, x, lower, unit, alpha)
    worst = float(np.max(np.abs(res) / bnd)) if res.size else 0.0
    print("%s: residual / bound at most %.3g" % (what, worst))
    assert np.all(np.isfinite(res)), what
    assert np.all(np.abs(res) <= bnd), "%s: residual above the bound at %s (ratio %.3g)" % (what, np.argwhere(np.abs(res) > bnd)[:3].tolist(), worst)


# ---------------------------------------------------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------------------------------------------------
def dominant_values(rng, n, rowptr, colidx, lower=True, unit=False):
    """values for the pattern with |t_ii| >= 1 + sum |t_ij| over the selected entries: off-diagonals log-uniform in
    [2^-4, 2^4) with random signs (the other triangle too: it must not matter), the diagonal up to twice the sum; under
    unit the off-diagonals of a row are scaled to sum below 1 instead and stored diagonals get a value that must not
    be used"""
    rp = np.asarray(rowptr, np.int64)
    nnz = len(colidx)
    val = NM.log_uniform(rng, nnz, 8)                                       # signed
    sel, dg = selected(rp, colidx, lower), on_diagonal(rp, colidx)
    if unit:
        s = NM.row_sums(rp, np.where(sel, np.abs(val), 0.0))
        scale = np.where(s > 0.5, 0.5 / np.maximum(s, 1e-300), 1.0)
        val = np.where(sel, val * scale[NM.row_of_entries(rp)], val)
        val[dg] = 1e30
    else:
        s = NM.row_sums(rp, np.where(sel, np.abs(val), 0.0))
        d = (1.0 + s) * (1.0 + rng.random(n)) * rng.choice([-1.0, 1.0], n)
        val[dg] = d[NM.row_of_entries(rp)[dg]]
    return val


class Exact:
    pass


def grid_problem(rng, n, rowptr, colidx, lower=True, unit=False, nrhs=None):
    """T with power-of-two diagonals (1, 2, 4, 8) and off-diagonals in -4 .. 4, x in -8 .. 8, b' = T x formed in int64 and
    handed over as b = b' / alpha for alpha = 1/2 (exact).  alpha * b is then b' exactly, every partial sum of every
    row, in any order, fused or not, is an integer far below 2^53, and b'_i - sum = t_ii x_i divides exactly: the solve
    must return x with ==.  Entries in the other triangle and, under unit, stored diagonals get values that would spoil
    the result if they were used."""
    rp, ci = np.asarray(rowptr, np.int64), np.asarray(colidx, np.int64)
    nnz = len(ci)
    sel, dg = selected(rp, ci, lower), on_diagonal(rp, ci)
    tv = rng.integers(-4, 5, nnz)
    tv[dg] = 2 ** rng.integers(0, 4, int(dg.sum()))
    shape = (n,) if nrhs is None else (n, nrhs)
    x = rng.integers(-8, 9, shape)
    x2 = x.reshape(n, -1)
    use = sel if unit else (sel | dg)
    terms = np.where(use, tv, 0)[:, None] * x2[ci]
    bp = NM.row_sums(rp, terms) + (x2 if unit else 0)
    g = Exact()
    g.val = tv.astype(np.float64)
    if unit:
        g.val[dg] = 3.0                                                     # stored, and to be ignored
    g.alpha = 0.5
    g.b = (bp * 2).astype(np.float64).reshape(shape)
    g.x = x.astype(np.float64)
    return g


# ---------------------------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------------------------
def triangle_of(n, rowptr, colidx, lower=True):
    """the pattern's triangle plus a full diagonal, rows sorted, no duplicates (for matrices that lack diagonals)"""
    rp = np.asarray(rowptr, np.int64)
    rows = []
    for i in range(n):
        c = np.unique(np.asarray(colidx[rp[i]:rp[i + 1]], np.int64))
        c = c[c < i] if lower else c[c > i]
        rows.append(np.concatenate([c, [i]]) if lower else np.concatenate([[i], c]))
    return csr_of_rows(rows)


def grid5(side, lower=True):
    """the lower (or upper) part of the five-point stencil on a side x side grid: diagonal, west and south neighbours"""
    rows = []
    for i in range(side * side):
        r, c = divmod(i, side)
        nb = ([i - side] if r > 0 else []) + ([i - 1] if c > 0 else []) if lower else \
             ([i + 1] if c < side - 1 else []) + ([i + side] if r < side - 1 else [])
        rows.append(nb + [i] if lower else [i] + nb)
    return csr_of_rows(rows)


def bidiagonal(n):
    return csr_of_rows([[0]] + [[i - 1, i] for i in range(1, n)])


def diagonal(n):
    return csr_of_rows([[i] for i in range(n)])


def arrow(n):
    """dense first column plus dense last row (lower)"""
    return csr_of_rows([[0]] + [[0, i] for i in range(1, n - 1)] + [list(range(n))])


def random_lower(rng, n, per_row=3):
    """per_row columns drawn from [0, i) for every row i > 0 (duplicates possible: they add), then the diagonal"""
    return csr_of_rows([[0]] + [list(rng.integers(0, i, per_row)) + [i] for i in range(1, n)])


def staircase(widths):
    """levels of exactly the given widths: every row of level l > 0 names one row of level l - 1"""
    rows, first = [], 0
    for l, w in enumerate(widths):
        prev = first - widths[l - 1] if l else 0
        for k in range(w):
            i = first + k
            rows.append([i] if l == 0 else [prev + k % widths[l - 1], i])
        first += w
    return csr_of_rows(rows)


def row_lengths_case(lengths):
    """lower triangle whose later rows have exactly the given stored lengths (diagonal included), after enough
    diagonal-only rows to name"""
    lead = max(lengths)
    rows = [[i] for i in range(lead)]
    for k, L in enumerate(lengths):
        i = lead + k
        rows.append(list(range(L - 1)) + [i])
    return csr_of_rows(rows)


def messy(rng, n):
    """unsorted rows with off-diagonal duplicates and entries in both triangles, one diagonal a row"""
    rows = []
    for i in range(n):
        k = int(rng.integers(0, 7))
        c = list(rng.integers(0, n, k))
        c = [j for j in c if j != i]
        if c and rng.random() < 0.5:
            c += c[:2]                                                       # duplicates
        c.append(i)
        rows.append(list(rng.permutation(c)))
    return csr_of_rows(rows)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)
