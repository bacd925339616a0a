"""The narrow SDDMM's contract (include/sblas_hip_sddmm_narrow.h) restated in Python with an exact rational fma (a plain
helper module, like sddmm_numerics.py, which it builds on): for every stored entry e = (r, c) inside the part

    k <= 4:       s = +0, then s = fma(x_j, y_j, s) for j ascending
    5 <= k <= 8:  s0 over j in {0, 1, 4, 5}, s1 over j in {2, 3, 6, 7}, those below k, each from +0 by fma in ascending j;
                  s = s0 + s1
    out[e] = alpha * s, or fma(beta, old[e], alpha * s)

and +0.0 or beta * old[e] outside it.  Nothing here shares code with the library.  (The library also runs the padded steps
fma(+0, +0, s) of the kernel it promises the bits of; they change the sign of a zero sum at most, which == does not see.)"""
from fractions import Fraction

import numpy as np

from sddmm_numerics import entry_rows

PARTS = ("all", "lower", "upper", "strict_lower", "strict_upper")


def fma(x, y, acc):
    """fma(x, y, acc) with one rounding, exactly (finite arguments)"""
    return float(Fraction(x) * Fraction(y) + Fraction(acc))


def in_part(part, r, c):
    return {"all": True, "lower": c <= r, "upper": c >= r, "strict_lower": c < r, "strict_upper": c > r}[part]


def dot(x, y):
    k = len(x)
    assert 1 <= k <= 8
    if k <= 4:
        s = 0.0
        for j in range(k):
            s = fma(x[j], y[j], s)
        return s
    s0 = s1 = 0.0
    for j in (0, 1, 4, 5):
        if j < k:
            s0 = fma(x[j], y[j], s0)
    for j in (2, 3, 6, 7):
        if j < k:
            s1 = fma(x[j], y[j], s1)
    return s0 + s1


def restate(rowptr, colidx, X, Y, old, alpha, beta, part="all"):
    r, c = entry_rows(rowptr, colidx)
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    out = np.zeros(len(c))
    for e in range(len(c)):
        if not in_part(part, int(r[e]), int(c[e])):
            out[e] = 0.0 if beta == 0 else beta * old[e]
            continue
        sres = alpha * dot([float(v) for v in X[r[e]]], [float(v) for v in Y[c[e]]])
        out[e] = sres if beta == 0 else fma(beta, float(old[e]), sres)
    return out


def small_pattern(seed=0, rows=12, cols=12):
    """empty rows, duplicates, unsorted columns, every part populated"""
    rng = np.random.default_rng(seed)
    lens = [int(rng.integers(0, 7)) for _ in range(rows)]
    lens[1] = lens[rows - 2] = 0
    ci = []
    for i, n in enumerate(lens):
        row = rng.integers(0, cols, n).tolist()
        if n >= 3:
            row[2] = row[0]                          # a duplicate
        if n >= 2 and i < cols:
            row[1] = i                               # a diagonal entry behind another column: unsorted
        ci.extend(row)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return rows, cols, rp, np.asarray(ci, np.int32)
