"""What the FSAI tests share: the cases, G's pattern and G's values restated in Python (one IEEE operation each, on Python
floats), and G as a dense matrix for the checks that need one.  No GPU and no library call in here."""
import math

import numpy as np

ROW_MAX = 64                                                                # the header's, restated on purpose


# ---- the cases ------------------------------------------------------------------------------------------------------
def csr_of(dense, stored=None):
    """the stored entries are those of the mask `stored`, by default the nonzeros of the dense matrix; rows ascend"""
    n = dense.shape[0]
    stored = dense != 0 if stored is None else stored
    rp, ci, val = [0], [], []
    for i in range(n):
        cols = np.flatnonzero(stored[i])
        ci.extend(int(c) for c in cols)
        val.extend(float(v) for v in dense[i, cols])
        rp.append(len(ci))
    return n, np.array(rp, np.int32), np.array(ci, np.int32), np.array(val, np.float64)


def band(n, half, diag):
    """a_ij = -1 / (|i - j| + 1) inside the band: diagonally dominant for the (half, diag) used here"""
    A = np.zeros((n, n))
    for i in range(n):
        for j in range(max(0, i - half), min(n, i + half + 1)):
            A[i, j] = diag if i == j else -1.0 / (abs(i - j) + 1)
    return A


def grid(side):
    A = np.zeros((side * side, side * side))
    for y in range(side):
        for x in range(side):
            i = y * side + x
            A[i, i] = 4.0
            for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                if 0 <= x + dx < side and 0 <= y + dy < side:
                    A[i, (y + dy) * side + x + dx] = -1.0
    return A


def clique(n):
    A = np.array([[-0.01 * (1 + (i + j) % 3) for j in range(n)] for i in range(n)])
    np.fill_diagonal(A, 3.0)
    return A


def random_spd(n, partners, seed):
    rng = np.random.default_rng(seed)
    A = np.zeros((n, n))
    for i in range(n):
        for j in rng.choice(n, partners, replace=False):
            if i != j:
                A[i, j] = A[j, i] = -(0.25 + rng.random())
    np.fill_diagonal(A, np.abs(A).sum(axis=1) + 1.0)
    return A


def mixed_tiers(n=70):
    """every stretch of 64 rows holds rows of 4, of 16 and of 64 lanes: row i's lower part has 1 .. 3, up to 21 or up to 64
    entries by i mod 3"""
    A = np.zeros((n, n))
    for i in range(n):
        reach = (2, 20, 63)[i % 3]
        for j in range(max(0, i - reach), i):
            A[i, j] = A[j, i] = -0.01 * (1 + (7 * i + 3 * j) % 5)
    np.fill_diagonal(A, 8.0)
    return A


def lower_of_square(rp, ci):
    """the lower triangle of the pattern of A^2, as a CSR pattern"""
    n = len(rp) - 1
    P = np.zeros((n, n), bool)
    P[np.repeat(np.arange(n), np.diff(rp)), ci] = True
    P2 = np.tril((P.astype(np.int64) @ P.astype(np.int64)) > 0)
    prp, pci = [0], []
    for i in range(n):
        pci.extend(int(c) for c in np.flatnonzero(P2[i]))
        prp.append(len(pci))
    return np.array(prp, np.int32), np.array(pci, np.int32)


_BUILDERS = {
    "n0": lambda: (np.zeros((0, 0)), {}),
    "n1": lambda: (np.array([[2.5]]), {}),
    "diagonal40": lambda: (np.diag(1.0 + np.arange(40.0) % 7), {}),
    "tridiagonal300": lambda: (band(300, 1, 2.5), {}),
    "grid24": lambda: (grid(24), {}),
    "band6": lambda: (band(200, 6, 4.0), {}),
    "band20": lambda: (band(150, 20, 8.0), {}),
    "band20_max8": lambda: (band(150, 20, 8.0), dict(max_row=8)),
    "band20_max1": lambda: (band(150, 20, 8.0), dict(max_row=1)),
    "clique70_max64": lambda: (clique(70), dict(max_row=64)),
    "random500": lambda: (random_spd(500, 6, 11), {}),
    "grid12_squared": lambda: (grid(12), dict(squared=True)),
    "mixed70": lambda: (mixed_tiers(), {}),
}
CASES = list(_BUILDERS)
_made = {}


def case(name):
    """-> dict(name, n, rp, ci, val, dense, pattern (None or (rp, ci)), max_row (None or k)); built once"""
    if name not in _made:
        dense, opt = _BUILDERS[name]()
        n, rp, ci, val = csr_of(dense)
        pat = lower_of_square(rp, ci) if opt.get("squared") else None
        _made[name] = dict(name=name, n=n, rp=rp, ci=ci, val=val, dense=dense, pattern=pat, max_row=opt.get("max_row"))
    return _made[name]


# ---- the pattern ----------------------------------------------------------------------------------------------------
class Refused(Exception):
    def __init__(self, row):
        super().__init__("row %d" % row)
        self.bad_row = row


def pattern(n, rp, ci, pat=None, max_row=None):
    """G's pattern -> (rowptr_g, colidx_g), or Refused(first bad row).  A's own structure is taken as checked."""
    srp, sci = (rp, ci) if pat is None else pat
    out_rp, out_ci = [0], []
    for i in range(n):
        cols = [int(c) for c in sci[srp[i]:srp[i + 1]]]
        if any(c < 0 or c >= n for c in cols) or any(b <= a for a, b in zip(cols, cols[1:])):
            raise Refused(i)
        low = [c for c in cols if c <= i]
        if not low or low[-1] != i:
            raise Refused(i)
        if max_row is not None and len(low) > max_row:
            low = low[len(low) - max_row:]
        if len(low) > ROW_MAX:
            raise Refused(i)
        out_ci.extend(low)
        out_rp.append(len(out_ci))
    return np.array(out_rp, np.int32), np.array(out_ci, np.int32)


# ---- the values -----------------------------------------------------------------------------------------------------
def positive(v):
    return v > 0.0 and math.isfinite(v)


def row_values(rows, J):
    """one row of G by the scalar loop: rows[r] is {column: value} of A's row r -> (g, failed)"""
    m = len(J)
    M = [[float(rows[J[p]].get(J[q], 0.0)) for q in range(p + 1)] for p in range(m)]
    aii = M[m - 1][m - 1]
    for k in range(m):
        d = M[k][k]
        if not positive(d):
            return [0.0] * (m - 1) + [1.0 / math.sqrt(aii) if positive(aii) else 1.0], True
        c = math.sqrt(d)
        M[k][k] = c
        for p in range(k + 1, m):
            M[p][k] = M[p][k] / c
        for p in range(k + 1, m):
            for q in range(k + 1, p + 1):
                prod = M[p][k] * M[q][k]
                M[p][q] = M[p][q] - prod
    g, t = [0.0] * m, [0.0] * m
    g[m - 1] = 1.0 / M[m - 1][m - 1]
    for q in range(m - 1, 0, -1):
        for p in range(q):
            prod = M[q][p] * g[q]
            t[p] = t[p] + prod
        g[q - 1] = (-t[q - 1]) / M[q - 1][q - 1]
    return g, False


def values(n, rp, ci, val, grp, gci):
    """G's values on the pattern (grp, gci) -> (val_g, least failed row or None)"""
    rows = [{int(c): float(v) for c, v in zip(ci[rp[i]:rp[i + 1]], val[rp[i]:rp[i + 1]])} for i in range(n)]
    out, bad = [], None
    for i in range(n):
        g, failed = row_values(rows, [int(c) for c in gci[grp[i]:grp[i + 1]]])
        out.extend(g)
        if failed and bad is None:
            bad = i
    return np.array(out, np.float64), bad


def dense_g(n, grp, gci, gval):
    G = np.zeros((n, n))
    G[np.repeat(np.arange(n), np.diff(grp)), gci] = gval
    return G


# ---- the planted failures: name -> (n, rp, ci, val, least failed row) -----------------------------------------------
def failures():
    out = {}
    for name, what in (("negative_diagonal", -4.0), ("zero_diagonal", 0.0), ("nan_diagonal", float("nan")), ("inf_diagonal", float("inf"))):
        A = grid(8)
        stored = A != 0
        A[20, 20] = A[41, 41] = what
        out[name] = csr_of(A, stored) + (20,)
    for name, what in (("nan_value", float("nan")), ("inf_value", float("inf"))):
        A = band(60, 6, 4.0)
        stored = A != 0
        A[30, 27] = A[27, 30] = what
        A[50, 49] = A[49, 50] = what
        out[name] = csr_of(A, stored) + (30,)
    A = band(40, 1, 2.5)
    A[10, 10], A[11, 11], A[11, 10], A[10, 11] = 1.0, 1.0, 2.0, 2.0           # [[1, 2], [2, 1]]: the second pivot is 1 - 4
    out["indefinite_block"] = csr_of(A) + (11,)
    return out
