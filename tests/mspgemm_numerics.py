"""The masked SpGEMM contract of include/sblas_hip_mspgemm.h restated in numpy: out = M o (X Y^T) for a CSR pattern M
(m x n), X (m x k) and Y (n x k), rows of all three unsorted and with duplicates if they like.  restate() is (V) as a plain
double loop, np.float64 products and adds, one mask entry at a time.  Also the cases both test files (host reference and
GPU plan) go through; the GPU's sizes come from mspgemm_limits().  Values are compared with spgemm_numerics.same_bits."""
from fractions import Fraction

import numpy as np

import spgemm_numerics as GN


def rows_of(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int32), np.diff(np.asarray(rowptr, np.int64)))


def restate(M, X, Y):
    """out (one double per stored mask entry) by the contract; M = (rowptr, colidx), X and Y = (rowptr, colidx, val)"""
    rpm, cim = M[0], M[1]
    rpx, cix, vx = X[0], X[1], np.asarray(X[2], np.float64)
    rpy, ciy, vy = Y[0], Y[1], np.asarray(Y[2], np.float64)
    out = np.zeros(len(cim), np.float64)
    with np.errstate(all="ignore"):
        for i in range(len(rpm) - 1):
            for t in range(rpm[i], rpm[i + 1]):
                j = cim[t]
                acc, first = np.float64(0.0), True                       # no pair: +0.0
                for e in range(rpx[i], rpx[i + 1]):
                    for g in range(rpy[j], rpy[j + 1]):
                        if cix[e] == ciy[g]:
                            p = np.float64(vx[e]) * np.float64(vy[g])
                            acc = p if first else acc + p                # a single product is copied
                            first = False
                out[t] = acc
    return out


def csr_of_rows(rows):
    """(rowptr, colidx, val) from a list of (columns, values)"""
    rp, ci, v = [0], [], []
    for c, w in rows:
        ci += list(c)
        v += list(w)
        rp.append(len(ci))
    return np.array(rp, np.int32), np.array(ci, np.int32), np.array(v, np.float64)


def pattern_of_rows(rows):
    rp, ci, _ = csr_of_rows([(c, [0.0] * len(c)) for c in rows])
    return rp, ci


def empty(rows):
    return np.zeros(rows + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64)


def full_row(rng, cols, length, sort=True):
    """one row of `length` distinct columns out of `cols`, with values"""
    c = rng.choice(cols, length, replace=False)
    return (np.sort(c) if sort else c), rng.random(length) * 2 - 1


def random_case(rng, m, n, k, per_mask, per_x, per_y, sort=True, dup=None):
    """a random (m, n, k, M, X, Y); dup in (None, "m", "x", "y"): that operand gets, in every third non-empty row, a copy
    of the row's first entry appended (a duplicate, and with it an unsorted row)"""
    M = GN.random_csr(rng, m, n, per_mask, sort=sort, empty_every=6)
    X = GN.random_csr(rng, m, k, per_x, sort=sort, empty_every=5)
    Y = GN.random_csr(rng, n, k, per_y, sort=sort, empty_every=7)
    ops = {"m": M, "x": X, "y": Y}
    if dup:
        ops[dup] = add_dups(rng, ops[dup])
    return m, n, k, ops["m"][:2], ops["x"], ops["y"]


def add_dups(rng, A, every=3):
    """A with a copy of the row's first column (and a value of its own) appended to every `every`-th non-empty row"""
    rp, ci, v = A
    rows = []
    for i in range(len(rp) - 1):
        c, w = list(ci[rp[i]:rp[i + 1]]), list(v[rp[i]:rp[i + 1]])
        if c and i % every == 0:
            c.append(c[0]), w.append(float(rng.random() - 0.5))
        rows.append((c, w))
    return csr_of_rows(rows)


def rows_of_lengths(rng, cols, lengths, sort=True):
    """a CSR whose row i has lengths[i] distinct columns"""
    return csr_of_rows([full_row(rng, cols, int(L), sort) for L in lengths])


def identity_pattern(n):
    return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)


def host_cases():
    """name -> (m, n, k, M, X, Y): the places a masked product can go wrong, small enough for the double loop"""
    rng = np.random.default_rng(3500)
    cases = {}
    R = lambda rows, cols, per, **kw: GN.random_csr(rng, rows, cols, per, **kw)
    cases["m0"] = (0, 6, 5, empty(0)[:2], empty(0), R(6, 5, 2))
    cases["n0"] = (6, 0, 5, empty(6)[:2], R(6, 5, 2), empty(0))
    cases["k0"] = (6, 7, 0, R(6, 7, 2)[:2], empty(6), empty(7))
    cases["all0"] = (0, 0, 0, empty(0)[:2], empty(0), empty(0))
    cases["mask_empty"] = (9, 8, 7, empty(9)[:2], R(9, 7, 3), R(8, 7, 3))
    cases["x_empty"] = (9, 8, 7, R(9, 8, 3)[:2], empty(9), R(8, 7, 3))
    cases["y_empty"] = (9, 8, 7, R(9, 8, 3)[:2], R(9, 7, 3), empty(8))
    cases["one_by_one"] = (1, 1, 1, pattern_of_rows([[0]]), csr_of_rows([([0], [1.0 / 3.0])]), csr_of_rows([([0], [3.0])]))
    cases["identity_mask"] = (12, 12, 9, identity_pattern(12), R(12, 9, 3), R(12, 9, 3))
    cases["identity_y"] = (10, 7, 7, R(10, 7, 3)[:2], R(10, 7, 3), identity_pattern(7) + (rng.random(7) + 1.0,))
    # row 0: columns 0 and 1 have pairs, column 2 names a Y row that shares no column with X's row: +0.0
    cases["no_pair"] = (1, 3, 6, pattern_of_rows([[0, 1, 2]]), csr_of_rows([([1, 4], [2.0, -3.0])]),
                        csr_of_rows([([1], [0.5]), ([4, 1], [1.0, 1.0]), ([0, 2, 5], [7.0, 7.0, 7.0])]))
    cases["minus_zero"] = (1, 2, 3, pattern_of_rows([[0, 1]]), csr_of_rows([([2, 0], [-0.0, -1.0])]),
                           csr_of_rows([([2], [5.0]), ([0, 2], [0.0, 1.0])]))
    cases["dup_mask"] = random_case(rng, 14, 11, 9, 3, 3, 3, dup="m")
    cases["dup_x"] = random_case(rng, 14, 11, 9, 3, 3, 3, dup="x")
    cases["dup_y"] = random_case(rng, 14, 11, 9, 3, 3, 3, dup="y")
    # three products on one entry, and the order shows: X's stored order is the major one
    cases["dup_order"] = (1, 1, 4, pattern_of_rows([[0, 0]]), csr_of_rows([([3, 1, 3], [1e16, 1.0, -1e16])]),
                          csr_of_rows([([1, 3], [1.0, 1.0])]))
    cases["dup_order_y"] = (1, 1, 4, pattern_of_rows([[0]]), csr_of_rows([([2], [1.0])]),
                            csr_of_rows([([2, 0, 2, 2], [1e16, 9.0, 1.0, -1e16])]))
    cases["unsorted"] = random_case(rng, 20, 17, 13, 4, 4, 4, sort=False)
    cases["rect"] = random_case(rng, 70, 190, 45, 4, 4, 3)
    cases["rect_unsorted"] = random_case(rng, 70, 190, 45, 4, 4, 3, sort=False, dup="x")
    return cases


def gpu_cases(lim):
    """name -> (m, n, k, M, X, Y): the shapes at which the kernels take another branch; lim = mspgemm_limits()"""
    rng = np.random.default_rng(3530)
    cap, threads = lim["lds_row"], lim["threads"]
    cases = {}
    # X rows at the lane count and at the LDS capacity, each under a mask row long enough that waves begin inside it;
    # Y rows shorter and longer than X's, so that both sides are walked
    k = cap + 40
    xlens = [0, 1, 63, 64, 65, cap - 1, cap, cap + 1, 3, 0, 2, 5]
    ylens = [int(v) for v in rng.choice([0, 2, 40, cap + 30], 90)]
    mlens = [70] * 8 + [3, 4, 0, 5]
    cases["x_row_lengths"] = (len(xlens), 90, k, rows_of_lengths(rng, 90, mlens)[:2], rows_of_lengths(rng, k, xlens), rows_of_lengths(rng, k, ylens))
    # one mask row that crosses workgroups
    cases["long_mask_row"] = (3, 5000, 64, rows_of_lengths(rng, 5000, [2, 5000, 3])[:2], rows_of_lengths(rng, 64, [9, 20, 4]),
                              GN.random_csr(rng, 5000, 64, 3, empty_every=9))
    # one row of 5000 on one side against rows of 3 on the other: the longer side is searched
    short = rows_of_lengths(rng, 6000, [3] * 40)
    hub = rows_of_lengths(rng, 6000, [5000, 3, 0, 3])
    hub_mask = csr_of_rows([([0, int(rng.integers(1, 4))], [0.0, 0.0]) for _ in range(40)])[:2]
    cases["long_y_row"] = (40, 4, 6000, hub_mask, short, hub)
    cases["long_x_row"] = (4, 40, 6000, rows_of_lengths(rng, 40, [40, 7, 2, 0])[:2], hub, short)
    # rows of every length around the wave: waves hold several i
    slens = [int(v) for v in rng.integers(0, 2 * 64 + 30, 40)]
    cases["straddle"] = (40, 300, 50, rows_of_lengths(rng, 300, slens)[:2], GN.random_csr(rng, 40, 50, 6, empty_every=8), GN.random_csr(rng, 300, 50, 5, empty_every=11))
    cases["exact_workgroup"] = (2, threads, 30, rows_of_lengths(rng, threads, [threads, threads])[:2], GN.random_csr(rng, 2, 30, 6),
                                GN.random_csr(rng, threads, 30, 4))
    cases["rect_big"] = random_case(rng, 700, 1900, 450, 4, 5, 4)
    for name in list(cases):                               # the same shapes unsorted: the general path's own cases
        m, n, kk, M, X, Y = cases[name]
        if name in ("x_row_lengths", "straddle", "rect_big"):
            cases[name + "_unsorted"] = (m, n, kk, M, shuffle_rows(rng, X), shuffle_rows(rng, add_dups(rng, Y, every=4)))
    return cases


def shuffle_rows(rng, A):
    """the same matrix with the entries of every row in a random order"""
    rp, ci, v = A
    perm = np.concatenate([rp[i] + rng.permutation(rp[i + 1] - rp[i]) for i in range(len(rp) - 1)] + [np.zeros(0, np.int64)]).astype(np.int64)
    return rp, ci[perm], v[perm]


def special_values(X, Y, seed):
    """the same patterns with -0.0, denormals, +-Inf and NaN sprinkled over the values"""
    rng = np.random.default_rng(seed)
    pool = np.array([-0.0, 0.0, 5e-324, -2.0 ** -1040, np.inf, -np.inf, np.nan, 1.0, -1.0, 1e308, 3.0])
    draw = lambda v: np.where(rng.random(len(v)) < 0.5, pool[rng.integers(0, len(pool), len(v))], v)
    return (X[0], X[1], draw(X[2])), (Y[0], Y[1], draw(Y[2]))


def ascending(rowptr, colidx):
    return all((np.diff(colidx[rowptr[i]:rowptr[i + 1]]) > 0).all() for i in range(len(rowptr) - 1))


def fma(x, y, acc):
    """fma(x, y, acc) with one rounding, exactly (finite arguments)"""
    return float(Fraction(x) * Fraction(y) + Fraction(acc))


# Two entries on which a fused multiply-add changes the last bit: out = fl(fl(x1 * y1) + fl(x2 * y2)) by the contract, and
# both contractions, fma(x2, y2, fl(x1 * y1)) and fma(x1, y1, fl(x2 * y2)), give another double.  Found by a search over
# random triples (test_mspgemm_host.py repeats the arithmetic exactly, with fractions); (x1, y1, x2, y2) each.
FMA_CASES = (
    (-0.2035148685186401, 0.48856322275077213, 0.6054855981078646, -0.15955045331293305),
    (0.659117212148316, -0.35103161645362047, -0.7373731825903156, -0.3089577904640588),
)


def fma_case(q):
    """(m, n, k, M, X, Y) of FMA_CASES[q]: one mask entry, two shared columns"""
    x1, y1, x2, y2 = FMA_CASES[q]
    return 1, 1, 2, pattern_of_rows([[0]]), csr_of_rows([([0, 1], [x1, x2])]), csr_of_rows([([0, 1], [y1, y2])])
