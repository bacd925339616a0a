"""The GEAM contract of include/sblas_hip_geam.h restated in numpy on top of tests/spgemm_numerics.py: C = alpha * A +
beta * B is sum_triplets() of A's triplets (i, j, alpha * a) followed by B's (i, j, beta * b), and dest_a / dest_b are
read off the same stable lexsort.  Also the shapes both test files (host reference and GPU plan) go through."""
import numpy as np

import spgemm_numerics as GN

SCALARS = (1.0, -1.0, 0.0, 0.5, 3e200)


def rows_of(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int32), np.diff(np.asarray(rowptr, np.int64)))


def restate(rows, A, B, alpha, beta):
    """(rowptr_c, colidx_c, val_c, dest_a, dest_b) by the contract"""
    na = len(A[1])
    row = np.concatenate((rows_of(A[0]), rows_of(B[0]))).astype(np.int32)
    col = np.concatenate((A[1], B[1])).astype(np.int32)
    with np.errstate(all="ignore"):
        val = np.concatenate((np.float64(alpha) * np.asarray(A[2], np.float64), np.float64(beta) * np.asarray(B[2], np.float64)))
    rowptr, colidx, out = GN.sum_triplets(rows, row, col, val)
    dest = np.zeros(len(row), np.int32)
    if len(row):
        order = np.lexsort((col, row))
        head = np.ones(len(row), bool)
        head[1:] = (row[order][1:] != row[order][:-1]) | (col[order][1:] != col[order][:-1])
        dest[order] = np.cumsum(head) - 1
    return rowptr, colidx, out, dest[:na], dest[na:]


def csr_of_rows(rows):
    """(rowptr, colidx, val) from a list of (columns, values)"""
    rp, ci, v = [0], [], []
    for c, w in rows:
        ci += list(c)
        v += list(w)
        rp.append(len(ci))
    return np.array(rp, np.int32), np.array(ci, np.int32), np.array(v, np.float64)


def empty(rows):
    return np.zeros(rows + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64)


def with_pattern(rng, pattern_rows):
    return csr_of_rows([(c, rng.random(len(c)) * 2 - 1) for c in pattern_rows])


def shape_cases():
    """name -> (rows, cols, A, B): the places a sum of two patterns can go wrong"""
    rng = np.random.default_rng(3400)
    cases = {}
    cases["rows0"] = (0, 5, empty(0), empty(0))
    one = [[0] if rng.random() < 0.6 else [] for _ in range(9)]
    two = [[0] if rng.random() < 0.6 else [] for _ in range(9)]
    cases["cols1"] = (9, 1, with_pattern(rng, one), with_pattern(rng, two))
    cases["both_empty"] = (7, 9, empty(7), empty(7))
    R = GN.random_csr(rng, 40, 33, 4)
    cases["a_empty"] = (40, 33, empty(40), R)
    cases["b_empty"] = (40, 33, R, empty(40))
    cases["identical"] = (40, 33, R, (R[0], R[1], rng.random(len(R[1])) - 0.5))
    even = [np.sort(rng.choice(20, rng.integers(0, 6), replace=False)) * 2 for _ in range(30)]
    odd = [np.sort(rng.choice(20, rng.integers(0, 6), replace=False)) * 2 + 1 for _ in range(30)]
    cases["disjoint"] = (30, 40, with_pattern(rng, even), with_pattern(rng, odd))
    big = [np.sort(rng.choice(50, rng.integers(2, 12), replace=False)) for _ in range(35)]
    small = [np.sort(rng.choice(r, rng.integers(0, len(r)), replace=False)) for r in big]
    cases["a_in_b"] = (35, 50, with_pattern(rng, small), with_pattern(rng, big))
    cases["b_in_a"] = (35, 50, with_pattern(rng, big), with_pattern(rng, small))
    first_a = [np.concatenate(([0], 1 + 2 * np.sort(rng.choice(20, 4, replace=False)))) for _ in range(12)]
    first_b = [np.concatenate(([0], 2 + 2 * np.sort(rng.choice(19, 3, replace=False)))) for _ in range(12)]
    cases["match_first_col"] = (12, 41, with_pattern(rng, first_a), with_pattern(rng, first_b))
    last_a = [np.concatenate((2 * np.sort(rng.choice(20, 4, replace=False)), [40])) for _ in range(12)]
    last_b = [np.concatenate((1 + 2 * np.sort(rng.choice(19, 3, replace=False)), [40])) for _ in range(12)]
    cases["match_last_col"] = (12, 41, with_pattern(rng, last_a), with_pattern(rng, last_b))
    cases["unsorted"] = (50, 37, GN.random_csr(rng, 50, 37, 5, sort=False), GN.random_csr(rng, 50, 37, 5, sort=False))
    # (1e16 + 1) - 1e16 = 0 in the order of (V) and 1 in any order that takes B's term earlier: three terms on one entry
    D = csr_of_rows([([3, 1, 3], [1e16, 2.0, 1.0]), ([], []), ([0, 0, 0], [0.1, 0.2, 0.3])])
    E = csr_of_rows([([3, 4], [-1e16, 1.0]), ([2], [1.0]), ([5], [1.0])])
    F = csr_of_rows([([4, 3, 3], [1.0, -1e16, 5.0]), ([2, 2], [1.0, 2.0 ** -60]), ([0], [0.7])])
    cases["dup_a"] = (3, 6, D, E)
    cases["dup_b"] = (3, 6, E, D)
    cases["dup_both"] = (3, 6, D, F)
    for k in range(24):
        rows, cols = int(rng.integers(1, 60)), int(rng.integers(1, 70))
        for sort in (True, False):
            cases["random%d_%s" % (k, "sorted" if sort else "unsorted")] = (
                rows, cols, GN.random_csr(rng, rows, cols, int(rng.integers(1, 7)), sort=sort, empty_every=int(rng.integers(0, 4))),
                GN.random_csr(rng, rows, cols, int(rng.integers(1, 7)), sort=sort, empty_every=int(rng.integers(0, 5))))
    return cases


def scalars_of(name):
    """the case's (alpha, beta) from SCALARS, fixed by its name"""
    h = sum(ord(c) * (j + 1) for j, c in enumerate(name))
    return SCALARS[h % 5], SCALARS[(h // 5) % 5]


def special_values(A, B, seed):
    """the same patterns with -0.0, denormals, +-Inf and NaN sprinkled over the values"""
    rng = np.random.default_rng(seed)
    pool = np.array([-0.0, 0.0, 5e-324, -2.0 ** -1040, np.inf, -np.inf, np.nan, 1.0, -1.0, 1e308, 3.0])
    draw = lambda v: np.where(rng.random(len(v)) < 0.5, pool[rng.integers(0, len(pool), len(v))], v)
    return (A[0], A[1], draw(A[2])), (B[0], B[1], draw(B[2]))


# fl(alpha * a) + fl(beta * b) against a fused multiply-add: 3 * fl(1/3) = 1 - 2^-54 exactly, which rounds to 1, so the
# contract's value is 1 + -1 = +0.0, while fusing A's product, fma(3, fl(1/3), -1), gives -2^-54 and fusing B's,
# fma(-3, fl(1/3), 1), gives +2^-54: either contraction changes the bits
FMA_ALPHA, FMA_A, FMA_BETA, FMA_B = 3.0, 1.0 / 3.0, -3.0, 1.0 / 3.0
