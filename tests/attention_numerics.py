"""Helpers of the fused-attention tests (test_attention_host.py, test_gpu_attention.py): the three patterns, the operands,
the exact reference of a row's weighted sum and the bound a computed one has to meet.

The fused kernels promise the composition's bits for the probabilities P and the score gradients dS (contract B), so the
only new floating-point work to judge is O[i, c] = sum_e P[e] V[c(e), c] and dQ[i, c] = sum_e dS[e] K[c(e), c].  Both are
dot products of length L (the row's length) over GIVEN weights; the reference is the exact rational value of that sum
for the weights the GPU itself produced, and the bound is the standard one for a dot product summed in any order,

    |got - ref| <= gamma(L + 2 + ceil(L / 4096)) * sum_e |w[e] Y[c(e), c]| + (L + 2) * 2^-1074,   gamma(m) = m u / (1 - m u),

u = 2^-53: tests/numerics.py's SpMM bound (L products and additions, two spare roundings) with one more addition for each
supercell partial a long row folds.  It holds for every order of the fmas and carries no measured margin."""
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)
ETA = Fraction(1, 2 ** 1074)
SUPER = 4096
WIDTHS = [(1, 1), (5, 3), (8, 8), (33, 17), (64, 64), (64, 16), (16, 128), (128, 128)]
SCALES = (1.0, 0.125, -0.3)
EDGE_COLS = 600


def gamma(m):
    return m * U / (1 - m * U)


def bound_factor(L):
    return gamma(L + 2 + -(-L // SUPER))


# ---- patterns ------------------------------------------------------------------------------------------------------
def rowptr_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def edge_lengths():
    from test_gpu_softmax import EDGES
    return [0, 1, 2] + list(EDGES)


def edges_pattern(seed=0):
    """one row per length in 0, 1, 2 and the softmax tests' EDGES, columns drawn with repeats from 600"""
    lens = edge_lengths()
    rp = rowptr_of(lens)
    ci = np.random.default_rng(seed).integers(0, EDGE_COLS, int(rp[-1])).astype(np.int32)
    return len(lens), EDGE_COLS, rp, ci


def small_pattern():
    from test_gpu_autograd import small_pattern as sp
    return sp()


def big_pattern():
    from sblas_amd import synth
    rp, ci, _ = synth.random_csr(20000, 20000, 8, seed=5, empty_every=11, long_row=(17, 9000))
    return 20000, 20000, np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)


PATTERNS = {"small": small_pattern, "edges": edges_pattern, "big": big_pattern}
_cache = {}


def pattern(name):
    """(rows, cols, rowptr, colidx), made once and shared; nobody writes to it"""
    if name not in _cache:
        rows, cols, rp, ci = PATTERNS[name]()
        rp.setflags(write=False), ci.setflags(write=False)
        _cache[name] = (rows, cols, rp, ci)
    return _cache[name]


def operands(rows, cols, d, dv, seed=0):
    """Q, K, V, dO: uniform in (-1, 1); scores of a few units at most, so no exp underflows to zero"""
    rng = np.random.default_rng(1000 * d + dv + seed)
    u = lambda *shape: rng.uniform(-1.0, 1.0, shape)
    return u(rows, d), u(cols, d), u(cols, dv), u(rows, dv)


def sample_rows(rp, count=6, seed=0):
    """a few rows, always with the longest, one of the shortest non-empty ones and an empty one when there is one"""
    lens = np.diff(np.asarray(rp, np.int64))
    rng = np.random.default_rng(seed)
    rows = set(int(r) for r in rng.choice(len(lens), min(count, len(lens)), replace=False))
    rows.add(int(lens.argmax()))
    if (lens > 0).any():
        rows.add(int(np.flatnonzero(lens > 0)[lens[lens > 0].argmin()]))
    if (lens == 0).any():
        rows.add(int(np.flatnonzero(lens == 0)[0]))
    return sorted(rows)


# ---- the exact sum -------------------------------------------------------------------------------------------------
def _int_parts(x):
    """x = m * 2^e with m an integer (as Python ints) -- exact for every finite double"""
    m, e = np.frexp(np.asarray(x, np.float64))
    return np.ldexp(m, 53).astype(np.int64).astype(object), e.astype(np.int64) - 53


def exact_weighted_sum(w, Y):
    """(sum_e w[e] Y[e, c], sum_e |w[e] Y[e, c]|) for every column c as Fractions: integer arithmetic, no rounding"""
    w, Y = np.asarray(w, np.float64), np.asarray(Y, np.float64)
    n = Y.shape[1]
    if len(w) == 0:
        return [Fraction(0)] * n, [Fraction(0)] * n
    assert np.isfinite(w).all() and np.isfinite(Y).all()
    mw, ew = _int_parts(w)
    my, ey = _int_parts(Y)
    e = ew[:, None] + ey
    emin = int(e.min())
    terms = np.left_shift(mw[:, None] * my, (e - emin).astype(object))
    unit = Fraction(2) ** emin
    return [Fraction(int(v)) * unit for v in terms.sum(axis=0)], [Fraction(int(v)) * unit for v in np.abs(terms).sum(axis=0)]


def check_rows(got, rp, ci, w, Y, rows):
    """got[i, :] against the exact sum_e w[e] Y[ci[e], :] of the rows `rows`, within the bound of the module docstring.
    Returns dict(ok, worst = the largest error / bound, outputs judged, where)."""
    rp = np.asarray(rp, np.int64)
    worst, where, judged = 0.0, None, 0
    for r in rows:
        lo, hi = int(rp[r]), int(rp[r + 1])
        L = hi - lo
        ref, mag = exact_weighted_sum(w[lo:hi], Y[np.asarray(ci[lo:hi], np.int64)])
        f = bound_factor(L)
        for c in range(Y.shape[1]):
            g = float(got[r, c])
            if not np.isfinite(g):
                return dict(ok=False, worst=float("inf"), outputs=judged, where=(r, c))
            bnd = f * mag[c] + (L + 2) * ETA
            ratio = float(abs(Fraction(g) - ref[c]) / bnd)
            judged += 1
            if ratio > worst:
                worst, where = ratio, (r, c)
    return dict(ok=worst <= 1.0, worst=worst, outputs=judged, where=where)


def numpy_rows(rp, ci, w, Y, rows_total):
    """the same sums in plain float64, one row at a time"""
    rp = np.asarray(rp, np.int64)
    out = np.zeros((rows_total, Y.shape[1]))
    for r in range(rows_total):
        lo, hi = rp[r], rp[r + 1]
        if hi > lo:
            out[r] = (w[lo:hi, None] * Y[np.asarray(ci[lo:hi], np.int64)]).sum(axis=0)
    return out


# ---- the composition in numpy (host tests; the GPU tests compare with the library's own composition) ---------------
def numpy_attention(rp, ci, Q, K, V, scale):
    """(O, P, row_max, row_sum) by the textbook formulas in float64"""
    rp = np.asarray(rp, np.int64)
    rows = len(rp) - 1
    r = np.repeat(np.arange(rows), np.diff(rp))
    t = scale * np.einsum("ek,ek->e", Q[r], K[np.asarray(ci, np.int64)])
    m = np.full(rows, -np.inf)
    np.maximum.at(m, r, t)
    e = np.exp(t - m[r])
    z = np.zeros(rows)
    np.add.at(z, r, e)
    P = e / z[r]
    return numpy_rows(rp, ci, P, V, rows), P, m, z


def classes(x):
    """0 finite non-zero, 1 NaN, 2 +Inf, 3 -Inf, 4 zero"""
    x = np.asarray(x, np.float64)
    return np.where(np.isnan(x), 1, np.where(x == np.inf, 2, np.where(x == -np.inf, 3, np.where(x == 0, 4, 0))))
