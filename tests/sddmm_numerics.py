"""Numerics references and checkers for SDDMM (a plain helper module, like numerics.py, which it builds on).

The operation: out[e] = alpha * <X[row(e), :], Y[col(e), :]> + beta * old[e] for every stored entry e of a CSR pattern
(rowptr, colidx); X is rows x k, Y is cols x k, both held here as 2-D numpy arrays.  beta == 0 means old is not read.
Nothing here shares code or summation order with the GPU kernels:

- reference_dd(): the result in double-double (error-free TwoProd / TwoSum from numerics.py), for any finite data.
- grid_problem(): operands on an exact grid (integer mantissa * 2^e) such that every partial sum of a dot product, in
  any order and with or without FMA, is representable; the expected output comes from integer arithmetic and must be
  matched with ==.
- bound(): |got - ref| <= gamma(k + 2) * (|alpha| sum_j |x_j y_j| + |beta| |old|) + (k + 2) * eta.  At most k roundings
  in the dot product (k - 1 adds and the products, fused or not, are covered by k), one for alpha, one for beta * old or
  the final add; it holds for every summation order, so it carries no measured margin.
- predict_class(): NaN / +Inf / -Inf / finite of each output from the classes of the operands."""
import math
from fractions import Fraction

import numpy as np

from numerics import _fast_two_sum, _pow2_scale, _two_prod, _two_sum, class_of, eta, gamma, log_uniform, row_of_entries  # noqa: F401

F64 = np.float64


def entry_rows(rowptr, colidx):
    return row_of_entries(rowptr), np.asarray(colidx, np.int64)


def _dd_add(h1, l1, h2, l2):
    s, e = _two_sum(h1, h2)
    return _fast_two_sum(s, e + (l1 + l2))


def reference_dd(rowptr, colidx, X, Y, old, alpha, beta, chunk=1 << 16):
    """(hi, lo) float64 arrays of nnz entries, hi + lo within ~2^-100 (relative to |alpha| sum |x y| + |beta old|) of
    alpha * <x, y> + beta * old.  The k products are added one at a time in double-double."""
    r, c = entry_rows(rowptr, colidx)
    X = np.asarray(X, F64)
    Y = np.asarray(Y, F64)
    nnz, k = len(c), X.shape[1]
    sx, sy = _pow2_scale(X), _pow2_scale(Y)
    Xs, Ys = np.ldexp(X, sx), np.ldexp(Y, sy)
    hi, lo = np.zeros(nnz), np.zeros(nnz)
    for e0 in range(0, nnz, chunk):
        rr, cc = r[e0:e0 + chunk], c[e0:e0 + chunk]
        h, l = np.zeros(len(rr)), np.zeros(len(rr))
        for j in range(k):
            ph, pl = _two_prod(Xs[rr, j], Ys[cc, j])
            h, l = _dd_add(h, l, ph, pl)
        p1, e1 = _two_prod(np.full_like(h, alpha), h)
        th, tl = _fast_two_sum(p1, e1 + alpha * l)
        hi[e0:e0 + chunk] = np.ldexp(th, -(sx + sy))
        lo[e0:e0 + chunk] = np.ldexp(tl, -(sx + sy))
    if beta:
        od = np.asarray(old, F64)
        so = _pow2_scale(od)
        ch, cl = _two_prod(np.full_like(od, beta), np.ldexp(od, so))
        hi, lo = _dd_add(hi, lo, np.ldexp(ch, -so), np.ldexp(cl, -so))
    return hi, lo


def abs_sum(rowptr, colidx, X, Y, old, alpha, beta, chunk=1 << 16):
    """|alpha| sum_j |x_j y_j| + |beta old| per entry in float64, rounded up so that it bounds the exact value."""
    r, c = entry_rows(rowptr, colidx)
    X = np.abs(np.asarray(X, F64))
    Y = np.abs(np.asarray(Y, F64))
    nnz, k = len(c), X.shape[1]
    out = np.zeros(nnz)
    for e0 in range(0, nnz, chunk):
        out[e0:e0 + chunk] = (X[r[e0:e0 + chunk]] * Y[c[e0:e0 + chunk]]).sum(axis=1)
    out *= abs(alpha)
    if beta:
        out += abs(beta) * np.abs(np.asarray(old, F64))
    return out * (1.0 + (k + 4) * 2.0 ** -52)


def bound(rowptr, colidx, X, Y, old, alpha, beta):
    k = np.asarray(X).shape[1]
    return gamma(k + 2, F64) * abs_sum(rowptr, colidx, X, Y, old, alpha, beta) + (k + 2) * eta(F64)


def check_bound(got, ref, bnd):
    """(ok, worst err / bound, entry of the worst, entries over): every entry is judged."""
    got = np.asarray(got, F64)
    err = np.abs((got - ref[0]) - ref[1]) if isinstance(ref, tuple) else np.abs(got - np.asarray(ref, F64))
    if err.size == 0:
        return True, 0.0, None, 0
    ratio = np.where(np.isfinite(err), err / np.maximum(bnd, np.finfo(F64).tiny), np.inf)
    w = int(np.argmax(ratio))
    return bool((ratio <= 1.0).all()), float(ratio[w]), w, int((ratio > 1.0).sum())


def check_general(got, rowptr, colidx, X, Y, old, alpha, beta):
    ref = reference_dd(rowptr, colidx, X, Y, old, alpha, beta)
    return check_bound(got, ref, bound(rowptr, colidx, X, Y, old, alpha, beta))


def exact_fraction(rowptr, colidx, X, Y, old, alpha, beta):
    """The result in rationals (the slow, obviously-right reference of the host tests): a list of Fractions."""
    r, c = entry_rows(rowptr, colidx)
    fa, fb = Fraction(float(alpha)), Fraction(float(beta))
    out = []
    for e in range(len(c)):
        s = sum((Fraction(float(a)) * Fraction(float(b)) for a, b in zip(X[r[e]], Y[c[e]])), Fraction(0))
        out.append(fa * s + (fb * Fraction(float(old[e])) if beta else 0))
    return out


class GridProblem:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _signed_ints(rng, shape, bits):
    mag = rng.integers(1, 1 << bits, size=shape, dtype=np.int64)
    return np.where(rng.random(shape) < 0.5, -mag, mag)


def grid_problem(rowptr, colidx, rows, cols, k, alpha, beta, spread=6, seed=0):
    """X, Y, old on an exact grid and the exact expected output.  X = ix * 2^ox, Y = iy * 2^oy with `bits`-bit integer
    mantissas and exponent offsets in [0, spread / 2]; every product is an integer below 2^(2 bits + spread), a sum of k
    of them stays below 2^53 grid units in any order, so neither the adds nor an FMA ever round.  alpha, beta: +-2^e or 0."""
    for s in (alpha, beta):
        assert s == 0 or math.frexp(abs(s))[0] == 0.5, "alpha / beta must be +-2^e or 0"
    rng = np.random.default_rng(seed)
    r, c = entry_rows(rowptr, colidx)
    nnz = len(c)
    sa = spread // 2
    bits = max(1, min(20, (53 - 3 - 2 * sa - max(k, 1).bit_length()) // 2))
    ix, iy = _signed_ints(rng, (rows, k), bits), _signed_ints(rng, (cols, k), bits)
    ox = rng.integers(0, sa + 1, (rows, k))
    oy = rng.integers(0, sa + 1, (cols, k))
    io = _signed_ints(rng, nnz, bits)
    ea = int(math.frexp(abs(alpha))[1]) - 1 if alpha else 0
    eb = int(math.frexp(abs(beta))[1]) - 1 if beta else 0
    # old = io * 2^(ea - eb): beta * old and alpha * products share the unit 2^ea
    dot = np.zeros(nnz, np.int64)
    worst = np.zeros(nnz, np.int64)
    for j in range(k):
        t = (ix[r, j] * iy[c, j]) << (ox[r, j] + oy[c, j])
        dot += t
        worst += np.abs(t)
    exact = dot * (0 if alpha == 0 else (-1 if alpha < 0 else 1))
    if beta:
        exact = exact + io * (-1 if beta < 0 else 1)
        worst = worst + np.abs(io)
    assert nnz == 0 or int(worst.max()) < (1 << 53), "grid precondition: a partial sum leaves the 53-bit grid"
    f = lambda i, e: np.ldexp(i.astype(F64), e)
    return GridProblem(X=f(ix, ox), Y=f(iy, oy), old=f(io, np.full(nnz, ea - eb)), alpha=float(alpha), beta=float(beta),
                       expected=f(exact, np.full(nnz, ea)), bits=bits, k=k)


def _stand_in(x):
    x = np.asarray(x, F64)
    return np.where(np.isfinite(x), np.sign(x), x)


def predict_class(rowptr, colidx, X, Y, old, alpha, beta):
    """0 finite, 1 NaN, 2 +Inf, 3 -Inf per entry (alpha != 0 and finite, beta finite; finite data must not overflow;
    beta == 0 ignores old).  The class of an IEEE sum does not depend on its order."""
    assert alpha != 0 and np.isfinite(alpha) and np.isfinite(beta)
    r, c = entry_rows(rowptr, colidx)
    with np.errstate(invalid="ignore"):
        t = _stand_in(X)[r] * _stand_in(Y)[c] * np.sign(alpha)
        cnt = [np.isnan(t).sum(axis=1), (t == np.inf).sum(axis=1), (t == -np.inf).sum(axis=1)]
        if beta:
            o = np.asarray(old, F64) * np.sign(beta)
            cnt = [cnt[0] + np.isnan(o), cnt[1] + (o == np.inf), cnt[2] + (o == -np.inf)]
    nan = (cnt[0] > 0) | ((cnt[1] > 0) & (cnt[2] > 0))
    return np.where(nan, 1, np.where(cnt[1] > 0, 2, np.where(cnt[2] > 0, 3, 0)))
