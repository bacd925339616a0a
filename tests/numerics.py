"""Numerics references and checkers for the kernel tests (a plain helper module; tests import it like test_gpu_parity).

Everything here describes one operation, out = alpha * A * B + beta * C, with A an m x k CSR matrix given by
(rowptr, colidx, val) -- duplicates summed, rows in any order -- and B, C, out dense m x n / k x n arrays held here as
2-D numpy arrays (row r, column j), whatever order the kernel under test uses.  SpMV is n = 1; A^T x and A^T B are the
same operation on the host-built transpose (csc_of).  beta == 0 means C is not read: its values do not matter.

References and checkers, none of which shares code or summation order with the GPU kernels:

- grid_problem(): values on an exact grid (int_mantissa * 2^e) whose every partial sum, in any order and with or
  without FMA, is representable; the expected output comes from integer arithmetic and must be matched with ==.
- reference_dd(): alpha*A*B + beta*C in double-double (error-free TwoProd by Veltkamp splitting, TwoSum), for any
  finite data; its own error is below 2^-100 (|alpha| sum|a*b| + |beta c|).
- check_bound(): the rounding-error bound every correct summation order satisfies,
      |got - ref| <= gamma(L+2) (|alpha| sum_k |a_ik b_kj| + |beta| |c_ij|) + (L+2) eta,
  gamma(m) = m u / (1 - m u), L = stored entries of the row (duplicates counted), eta = the smallest subnormal.
- predict_class(): NaN / +Inf / -Inf / finite of each output when A, B or C hold Inf / NaN (finite data must not
  overflow; alpha != 0).  The class of an IEEE sum does not depend on its order."""
import math
from fractions import Fraction

import numpy as np

F64, F32 = np.dtype(np.float64), np.dtype(np.float32)
PREC = {F64: 53, F32: 24}                   # significand bits
EMIN = {F64: -1074, F32: -149}              # exponent of the smallest subnormal
EMAX = {F64: 1024, F32: 128}                # 2^EMAX overflows
CLASSES = ("finite", "nan", "+inf", "-inf")


def unit(dtype):
    return 2.0 ** -PREC[np.dtype(dtype)]


def eta(dtype):
    return 2.0 ** EMIN[np.dtype(dtype)]


def gamma(m, dtype):
    u = unit(dtype)
    m = np.asarray(m, np.float64)
    return m * u / (1.0 - m * u)


# ---------------------------------------------------------------------------------------------------------------------
# structure helpers
# ---------------------------------------------------------------------------------------------------------------------
def row_of_entries(rowptr):
    rp = np.asarray(rowptr, np.int64)
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


def row_lengths(rowptr):
    return np.diff(np.asarray(rowptr, np.int64))


def row_sums(rowptr, terms):
    """Per-row sums of terms[nnz, ...] in entry order (empty rows give 0)."""
    rp = np.asarray(rowptr, np.int64)
    out = np.zeros((len(rp) - 1,) + terms.shape[1:], terms.dtype)
    nz = rp[1:] > rp[:-1]
    if nz.any():
        out[nz] = np.add.reduceat(terms, rp[:-1][nz], axis=0)
    return out


def csc_of(rows, cols, rowptr, colidx, val=None):
    """A^T as CSR (colptr, rowidx, perm): a stable sort of colidx, so column c lists its entries in CSR order;
    perm[q] is the CSR position of transposed entry q (valT = val[perm])."""
    ci = np.asarray(colidx, np.int64)
    perm = np.argsort(ci, kind="stable")
    colptr = np.zeros(cols + 1, np.int64)
    np.cumsum(np.bincount(ci, minlength=cols), out=colptr[1:])
    rowidx = row_of_entries(rowptr)[perm]
    return colptr, rowidx, perm


def cancelling_pairs(rowptr, colidx, k):
    """(lead, follow, lone) entry positions: inside each row, entries whose columns share col // 2 are paired (lead[i]
    with follow[i]); the rest are lone.  With B rows 2i and 2i+1 equal, a[follow] = -a[lead] cancels each pair exactly."""
    rp = np.asarray(rowptr, np.int64)
    ci = np.asarray(colidx, np.int64)
    nnz = len(ci)
    key = row_of_entries(rp) * (k + 2) + ci // 2
    order = np.lexsort((np.arange(nnz), key))
    ks = key[order]
    first = np.r_[True, ks[1:] != ks[:-1]]
    grp = np.cumsum(first) - 1
    pos = np.arange(nnz) - np.flatnonzero(first)[grp]
    size = np.bincount(grp)[grp]
    paired = (pos % 2 == 1) | (pos + 1 < size)                # pos 2q with a partner at 2q+1
    return order[(pos % 2 == 0) & paired], order[pos % 2 == 1], order[~paired]


# ---------------------------------------------------------------------------------------------------------------------
# exact grids
# ---------------------------------------------------------------------------------------------------------------------
class GridProblem:
    """A, B, C, alpha, beta on an exact grid and the exact expected output (float arrays of dtype)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _signed_ints(rng, shape, bits):
    mag = rng.integers(1, 1 << bits, size=shape, dtype=np.int64) if bits > 0 else np.ones(shape, np.int64)
    return np.where(rng.random(shape) < 0.5, -mag, mag)


def grid_problem(rowptr, colidx, k, n, dtype=np.float64, scale=0, spread=0, cancel=False, alpha=None, beta=None,
                 bits=None, seed=0, scale_b=None):
    """Replace the values of the structure (rowptr, colidx; k columns) with an exact grid problem of width n.

    scale, scale_b: A values are int * 2^(scale + s), B values int * 2^(scale_b + s) (scale_b = scale when None), the
           products int * 2^(scale + scale_b + s'); -537 / -537 puts the products of fp64 at k * 2^-1074 (subnormal),
           -75 / -74 does it for fp32; 480 puts fp64 products near 2^1000, 50 fp32 products near 2^120.
    spread: per-entry exponent offsets s in [0, spread] (A gets ceil(spread/2) of them, B the rest), so the products
           of one row span spread + bits binades.
    cancel: entries of a row whose columns share col // 2 come in pairs (v, -v) of large magnitude and B rows 2i and
           2i+1 are equal, so each pair cancels exactly; the rest are 0, +-1, +-2 or +-3 at the finest unit of A.
    alpha, beta: +- powers of two or 0 (random ones when None).  bits: mantissa bits of A, B and C (the most that
           keep every partial sum below 2^p grid units when None).  Asserts the exactness precondition."""
    dt = np.dtype(dtype)
    p = PREC[dt]
    rng = np.random.default_rng(seed)
    rp = np.asarray(rowptr, np.int64)
    ci = np.asarray(colidx, np.int64)
    m, nnz = len(rp) - 1, len(ci)
    L = int(row_lengths(rp).max()) if m else 0
    sa = (spread + 1) // 2
    sb = spread - sa
    if alpha is None:
        alpha = float(rng.choice([-4.0, -1.0, 0.5, 1.0, 2.0]))
    if beta is None:
        beta = float(rng.choice([0.0, -2.0, 0.25, 1.0]))
    for s in (alpha, beta):
        assert s == 0 or math.frexp(abs(s))[0] == 0.5, "alpha / beta must be +-2^e or 0"
    ea = int(math.frexp(abs(alpha))[1]) - 1
    eb = int(math.frexp(abs(beta))[1]) - 1 if beta else 0
    if bits is None:                                  # L products of (bits + bits) bits, 2^spread apart, plus C
        head = p - 2 - spread - max(L, 1).bit_length() - (6 if cancel else 0)
        bits = max(1, min(20, head // 2))
    # A: integer mantissas and exponent offsets
    ia = _signed_ints(rng, nnz, bits)
    oa = rng.integers(0, sa + 1, nnz) if sa else np.zeros(nnz, np.int64)
    ib = _signed_ints(rng, (k, n), bits)
    ob = rng.integers(0, sb + 1, (k, n)) if sb else np.zeros((k, n), np.int64)
    if cancel:
        ib[1::2] = ib[0::2][: k // 2]
        ob[1::2] = ob[0::2][: k // 2]
        lead, follow, lone = cancelling_pairs(rp, ci, k)
        ia[lead] = _signed_ints(rng, len(lead), bits)
        oa[lead] = sa
        ia[follow] = -ia[lead]
        oa[follow] = oa[lead]
        ia[lone] = rng.integers(-3, 4, len(lone))
        oa[lone] = 0
    ic = _signed_ints(rng, (m, n), bits)
    oc = rng.integers(0, spread + 1, (m, n)) if spread else np.zeros((m, n), np.int64)
    if cancel:                                        # C small too: the outputs are a few grid units or exactly 0
        ic = rng.integers(-2, 3, (m, n))
        oc[:] = 0
    # exponents: A = ia 2^(scale+oa), B = ib 2^(scale+ob), C = ic 2^(ec + oc) with C on the scale of alpha * products
    if scale_b is None:
        scale_b = scale
    e_prod = scale + scale_b + ea
    ec = e_prod - eb
    e0 = min(e_prod, ec + eb) if beta else e_prod
    emin = EMIN[dt]
    for e in (scale, scale_b, scale + ea, scale_b + ea, e_prod - ea, e_prod, ec, e0):
        assert e >= emin, "grid unit 2^%d under the smallest subnormal 2^%d" % (e, emin)
    # the expected output in units of 2^e0 (int64); the worst partial sum in any order is the sum of magnitudes
    vals = ia[:, None] * ib[ci] << (oa[:, None] + ob[ci] + (e_prod - e0))
    sgn_a = -1 if alpha < 0 else 1
    exact = sgn_a * row_sums(rp, vals)
    worst = row_sums(rp, np.abs(vals))
    assert (np.abs(vals) < (1 << 62)).all()
    if beta:
        cterm = (ic << (oc + (ec + eb - e0))) * (-1 if beta < 0 else 1)
        exact = exact + cterm
        worst = worst + np.abs(cterm)
    wmax = int(worst.max()) if worst.size else 0
    assert wmax < (1 << p), "grid precondition: a partial sum reaches %d >= 2^%d grid units" % (wmax, p)
    # the unscaled product sum (before alpha) and every operand must stay finite
    top = max(e0 + max(wmax, 1).bit_length(), e_prod - ea + max(wmax, 1).bit_length(),
              scale + sa + bits, scale_b + sb + bits, ec + spread + bits)
    assert top < EMAX[dt], "grid precondition: values reach 2^%d" % top
    f = lambda i, e: np.ldexp(i.astype(np.float64), e).astype(dt)
    A = f(ia, scale + oa)
    B = f(ib, scale_b + ob)
    C = f(ic, ec + oc)
    out = f(exact, np.full(exact.shape, e0))
    assert (A.astype(np.float64) == np.ldexp(ia.astype(np.float64), scale + oa)).all()
    return GridProblem(A=A, B=B, C=C, alpha=alpha, beta=beta, expected=out, bits=bits, e0=e0, worst=wmax,
                       rowptr=rp, colidx=ci, k=k, n=n, dtype=dt)


def exact_fraction(rowptr, colidx, A, B, C, alpha, beta):
    """alpha*A*B + beta*C in rationals (the slow, obviously-right reference of the host tests)."""
    rp = np.asarray(rowptr, np.int64)
    m, n = len(rp) - 1, B.shape[1]
    out = [[Fraction(0)] * n for _ in range(m)]
    fa, fb = Fraction(float(alpha)), Fraction(float(beta))
    for i in range(m):
        for j in range(n):
            s = Fraction(0)
            for q in range(rp[i], rp[i + 1]):
                s += Fraction(float(A[q])) * Fraction(float(B[colidx[q], j]))
            out[i][j] = fa * s + (fb * Fraction(float(C[i, j])) if beta else 0)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# double-double reference
# ---------------------------------------------------------------------------------------------------------------------
_SPLIT = 134217729.0          # 2^27 + 1


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _fast_two_sum(a, b):
    s = a + b
    return s, b - (s - a)


def _split(a):
    c = _SPLIT * a
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _dd_add(h1, l1, h2, l2):
    s, e = _two_sum(h1, h2)
    return _fast_two_sum(s, e + (l1 + l2))


def _pow2_scale(x):
    """2^s that brings max|x| near 1 (0 for an all-zero x)."""
    mx = float(np.max(np.abs(x))) if np.size(x) else 0.0
    return 0 if mx == 0 or not np.isfinite(mx) else -math.frexp(mx)[1]


def _dd_row_sums(rowptr, hi, lo):
    """Per-row double-double sums of (hi, lo)[nnz, n]: a pairwise tree inside every row, all rows at once."""
    lens = row_lengths(rowptr)
    while lens.size and lens.max() > 1:
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
        row = np.repeat(np.arange(len(lens)), lens)
        pos = np.arange(len(row)) - starts[row]
        left = np.flatnonzero(pos % 2 == 0)
        has_right = pos[left] + 1 < lens[row[left]]
        right = left[has_right] + 1
        h, l = hi[left].copy(), lo[left].copy()
        h2, l2 = _dd_add(h[has_right], l[has_right], hi[right], lo[right])
        h[has_right], l[has_right] = h2, l2
        hi, lo, lens = h, l, (lens + 1) // 2
    m = len(lens)
    out_h = np.zeros((m,) + hi.shape[1:])
    out_l = np.zeros_like(out_h)
    nz = lens > 0
    out_h[nz], out_l[nz] = hi, lo
    return out_h, out_l


def reference_dd(rowptr, colidx, A, B, C, alpha, beta, chunk=64):
    """alpha*A*B + beta*C for finite data, as (hi, lo) float64 arrays with hi + lo within 2^-100 of the exact result
    relative to |alpha| sum|a b| + |beta c| (plus an absolute ~2^-1074 where the scaled parts underflow)."""
    rp = np.asarray(rowptr, np.int64)
    ci = np.asarray(colidx, np.int64)
    A = np.asarray(A, np.float64)
    B = np.asarray(B, np.float64)
    m, n = len(rp) - 1, B.shape[1]
    sa, sb = _pow2_scale(A), _pow2_scale(B)
    As, Bs = np.ldexp(A, sa), np.ldexp(B, sb)
    hi = np.zeros((m, n))
    lo = np.zeros((m, n))
    for j0 in range(0, n, chunk):
        Bg = Bs[ci, j0:j0 + chunk]
        ph, pl = _two_prod(As[:, None], Bg)
        sh, sl = _dd_row_sums(rp, ph, pl)
        # alpha * (sh + sl): alpha's two halves times the pair, error-free on the leading part
        p1, e1 = _two_prod(np.full_like(sh, alpha), sh)
        th, tl = _fast_two_sum(p1, e1 + alpha * sl)
        hi[:, j0:j0 + chunk] = np.ldexp(th, -(sa + sb))
        lo[:, j0:j0 + chunk] = np.ldexp(tl, -(sa + sb))
    if beta:
        Cd = np.asarray(C, np.float64)
        sc = _pow2_scale(Cd)
        ch, cl = _two_prod(np.full_like(Cd, beta), np.ldexp(Cd, sc))
        ch, cl = np.ldexp(ch, -sc), np.ldexp(cl, -sc)
        hi, lo = _dd_add(hi, lo, ch, cl)
    return hi, lo


def abs_sum(rowptr, colidx, A, B, C, alpha, beta, chunk=64):
    """|alpha| sum_k |a_ik b_kj| + |beta c_ij| in float64, rounded up so that it bounds the exact value."""
    rp = np.asarray(rowptr, np.int64)
    ci = np.asarray(colidx, np.int64)
    A = np.abs(np.asarray(A, np.float64))
    B = np.abs(np.asarray(B, np.float64))
    m, n = len(rp) - 1, B.shape[1]
    out = np.zeros((m, n))
    for j0 in range(0, n, chunk):
        out[:, j0:j0 + chunk] = row_sums(rp, A[:, None] * B[ci, j0:j0 + chunk])
    out *= abs(alpha)
    if beta:
        out += abs(beta) * np.abs(np.asarray(C, np.float64))
    L = row_lengths(rp)[:, None]
    return out * (1.0 + (L + 4) * 2.0 ** -52)


# ---------------------------------------------------------------------------------------------------------------------
# the bound
# ---------------------------------------------------------------------------------------------------------------------
class BoundResult:
    def __init__(self, ok, worst, where, count):
        self.ok, self.worst, self.where, self.count = ok, worst, where, count

    def __bool__(self):
        return self.ok

    def __repr__(self):
        return "bound %s: worst err/bound = %.3g at (row, col) = %s, %d outputs over" % (
            "ok" if self.ok else "FAILED", self.worst, self.where, self.count)


def bound(rowptr, colidx, A, B, C, alpha, beta, dtype):
    L = row_lengths(rowptr)[:, None]
    return gamma(L + 2, dtype) * abs_sum(rowptr, colidx, A, B, C, alpha, beta) + (L + 2) * eta(dtype)


def check_bound(got, ref, bnd, mask=None):
    """got: the kernel's output (m x n); ref: (hi, lo) or an array; bnd: bound(...).  mask: outputs to judge."""
    got = np.asarray(got, np.float64)
    if isinstance(ref, tuple):
        err = np.abs((got - ref[0]) - ref[1])
    else:
        err = np.abs(got - np.asarray(ref, np.float64))
    ratio = np.where(np.isfinite(err), err / np.maximum(bnd, np.finfo(np.float64).tiny), np.inf)
    if mask is not None:
        ratio = np.where(mask, ratio, 0.0)
    over = ratio > 1.0
    if ratio.size == 0:
        return BoundResult(True, 0.0, None, 0)
    w = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return BoundResult(not over.any(), float(ratio[w]), tuple(int(i) for i in w), int(over.sum()))


def check_general(got, rowptr, colidx, A, B, C, alpha, beta, dtype, mask=None):
    """Bound check of got against the double-double reference (A, B, C in the kernel's value type; for fp32 the scalars
    are those of the value type, as the typed entry points use them)."""
    dt = np.dtype(dtype)
    if dt == F32:
        alpha, beta = float(np.float32(alpha)), float(np.float32(beta))
    ref = reference_dd(rowptr, colidx, A, B, C, alpha, beta)
    return check_bound(got, ref, bound(rowptr, colidx, A, B, C, alpha, beta, dt), mask)


# ---------------------------------------------------------------------------------------------------------------------
# IEEE classes
# ---------------------------------------------------------------------------------------------------------------------
def _stand_in(x):
    """Non-finite values as they are, finite ones by their sign (0 stays 0): the products of these have the class of
    the real products (0 * Inf = NaN), and a sum's class follows from how many NaN, +Inf and -Inf terms it has."""
    x = np.asarray(x, np.float64)
    return np.where(np.isfinite(x), np.sign(x), x)


def predict_class(rowptr, colidx, A, B, C, alpha, beta):
    """0 finite, 1 NaN, 2 +Inf, 3 -Inf for every output (alpha != 0, finite scalars; beta == 0 ignores C)."""
    assert alpha != 0 and np.isfinite(alpha) and np.isfinite(beta)
    ci = np.asarray(colidx, np.int64)
    with np.errstate(invalid="ignore"):
        t = _stand_in(A)[:, None] * _stand_in(B)[ci] * np.sign(alpha)
        cnt = [row_sums(rowptr, np.isnan(t).astype(np.int64)), row_sums(rowptr, (t == np.inf).astype(np.int64)),
               row_sums(rowptr, (t == -np.inf).astype(np.int64))]
        if beta:
            c = np.asarray(C, np.float64) * np.sign(beta)
            cnt = [cnt[0] + np.isnan(c), cnt[1] + (c == np.inf), cnt[2] + (c == -np.inf)]
    nan = (cnt[0] > 0) | ((cnt[1] > 0) & (cnt[2] > 0))
    return np.where(nan, 1, np.where(cnt[1] > 0, 2, np.where(cnt[2] > 0, 3, 0)))


def class_of(x):
    x = np.asarray(x, np.float64)
    return np.where(np.isnan(x), 1, np.where(x == np.inf, 2, np.where(x == -np.inf, 3, 0)))


def check_classes(got, rowptr, colidx, A, B, C, alpha, beta):
    """(ok, message): the IEEE class of every output against predict_class."""
    want = predict_class(rowptr, colidx, A, B, C, alpha, beta)
    have = class_of(got)
    bad = np.argwhere(want != have)
    if len(bad) == 0:
        return True, ""
    r, c = bad[0]
    return False, "%d outputs in the wrong IEEE class; first (row %d, col %d): want %s, got %s (%r)" % (
        len(bad), r, c, CLASSES[want[r, c]], CLASSES[have[r, c]], got[r, c])


def finite_mask_inputs(rowptr, colidx, A, B, C, beta):
    """Outputs none of whose inputs is non-finite (the bound check judges those after an Inf / NaN test)."""
    ci = np.asarray(colidx, np.int64)
    bad = (~np.isfinite(np.asarray(A, np.float64)))[:, None] | (~np.isfinite(np.asarray(B, np.float64)))[ci]
    tainted = row_sums(rowptr, bad.astype(np.int64)) > 0
    if beta:
        tainted |= ~np.isfinite(np.asarray(C, np.float64))
    return ~tainted


def sanitized(A, B, C, beta):
    """Copies with every non-finite value replaced by 0 (for the bound reference of the untainted outputs)."""
    z = lambda x: np.where(np.isfinite(x), x, 0).astype(np.asarray(x).dtype)
    return z(A), z(B), (z(C) if beta else C)


# ---------------------------------------------------------------------------------------------------------------------
# general data
# ---------------------------------------------------------------------------------------------------------------------
def log_uniform(rng, shape, binades, dtype=np.float64, center=0):
    """Signed values whose exponents are uniform over `binades` binades around 2^center."""
    e = rng.uniform(center - binades / 2, center + binades / 2, shape)
    v = np.exp2(e) * np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    return v.astype(dtype)
