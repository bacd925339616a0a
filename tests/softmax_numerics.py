"""Numerics references, bounds, class rules and test inputs for the row-wise softmax on a CSR pattern and its backward (a
plain helper module, like sddmm_numerics.py).  Nothing here shares code with the GPU kernels.

The operation, per row with stored entries e in stored order:
    forward    t[e] = scale * x[e],  m = max t,  s = sum exp(t[e] - m),  out[e] = exp(t[e] - m) / s
    backward   D = sum p[e] dp[e],   dx[e] = scale * p[e] * (dp[e] - D)

References.  forward_reference() / backward_reference() evaluate these in `decimal` at PREC = 60 digits (Decimal.exp is
correctly rounded at that precision), so they are exact for every purpose of a 2^-53 comparison.  The forward reference
starts from t = fl(scale * x), the one correctly rounded IEEE product every implementation forms (numpy forms the same
number): softmax is not well conditioned with respect to a RELATIVE change of t (exp(t (1 + delta)) moves by |t| delta),
so a bound that counted that rounding would grow with |t| and say nothing about the kernel.

Forward bound (u = 2^-53, c_exp = 3 ulp = 6 u relative: the OpenCL full-profile limit for double exp, which the ROCm
device library documents it meets).  With d_i = t_i - m <= 0 (m is exact: a max rounds nothing):
    fl(d_i) = d_i (1 + e1), |e1| <= u, so exp(fl(d_i)) = exp(d_i) exp(d_i e1): a relative change of at most
        exp(|d_i| u) - 1;
    the computed leaf is exp(fl(d_i)) (1 + e2), |e2| <= 6 u:       leaf_i = exp(d_i) (1 + eta_i),
        |eta_i| <= (6 + |d_i|) u + second order;
    any summation of L non-negative leaves, in any order:            s^ = sum leaf_i (1 + th_i), |th_i| <= gamma(L - 1),
        so s^ = s (1 + sigma) with |sigma| <= sum_i p_i |eta_i| + gamma(L - 1) <= (6 + Dbar) u + (L - 1) u + second
        order, where p_i = exp(d_i) / s and Dbar = sum_i p_i |d_i| (the terms that contribute to the sum, by weight);
    the division rounds once more.
Together    |out_i - p_i| <= p_i * (6 + |d_i| + 6 + Dbar + (L - 1) + 1) u * (1 + second order)
and the bound used is  p_i * (13 + |d_i| + Dbar + L) * u * SLACK  with SLACK = 1.001 for the second-order terms (the
first-order sum stays below 2^-20 for L < 2^32, so they are below 2^-20 of it) and for Dbar being formed in floating
point.  It holds for every summation order and carries no measured margin.
Underflow (absolute form): a leaf in the subnormal range is within 3 subnormal ulps = 3 * 2^-1074 of exp(fl(d_i)); s^ >= 1
* (1 - tiny) because the max entry's leaf is exp(0) = 1; the quotient rounds to within 2^-1075 when it is subnormal.  So
    |out_i - p_i| <= relative bound + 4 * 2^-1074.
Row sums: sum_i out_i - 1 = sum_i (out_i - p_i), so |exact sum of the outputs - 1| <= sum_i bound_i.

Backward bound.  p and dp are the given numbers.  D^ = sum fl(p_j dp_j) in any order: |D^ - D| <= gamma(L) A with
A = sum |p_j dp_j|.  g^ = fl(dp_i - D^), q^ = fl(scale p_i), dx^ = fl(q^ g^): with g = dp_i - D
    |dx^ - dx| <= |scale p_i| * (3 u |g| + (L + 1) u A) * SLACK + (L + 4) * 2^-1074 * max(1, |scale p_i|)
(three roundings on the g path, the sum's error carried through, products that underflow absorbed by the last term).  g can
cancel to far below A, so the bound is absolute in A, as a dot product's is.

Classes (the rules of torch.softmax on each row): predict_class()."""
import math
from decimal import Decimal, localcontext

import numpy as np

from numerics import row_of_entries  # noqa: F401

PREC = 60
U = 2.0 ** -53
C_EXP = 6.0            # 3 ulp of the result, relative to it at worst: 3 * 2^-52
SLACK = 1.001
TINY = 2.0 ** -1074
SAMPLE_ROWS = 24       # whole rows checked against the Decimal reference on the large inputs (plus the two named ones)

FINITE, NAN, ZERO = 0, 1, 2


def _dec(v):
    return Decimal(float(v))


# ---- references ----------------------------------------------------------------------------------------------------
def forward_row_decimal(t):
    """softmax of the numbers t (Decimals or floats) in Decimal: (p, d) lists"""
    with localcontext() as ctx:
        ctx.prec = PREC
        t = [v if isinstance(v, Decimal) else _dec(v) for v in t]
        if not t:
            return [], []
        m = max(t)
        d = [v - m for v in t]
        e = [v.exp() for v in d]
        s = sum(e, Decimal(0))
        return [v / s for v in e], d


def backward_row_decimal(p, dp, scale):
    with localcontext() as ctx:
        ctx.prec = PREC
        p = [v if isinstance(v, Decimal) else _dec(v) for v in p]
        dp = [v if isinstance(v, Decimal) else _dec(v) for v in dp]
        D = sum((a * b for a, b in zip(p, dp)), Decimal(0))
        sc = scale if isinstance(scale, Decimal) else _dec(scale)
        return [sc * a * (b - D) for a, b in zip(p, dp)], D


def scaled(x, scale):
    """t = fl(scale * x): the correctly rounded product"""
    return np.float64(scale) * np.asarray(x, np.float64)


def forward_reference(rowptr, x, scale, rows=None):
    """{row: (p, d)} with Decimal lists per row, for the rows asked (all by default)"""
    t = scaled(x, scale)
    rows = range(len(rowptr) - 1) if rows is None else rows
    return {int(r): forward_row_decimal(t[rowptr[r]:rowptr[r + 1]]) for r in rows}


def backward_reference(rowptr, p, dp, scale, rows=None):
    rows = range(len(rowptr) - 1) if rows is None else rows
    return {int(r): backward_row_decimal(p[rowptr[r]:rowptr[r + 1]], dp[rowptr[r]:rowptr[r + 1]], scale) for r in rows}


# ---- bounds --------------------------------------------------------------------------------------------------------
def forward_bound_row(p, d):
    """float bounds on |out_i - p_i| for one row (relative form plus the underflow term), from the reference's p, d"""
    L = len(p)
    pf = np.array([float(v) for v in p])
    ad = np.array([abs(float(v)) for v in d])
    dbar = float((pf * ad).sum()) if L else 0.0
    rel = (2 * C_EXP + 1 + ad + dbar + L) * U * SLACK
    return rel, pf * rel + 4 * TINY


def check_forward(got, rowptr, x, scale, rows=None, absolute=False):
    """-> dict(ok, worst (err / bound), where (row, index), worst_u (largest relative error in units of u, over entries
    whose reference is normal), sum_worst (|exact row sum - 1| / its bound), entries).  absolute=False: the relative form
    alone (no entry is excused by the underflow term); absolute=True adds 4 * 2^-1074 per entry."""
    ref = forward_reference(rowptr, x, scale, rows)
    worst, where, worst_u, sum_worst, n = 0.0, None, 0.0, 0.0, 0
    with localcontext() as ctx:
        ctx.prec = PREC
        for r, (p, d) in ref.items():
            g = got[rowptr[r]:rowptr[r + 1]]
            rel, bnd_abs = forward_bound_row(p, d)
            total_bound = 0.0
            for i, (pi, gi) in enumerate(zip(p, g)):
                if not math.isfinite(gi):
                    return dict(ok=False, worst=float("inf"), where=(r, i), worst_u=float("inf"), sum_worst=float("inf"), entries=n)
                err = float(abs(_dec(gi) - pi))
                bnd = bnd_abs[i] if absolute else float(pi) * rel[i]
                total_bound += bnd
                ratio = err / bnd if bnd > 0 else (0.0 if err == 0 else float("inf"))
                if ratio > worst:
                    worst, where = ratio, (r, i)
                if float(pi) >= 2.0 ** -1022:
                    worst_u = max(worst_u, err / float(pi) / U)
                n += 1
            if len(p):
                ssum = float(abs(sum((_dec(v) for v in g), Decimal(0)) - 1))
                sum_worst = max(sum_worst, ssum / total_bound)
    return dict(ok=worst <= 1.0 and sum_worst <= 1.0, worst=worst, where=where, worst_u=worst_u, sum_worst=sum_worst, entries=n)


def check_backward(got, rowptr, p, dp, scale, rows=None):
    """-> dict(ok, worst (err / bound), where, entries)"""
    ref = backward_reference(rowptr, p, dp, scale, rows)
    worst, where, n = 0.0, None, 0
    for r, (dx, D) in ref.items():
        lo, hi = rowptr[r], rowptr[r + 1]
        L = hi - lo
        pr, dpr, g = p[lo:hi], dp[lo:hi], got[lo:hi]
        A = float(np.abs(pr * dpr).sum()) * (1 + L * U) + L * TINY
        Df = float(D)
        for i in range(L):
            if not math.isfinite(g[i]):
                return dict(ok=False, worst=float("inf"), where=(r, i), entries=n)
            sp = abs(scale * pr[i]) * (1 + U)
            gabs = abs(dpr[i] - Df) + abs(Df) * 4 * U + 4 * TINY
            bnd = sp * (3 * U * gabs + (L + 1) * U * A) * SLACK + (L + 4) * TINY * max(1.0, sp)
            with localcontext() as ctx:
                ctx.prec = PREC
                err = float(abs(_dec(g[i]) - dx[i]))
            ratio = err / bnd if bnd > 0 else (0.0 if err == 0 else float("inf"))
            if ratio > worst:
                worst, where = ratio, (r, i)
            n += 1
    return dict(ok=worst <= 1.0, worst=worst, where=where, entries=n)


# ---- plain numpy evaluations (what a careful user would write; used to test the references and the inputs) ------------
def numpy_forward(rowptr, x, scale):
    t = scaled(x, scale)
    lens = np.diff(np.asarray(rowptr, np.int64))
    if len(t) == 0:
        return t.copy()
    starts = np.asarray(rowptr[:-1], np.int64)[lens > 0]
    e = np.exp(t - np.repeat(np.maximum.reduceat(t, starts), lens[lens > 0]))
    return e / np.repeat(np.add.reduceat(e, starts), lens[lens > 0])


def numpy_backward(rowptr, p, dp, scale):
    out = np.empty_like(p)
    for r in range(len(rowptr) - 1):
        lo, hi = rowptr[r], rowptr[r + 1]
        if hi > lo:
            D = (p[lo:hi] * dp[lo:hi]).sum()
            out[lo:hi] = (scale * p[lo:hi]) * (dp[lo:hi] - D)
    return out


def _fold64(v):
    """the butterfly over groups of 64 consecutive numbers (len(v) a multiple of 64): v += v[l ^ 1], .. v += v[l ^ 32] adds
    neighbours, then neighbouring pairs, ...: six rounds of pairwise sums (addition commutes, so which side a partner is
    on does not matter)"""
    v = v.reshape(-1, 64)
    for _ in range(6):
        v = v[:, 0::2] + v[:, 1::2]
    return v.reshape(-1)


def ordered_row_sum(leaves):
    """the sum of a row's leaves in the order include/sblas_hip.h documents: cells of 64 (absent +0) folded by the
    butterfly, supercells of 64 cells folded the same way, supercell sums added left to right from +0"""
    L = len(leaves)
    cells = _fold64(np.concatenate([leaves, np.zeros(-L % 64)]))
    supers = _fold64(np.concatenate([cells, np.zeros(-len(cells) % 64)]))
    s = np.float64(0.0)
    for v in supers:
        s = s + v
    return s


def emulate_backward(rowptr, p, dp, scale):
    """the backward in IEEE double in the documented order: every operation in it is a correctly rounded +, -, * (the
    leaf fma(p, dp, +0) is the rounded product), so the kernel's output must equal this bit for bit"""
    out = np.empty_like(p)
    for r in range(len(rowptr) - 1):
        lo, hi = rowptr[r], rowptr[r + 1]
        if hi > lo:
            D = ordered_row_sum(p[lo:hi] * dp[lo:hi] + 0.0)
            out[lo:hi] = (np.float64(scale) * p[lo:hi]) * (dp[lo:hi] - D)
    return out


# ---- classes -------------------------------------------------------------------------------------------------------
def predict_class(rowptr, x, scale):
    """per entry: NAN (the row holds a NaN after scaling, its max is +Inf, or it holds -Inf only), ZERO (exactly +0: a
    -Inf entry of a row with a finite max), FINITE (a number in [0, 1]; exp may underflow to 0)"""
    with np.errstate(invalid="ignore"):
        t = scaled(x, scale)                       # 0 * Inf = NaN here as on the device
    out = np.full(len(t), FINITE, np.int64)
    for r in range(len(rowptr) - 1):
        lo, hi = rowptr[r], rowptr[r + 1]
        if hi == lo:
            continue
        row = t[lo:hi]
        if np.isnan(row).any() or row.max() == np.inf or row.max() == -np.inf:
            out[lo:hi] = NAN
        else:
            out[lo:hi][row == -np.inf] = ZERO
    return out


def class_mismatches(want, got):
    """indices where got is not of the class wanted"""
    got = np.asarray(got, np.float64)
    isnan = np.isnan(got)
    ok = np.where(want == NAN, isnan,
                  np.where(want == ZERO, (got == 0.0) & ~np.signbit(got), ~isnan & (got >= 0.0) & (got <= 1.0)))
    return np.flatnonzero(~ok)


# ---- inputs of the GPU tests (tests/test_softmax_host.py checks on the CPU that they meet the tests' conditions) --------
def small_pattern():
    """5 rows: unsorted order is meaningless here (no colidx), so: a duplicate value pair (row 0), an empty row (1), a
    one-entry row (3)"""
    rp = np.array([0, 3, 3, 5, 6, 9], np.int32)
    x = np.array([0.5, -1.25, 0.5, 2.0, -3.0, 7.0, 0.125, 0.25, -0.375])
    return rp, x


_patterns = {}


def pattern(name):
    """rowptr (int32 numpy) of a named test input; the large ones end in a one-entry row"""
    if name in _patterns:
        return _patterns[name]
    from sblas_amd import synth
    if name == "small":
        rp = small_pattern()[0]
    elif name == "mixed":          # every path: empty rows, lengths 1 .. 9000, a row of 20 000
        lens = [0, 1, 2, 8, 9, 0, 63, 64, 65, 130, 511, 512, 513, 0, 0, 4095, 4096, 4097, 7, 8191, 8192, 8193, 9000, 3, 20000, 1, 5]
        rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    elif name == "ash85":
        import os
        import sblas_amd as S
        rp = S.read_mtx(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ash85.mtx"))[4]
    elif name == "banded":         # 20 000 rows of 5
        rp = synth.banded(20000, 5, 40)[0].copy()
        rp[-1] = rp[-2] + 1
    elif name == "powerlaw":       # a row of 120 000 entries among rows of one to three
        rp = synth.powerlaw(150000, max_len=120000)[0]
    elif name == "nd24k_slice":    # 500 rows of 399
        rp = synth.nd24k_like(0.05)[1][0][:501].copy()
        rp[-1] = rp[-2] + 1
    else:
        raise KeyError(name)
    _patterns[name] = np.asarray(rp, np.int32)
    return _patterns[name]


def scores(rowptr, seed, scale=1.0, spread=60.0):
    """x with scale * x spread over at most `spread` inside every row, around a row centre drawn from +-200 / |scale|"""
    rng = np.random.default_rng(seed)
    lens = np.diff(rowptr.astype(np.int64))
    centre = np.repeat(rng.uniform(-200.0, 200.0, len(lens)), lens)
    half = 0.4999 * spread                                        # the roundings of centre + offset stay inside `spread`
    return (centre + rng.uniform(-half, half, int(rowptr[-1]))) / abs(scale)


def wide_row(seed=0, length=700, spread=1500.0):
    """one row whose scores span `spread`: most outputs underflow"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-spread / 2, spread / 2, length)
    x[3], x[length - 2] = spread / 2, -spread / 2
    return np.array([0, length], np.int32), x


def sample_rows(rowptr, seed=1, n=SAMPLE_ROWS):
    """the rows checked against the Decimal reference: all when there are few, else n drawn by seed plus the longest row
    and the first one-entry row"""
    lens = np.diff(rowptr.astype(np.int64))
    rows = len(lens)
    if rows <= 2 * n:
        return list(range(rows))
    pick = set(int(r) for r in np.random.default_rng(seed).choice(rows, n, replace=False))
    pick.add(int(lens.argmax()))
    ones = np.flatnonzero(lens == 1)
    if len(ones):
        pick.add(int(ones[0]))
    return sorted(pick)
