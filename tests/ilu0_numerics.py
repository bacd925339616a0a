"""The ILU(0) contract of include/sblas_hip.h restated in numpy (a plain helper module; no scipy, and nothing shared
with the kernels): lu = ILU0(A) on A's own pattern, rows strictly ascending in column with a stored diagonal.

- check(): the structure check's order and its bad row, by the contract's own words.
- ilu0_ref(): the row-wise (IKJ) elimination in scalar float64, a rounded product and a rounded difference per update,
  every entry updated in ascending k.  It is the BIT reference: the device must give the same bits.
- residual_ratio(): (L U - A) on the pattern, evaluated exactly with fractions.Fraction and held against the
  rounding-error bound that every evaluation of that recurrence satisfies (Higham, Accuracy and Stability of Numerical
  Algorithms, 2nd ed., Lemma 8.4), with no margin.
- the generators of the shapes the tests use."""
from fractions import Fraction

import numpy as np

import sptrsv_numerics as TN

csr_of_rows = TN.csr_of_rows
bits = TN.bits


# ---------------------------------------------------------------------------------------------------------------------
# structure
# ---------------------------------------------------------------------------------------------------------------------
def check(n, rowptr, colidx):
    """-> (diag_pos, None) for a sound structure, (None, bad_row) otherwise: rowptr first (starts at 0, never steps
    down), then every column's range in every row, then row by row strictly ascending columns and a stored diagonal"""
    rp, ci = np.asarray(rowptr, np.int64), np.asarray(colidx, np.int64)
    if rp[0] != 0:
        return None, 0
    for i in range(n):
        if rp[i + 1] < rp[i]:
            return None, i
    for i in range(n):
        c = ci[rp[i]:rp[i + 1]]
        if ((c < 0) | (c >= n)).any():
            return None, i
    dpos = np.zeros(n, np.int32)
    for i in range(n):
        c = ci[rp[i]:rp[i + 1]]
        if (np.diff(c) <= 0).any() or not (c == i).any():
            return None, i
        dpos[i] = rp[i] + int(np.argmax(c == i))
    return dpos, None


def full_sorted(n, rowptr, colidx):
    """the pattern with every diagonal added, rows sorted, nothing doubled"""
    rp = np.asarray(rowptr, np.int64)
    return csr_of_rows([sorted(set(np.asarray(colidx[rp[i]:rp[i + 1]], np.int64).tolist()) | {i}) for i in range(n)])


# ---------------------------------------------------------------------------------------------------------------------
# the bit reference
# ---------------------------------------------------------------------------------------------------------------------
def ilu0_ref(n, rp, ci, val):
    """lu = ILU0(A): the loop of the contract in scalar float64"""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    lu = np.array(val, np.float64)
    dpos = [int(rp[i] + np.searchsorted(ci[rp[i]:rp[i + 1]], i)) for i in range(n)]
    with np.errstate(all="ignore"):                                         # a zero pivot divides as IEEE 754 says
        for i in range(n):
            place = {int(ci[p]): p for p in range(rp[i], rp[i + 1])}
            for e in range(rp[i], dpos[i]):
                k = int(ci[e])
                l = lu[e] / lu[dpos[k]]
                lu[e] = l
                for f in range(dpos[k] + 1, rp[k + 1]):
                    p = place.get(int(ci[f]))
                    if p is not None:
                        t = l * lu[f]                                       # the product rounded,
                        lu[p] = lu[p] - t                                   # then the difference
    return lu


# ---------------------------------------------------------------------------------------------------------------------
# the residual on the pattern
# ---------------------------------------------------------------------------------------------------------------------
def residual_ratio(n, rp, ci, val, lu):
    """max over the stored (i, j) of |a_ij - sum_k l_ik u_kj - (l_ij u_jj or u_ij)| / (gamma(m + 1) * sum |terms|), the
    sum over the k < min(i, j) that row i stores and whose row stores j, m their number, the residual exact (Fraction).
    Lemma 8.4: y = (c - sum_{k=1..m} a_k b_k) / b evaluated in floating point in any order satisfies
    |c - sum a_k b_k - b y| <= gamma(m + 1) (sum |a_k b_k| + |b y|); for an entry of U, b = 1 and the division is exact.
    Nothing but finite data is expected."""
    rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    u = Fraction(1, 2 ** 53)
    F = [Fraction(float(v)) for v in lu]
    place = [{int(ci[p]): p for p in range(rp[i], rp[i + 1])} for i in range(n)]
    worst = Fraction(0)
    for i in range(n):
        for p in range(rp[i], rp[i + 1]):
            j = int(ci[p])
            last = F[p] * F[place[j][j]] if j < i else F[p]
            res, mag, m = Fraction(float(val[p])) - last, abs(last), 0
            for e in range(rp[i], rp[i + 1]):
                k = int(ci[e])
                if k >= min(i, j):
                    break
                f = place[k].get(j)
                if f is not None:
                    t = F[e] * F[f]
                    res, mag, m = res - t, mag + abs(t), m + 1
            if res != 0:
                gam = (m + 1) * u / (1 - (m + 1) * u)
                assert mag > 0
                worst = max(worst, abs(res) / (gam * mag))
    return float(worst)


# ---------------------------------------------------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------------------------------------------------
def dominant_values(rng, n, rp, ci):
    """off-diagonals uniform in [-1, 1), the diagonal 1 to 2 times (1 + the row's absolute off-diagonal sum), signed"""
    rp = np.asarray(rp, np.int64)
    val = rng.uniform(-1.0, 1.0, len(ci))
    dg = TN.on_diagonal(rp, ci)
    row = np.repeat(np.arange(n), np.diff(rp))
    s = np.bincount(row, np.where(dg, 0.0, np.abs(val)), minlength=n)
    d = (1.0 + s) * (1.0 + rng.random(n)) * rng.choice([-1.0, 1.0], n)
    val[dg] = d
    return val


def exact_bidiagonal_product(rng, n):
    """A = L0 U0 stored with the full tridiagonal pattern, where no fill arises: L0 unit lower bidiagonal with small
    integers, U0 upper bidiagonal with power-of-two pivots and small integers above them.  Every quotient and every
    update of ILU(0) is exact, so lu must hold L0 and U0 themselves.  -> (rp, ci, val, lu0)"""
    l = rng.integers(-3, 4, n).astype(np.float64)                           # l[i]: L0[i, i - 1]
    d = 2.0 ** rng.integers(0, 4, n)                                        # U0[i, i]
    s = rng.integers(-3, 4, n).astype(np.float64)                           # s[i]: U0[i, i + 1]
    rows, vals, want = [], [], []
    for i in range(n):
        r, v, w = [], [], []
        if i > 0:
            r.append(i - 1), v.append(l[i] * d[i - 1]), w.append(l[i])
        r.append(i), v.append(d[i] + (l[i] * s[i - 1] if i > 0 else 0.0)), w.append(d[i])
        if i < n - 1:
            r.append(i + 1), v.append(s[i]), w.append(s[i])
        rows.append(r), vals.append(v), want.append(w)
    rp, ci = csr_of_rows(rows)
    return rp, ci, np.concatenate(vals), np.concatenate(want)


# ---------------------------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------------------------
def grid5(side):
    """the five-point stencil on a side x side grid, full"""
    rows = []
    for i in range(side * side):
        r, c = divmod(i, side)
        rows.append(([i - side] if r > 0 else []) + ([i - 1] if c > 0 else []) + [i] + ([i + 1] if c < side - 1 else []) +
                    ([i + side] if r < side - 1 else []))
    return csr_of_rows(rows)


def tridiagonal(n):
    return csr_of_rows([[j for j in (i - 1, i, i + 1) if 0 <= j < n] for i in range(n)])


def band(n, half):
    return csr_of_rows([list(range(max(i - half, 0), min(i + half, n - 1) + 1)) for i in range(n)])


def block_diagonal(blocks, size):
    return csr_of_rows([list(range(b * size, (b + 1) * size)) for b in range(blocks) for _ in range(size)])


def random_near_diagonal(rng, n, per_row, reach):
    """about per_row entries a row, drawn within `reach` of the diagonal, plus the diagonal"""
    rows = []
    for i in range(n):
        c = rng.integers(max(i - reach, 0), min(i + reach, n - 1) + 1, per_row - 1)
        rows.append(sorted(set(c.tolist()) | {i}))
    return csr_of_rows(rows)


def leading_block(m, rp, ci, val):
    """the leading m x m block of the matrix"""
    rp = np.asarray(rp, np.int64)
    keep = [np.flatnonzero(ci[rp[i]:rp[i + 1]] < m) + rp[i] for i in range(m)]
    rp2, ci2 = csr_of_rows([ci[k] for k in keep])
    return rp2, ci2, np.concatenate([val[k] for k in keep])


def arrow_band(lengths, every=5):
    """A band of lead = max(lengths) + 6 rows (columns i - 1 .. i + 2), then one row for each length p in `lengths` with
    exactly p stored entries: the columns 0 .. p - 2 and its diagonal (a lower arrow).  Every `every`-th band row also
    stores the columns of ALL the arrow rows, so that the rows k an arrow row eliminates with have upper parts that hit
    its entries, its diagonal among them, and miss (the other arrow rows' columns).  -> (rp, ci, first arrow row)"""
    lead = max(lengths) + 6
    n = lead + len(lengths)
    rows = []
    for i in range(lead):
        rows.append([j for j in (i - 1, i, i + 1, i + 2) if 0 <= j < lead] + (list(range(lead, n)) if i % every == 0 else []))
    for t, p in enumerate(lengths):
        rows.append(list(range(p - 1)) + [lead + t])
    rp, ci = csr_of_rows(rows)
    assert np.diff(rp)[lead:].tolist() == list(lengths)
    return rp, ci, lead
