"""What the Krylov solvers' tests share: the pinned dot product restated in numpy, the vectors that show its order,
the matrices of the solver cases and the host loops the counts are held against.  No GPU and no library call in here."""
import numpy as np

import ilu0_numerics as IN
import sptrsv_numerics as TN

CELL, WIDTH = 2048, 256                                                     # the header's C and W, restated on purpose


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(got, want):
    """== on the bits, NaNs compared as NaNs (which NaN a sum of several returns is not part of the contract)"""
    got, want = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(want, np.float64))
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def butterfly(v):
    """v[..., l] = v[..., l] + v[..., l ^ m] for m = 1, 2, ... 128 over the 256 lanes of the last axis -> lane 0"""
    lanes = np.arange(WIDTH)
    for m in (1, 2, 4, 8, 16, 32, 64, 128):
        v = v + v[..., lanes ^ m]
    return v[..., 0]


def dot_np(x, y):
    """The written order, in numpy: cells of CELL elements; lane t of a cell takes elements t, t + 256, ... in order,
    acc = acc + x * y from +0 with the product rounded and then the sum, absent elements skipped; the butterfly; then
    lane t of the second stage adds partial[t], partial[t + 256], ... in order from +0, and the same butterfly."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n = len(x)
    cells = -(-n // CELL)
    with np.errstate(all="ignore"):
        if cells == 0:
            return np.float64(0.0)
        pad = cells * CELL - n
        live = np.concatenate([np.ones(n, bool), np.zeros(pad, bool)]).reshape(cells, CELL // WIDTH, WIDTH)
        prod = (np.concatenate([x, np.zeros(pad)]) * np.concatenate([y, np.zeros(pad)])).reshape(cells, CELL // WIDTH, WIDTH)
        acc = np.zeros((cells, WIDTH))
        for k in range(CELL // WIDTH):
            acc = np.where(live[:, k], acc + prod[:, k], acc)
        partial = butterfly(acc)
        rounds = -(-cells // WIDTH)
        grid = np.concatenate([partial, np.zeros(rounds * WIDTH - cells)]).reshape(rounds, WIDTH)
        there = (np.arange(rounds * WIDTH) < cells).reshape(rounds, WIDTH)
        acc = np.zeros(WIDTH)
        for k in range(rounds):
            acc = np.where(there[k], acc + grid[k], acc)
        return butterfly(acc)


def sizes():
    """n of the dot tests: the lane, wave and workgroup edges, the cell edges, several cells with a ragged last one, and
    more cells than the second stage has lanes"""
    return [0, 1, 63, 64, 65, 255, 256, 257, CELL - 1, CELL, CELL + 1, 3 * CELL + 5, WIDTH * CELL + 3]


def vectors(kind, n, seed=0):
    """(x, y) of n entries.  random: standard normal.  mixed: magnitudes 1e+-150 so that the order of the additions
    shows (and products overflow and underflow).  special: random with Inf, -Inf and NaN planted."""
    rng = np.random.default_rng(1000 * seed + n % 997)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    if kind == "mixed":
        x = x * 10.0 ** rng.choice([-150, -75, 0, 75, 150], n)
        y = y * 10.0 ** rng.choice([-150, -75, 0, 75, 150], n)
    elif kind == "special" and n:
        for v, what in ((x, np.inf), (y, -np.inf), (x, np.nan), (y, 0.0)):
            v[rng.integers(0, n, max(n // 200, 1))] = what
    elif kind != "random":
        assert n == 0 or kind == "special", kind
    return x, y


# ---- matrices ---------------------------------------------------------------------------------------------------------
def laplacian(side):
    rp, ci = IN.grid5(side)
    return side * side, rp, ci, np.where(TN.on_diagonal(rp, ci), 4.0, -1.0)


def spd_perturbed(side, seed=3):
    """the grid's pattern with random symmetric off-diagonal entries in [-1, -0.5] and a diagonal that dominates: SPD"""
    n, rp, ci, _ = laplacian(side)
    rng = np.random.default_rng(seed)
    row = np.repeat(np.arange(n), np.diff(rp))
    lo, hi = np.minimum(row, ci), np.maximum(row, ci)
    w = -(0.5 + 0.5 * rng.random(n * n)).reshape(n, n)
    val = w[lo, hi]
    off = np.bincount(row, np.where(row == ci, 0.0, np.abs(val)), minlength=n)
    val = np.where(row == ci, off[row] + 0.1 + rng.random(n)[row], val)
    return n, rp, ci, val


def convection_diffusion(side, wind=1.5):
    """-lap(u) + wind * du/dx with first-order upwind differences on the grid: nonsymmetric, diagonally dominant"""
    n, rp, ci, _ = laplacian(side)
    row = np.repeat(np.arange(n), np.diff(rp))
    val = np.where(row == ci, 4.0 + wind, -1.0)
    val = np.where(ci == row - 1, -1.0 - wind, val)                          # the upwind neighbour along x
    return n, rp, ci, val


def matvec(n, rp, ci, val, x):
    row = np.repeat(np.arange(n), np.diff(rp.astype(np.int64)))
    return np.bincount(row, val * x[ci], minlength=n)


def host_pcg(n, rp, ci, val, b, lu, tol, limit=1000):
    """The host loop of tests/test_gpu_ilu0.py and test_gpu_color.py, restated: preconditioned CG with A p by rows and
    M^-1 r by substitution with the factor lu in stored order (lu = None: plain CG).  -> (iterations until |r| <=
    tol |b|, x at that iterate)"""
    rp = rp.astype(np.int64)

    def precond(r):
        if lu is None:
            return r.copy()
        y = np.zeros(n)
        for i in range(n):
            c, v = ci[rp[i]:rp[i + 1]], lu[rp[i]:rp[i + 1]]
            y[i] = r[i] - np.dot(v[c < i], y[c[c < i]])
        z = np.zeros(n)
        for i in range(n - 1, -1, -1):
            c, v = ci[rp[i]:rp[i + 1]], lu[rp[i]:rp[i + 1]]
            z[i] = (y[i] - np.dot(v[c > i], z[c[c > i]])) / v[c == i][0]
        return z

    x, r = np.zeros(n), b.copy()
    z = precond(r)
    p, rz, stop = z.copy(), r @ z, tol * np.linalg.norm(b)
    for it in range(1, limit + 1):
        q = matvec(n, rp, ci, val, p)
        alpha = rz / (p @ q)
        x, r = x + alpha * p, r - alpha * q
        if np.linalg.norm(r) <= stop:
            return it, x
        z = precond(r)
        rz, old = r @ z, rz
        p = z + (rz / old) * p
    return limit + 1, x
