"""The multicolour-reordering contract of include/sblas_hip.h restated in numpy (a plain helper module; no scipy, and
nothing shared with the kernels).

- priority(): h(v) = fmix32(v + 0x9E3779B9 * (seed + 1)) in wrapping uint32.
- neighbours(): u is a neighbour of v when u != v and the pattern stores (v, u) or (u, v).
- color_scalar(): the rule's own words -- visit the vertices in descending h, take the smallest colour no already-coloured
  neighbour holds.
- color_rounds(): the synchronous parallel form (Jones-Plassmann): in a round every uncoloured vertex none of whose
  uncoloured neighbours has a higher h takes its first fit, seeing only the colours of the rounds before -> the colours
  and the number of rounds.
- order(): perm, inv and color_ptr from the colours.
- permute(): P A P^T on the host, by the contract's own words, with src.
- the generators of the shapes the tests use."""
import numpy as np

import ilu0_numerics as IN
import sptrsv_numerics as TN

csr_of_rows = TN.csr_of_rows


# ---------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------
def fmix32(x):
    x = np.asarray(x, np.uint64) & 0xffffffff
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xffffffff
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xffffffff
    x ^= x >> 16
    return x


def priority(n, seed):
    salt = (0x9E3779B9 * ((seed + 1) & 0xffffffff)) & 0xffffffff
    return fmix32((np.arange(n, dtype=np.uint64) + salt) & 0xffffffff)


def neighbours(n, rowptr, colidx):
    """the sorted distinct neighbours of every vertex, as a list of int64 arrays"""
    rp = np.asarray(rowptr, np.int64)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    col = np.asarray(colidx, np.int64)
    a, b = np.concatenate([row, col]), np.concatenate([col, row])
    keep = a != b
    pairs = np.unique(a[keep] * max(n, 1) + b[keep])
    a, b = pairs // max(n, 1), pairs % max(n, 1)
    cut = np.searchsorted(a, np.arange(n + 1))
    return [b[cut[v]:cut[v + 1]] for v in range(n)]


def first_fit(colors):
    """the smallest c >= 0 not among `colors`"""
    held = set(int(c) for c in colors)
    c = 0
    while c in held:
        c += 1
    return c


def color_scalar(n, rowptr, colidx, seed=0):
    h, nb = priority(n, seed), neighbours(n, rowptr, colidx)
    assert len(np.unique(h)) == n                                           # no two vertices tie
    color = np.full(n, -1, np.int64)
    for v in np.argsort(h)[::-1]:
        c = color[nb[v]]
        color[v] = first_fit(c[c >= 0])
    return color.astype(np.int32)


def color_rounds(n, rowptr, colidx, seed=0):
    """-> (color, rounds) of the synchronous parallel form"""
    h, nb = priority(n, seed), neighbours(n, rowptr, colidx)
    color = np.full(n, -1, np.int64)
    rounds = 0
    left = list(range(n))
    while left:
        seen = color.copy()                                                 # a round sees the rounds before it only
        later = []
        for v in left:
            u = nb[v]
            open_ = u[seen[u] < 0]
            if len(open_) and h[open_].max() > h[v]:
                later.append(v)
            else:
                c = seen[u]
                color[v] = first_fit(c[c >= 0])
        assert len(later) < len(left), "a round without progress"
        left = later
        rounds += 1
    return color.astype(np.int32), rounds


def order(color):
    """-> (perm, inv, color_ptr, n_colors): the vertices by (colour, vertex), the inverse, and the classes' extents"""
    color = np.asarray(color, np.int64)
    n = len(color)
    perm = np.argsort(color, kind="stable")
    inv = np.zeros(n, np.int64)
    inv[perm] = np.arange(n)
    k = int(color.max()) + 1 if n else 0
    ptr = np.zeros(k + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(color, minlength=k)) if n else 0
    return perm.astype(np.int32), inv.astype(np.int32), ptr.astype(np.int32), k


def check_coloring(n, rowptr, colidx, color, n_colors):
    """no stored off-diagonal entry joins equal colours, and every colour in [0, n_colors) is used"""
    rp = np.asarray(rowptr, np.int64)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    col = np.asarray(colidx, np.int64)
    off = row != col
    assert not (color[row[off]] == color[col[off]]).any()
    assert np.array_equal(np.unique(color), np.arange(n_colors))


# ---------------------------------------------------------------------------------------------------------------------
# P A P^T
# ---------------------------------------------------------------------------------------------------------------------
def permute(n, rowptr, colidx, perm):
    """-> (rowptr_b, colidx_b, src): row r of B holds the entries of row perm[r] of A, columns relabelled inv[col], sorted
    ascending by new column, equal columns in A's stored order; src[e] is the entry's place in A"""
    rp, ci, perm = np.asarray(rowptr, np.int64), np.asarray(colidx, np.int64), np.asarray(perm, np.int64)
    inv = np.zeros(n, np.int64)
    inv[perm] = np.arange(n)
    rows, src = [], []
    for r in range(n):
        e = np.arange(rp[perm[r]], rp[perm[r] + 1])
        c = inv[ci[e]]
        o = np.argsort(c, kind="stable")
        rows.append(c[o]), src.append(e[o])
    rpb, cib = csr_of_rows(rows)
    return rpb, cib, (np.concatenate(src) if len(ci) else np.zeros(0, np.int64)).astype(np.int32)


def is_symmetric(n, rowptr, colidx):
    rp = np.asarray(rowptr, np.int64)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    col = np.asarray(colidx, np.int64)
    return np.array_equal(np.unique(row * n + col), np.unique(col * n + row))


# ---------------------------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------------------------
def diagonal(n):
    return csr_of_rows([[i] for i in range(n)])


def clique(n):
    return csr_of_rows([list(range(n)) for _ in range(n)])


def star(leaves):
    """a hub (vertex 0) stored once: its row names every leaf, the leaves store their diagonal only -- an unsymmetric
    pattern whose hub has a long row and whose leaves meet the hub through the transpose alone"""
    return csr_of_rows([list(range(leaves + 1))] + [[i] for i in range(1, leaves + 1)])


def degree_rows(lengths):
    """One vertex for each p in `lengths` whose two rows hold exactly p stored entries together: after a bank of
    max(lengths) vertices joined in a path (vertex i stores i + 1), vertex bank + t stores the bank's first p columns and
    nothing else, and nobody names it, so row bank + t of A has p entries and row bank + t of A^T none.
    -> (rp, ci, first such vertex)"""
    bank = max(max(lengths), 2)
    rows = [[i + 1] for i in range(bank - 1)] + [[]]
    for p in lengths:
        rows.append(list(range(p)))
    rp, ci = csr_of_rows(rows)
    return rp, ci, bank


def degrees(n, rowptr, colidx):
    """p(v) = the stored entries of row v of A plus those of row v of A^T (duplicates and the diagonal counted)"""
    return np.diff(np.asarray(rowptr, np.int64)) + np.bincount(np.asarray(colidx, np.int64), minlength=n)


def cases():
    """name -> (n, rowptr, colidx, structurally symmetric): the shapes of the issue"""
    rng = np.random.default_rng(1)
    out = {}

    def add(name, rp, ci):
        n = len(rp) - 1
        out[name] = (n, rp, ci, is_symmetric(n, rp, ci))

    add("grid48", *IN.grid5(48))
    add("tridiagonal3000", *IN.tridiagonal(3000))
    add("band600", *IN.band(600, 20))
    add("block_diagonal", *IN.block_diagonal(6, 70))
    add("random4000", *IN.random_near_diagonal(rng, 4000, 6, 200))
    add("arrow_band", *IN.arrow_band([5, 33, 70, 300])[:2])
    add("messy", *TN.messy(np.random.default_rng(2), 700))
    add("diagonal", *diagonal(500))
    add("n0", np.zeros(1, np.int32), np.zeros(0, np.int32))
    add("n1", np.array([0, 1], np.int32), np.array([0], np.int32))
    add("clique130", *clique(130))
    add("star5000", *star(5000))
    return out
