"""The SpGEMM contract of include/sblas_hip.h restated in numpy (no scipy): C = A * B for two CSR matrices whose rows may
be unsorted and hold duplicates.

  1. expand: the triplets (i, j, a * b) in the numbering of (V) -- A's entries in stored order, and for each the entries
     of the B row it names in stored order;
  2. sort with numpy.lexsort((col, row)), which is stable;
  3. sum every run left to right: the first value is copied, each later one added by rank inside the run (vectorised
     across runs, sequential within one), so the result is the exact left-to-right sum and no pairwise one.

Values are compared as bits.  One class of values has no bits to compare: a NaN that an operation makes (Inf * 0,
Inf - Inf) has the sign and payload its adder chooses -- x86 makes the negative default NaN, the GPU the positive one --
and IEEE 754 leaves that open.  same_bits() therefore asks, where the reference holds a NaN, for a NaN, and everywhere
else for equal bits."""
import numpy as np


def expand(m, rowptr_a, colidx_a, val_a, rowptr_b, colidx_b, val_b):
    """(row, col, val) of every product, in the numbering of (V)"""
    rpa, rpb = np.asarray(rowptr_a, np.int64), np.asarray(rowptr_b, np.int64)
    cia, cib = np.asarray(colidx_a, np.int64), np.asarray(colidx_b, np.int64)
    va, vb = np.asarray(val_a, np.float64), np.asarray(val_b, np.float64)
    row_of_a = np.repeat(np.arange(m, dtype=np.int64), np.diff(rpa))
    lens = rpb[cia + 1] - rpb[cia] if len(cia) else np.zeros(0, np.int64)
    total = int(lens.sum())
    ent = np.repeat(np.arange(len(cia), dtype=np.int64), lens)            # the A entry of each product
    first = np.cumsum(lens) - lens
    bpos = rpb[cia[ent]] + (np.arange(total, dtype=np.int64) - first[ent])
    with np.errstate(all="ignore"):
        val = va[ent] * vb[bpos]
    return row_of_a[ent].astype(np.int32), cib[bpos].astype(np.int32), val


def sum_triplets(rows, row, col, val):
    """(rowptr, colidx, val) of the triplets: sorted by (row, col), equal pairs summed left to right in input order"""
    nnz = len(row)
    if nnz == 0:
        return np.zeros(rows + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64)
    order = np.lexsort((col, row))
    rs, cs, vs = row[order], col[order], val[order]
    head = np.ones(nnz, bool)
    head[1:] = (rs[1:] != rs[:-1]) | (cs[1:] != cs[:-1])
    start = np.flatnonzero(head)
    lens = np.diff(np.append(start, nnz))
    out = vs[start].copy()                                               # a run of one is copied
    with np.errstate(all="ignore"):
        for j in range(1, int(lens.max())):
            sel = lens > j
            out[sel] = out[sel] + vs[start[sel] + j]                     # ((p1 + p2) + p3) + ...
    rowptr = np.searchsorted(rs[start], np.arange(rows + 1), side="left")
    return rowptr.astype(np.int32), cs[start].astype(np.int32), out


def reference(m, n, rowptr_a, colidx_a, val_a, rowptr_b, colidx_b, val_b):
    """(rowptr_c, colidx_c, val_c) by the contract"""
    row, col, val = expand(m, rowptr_a, colidx_a, val_a, rowptr_b, colidx_b, val_b)
    return sum_triplets(m, row, col, val)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(got, ref):
    """equal bits, or a NaN where the reference holds a NaN (see the module comment)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape:
        return False
    nan = np.isnan(ref)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(ref)[~nan]))


def to_dense(m, n, rowptr, colidx, val):
    """dense m x n of a CSR, duplicates added (for integer-valued data, where every order is exact)"""
    d = np.zeros((m, n), np.float64)
    rows = np.repeat(np.arange(m), np.diff(np.asarray(rowptr, np.int64)))
    np.add.at(d, (rows, np.asarray(colidx, np.int64)), np.asarray(val, np.float64))
    return d


def pattern_dense(m, n, rowptr, colidx):
    d = np.zeros((m, n), bool)
    rows = np.repeat(np.arange(m), np.diff(np.asarray(rowptr, np.int64)))
    d[rows, np.asarray(colidx, np.int64)] = True
    return d


def random_csr(rng, rows, cols, per_row, sort=True, empty_every=0, integer=False):
    """a random CSR with row lengths 0 .. 2 * per_row (distinct columns in a row; ascending when sort)"""
    lens = rng.integers(0, 2 * per_row + 1, rows)
    lens = np.minimum(lens, cols)
    if empty_every:
        lens[::empty_every] = 0
    rowptr = np.zeros(rows + 1, np.int32)
    rowptr[1:] = np.cumsum(lens)
    colidx = np.zeros(int(rowptr[-1]), np.int32)
    for i in range(rows):
        c = rng.choice(cols, int(lens[i]), replace=False)
        colidx[rowptr[i]:rowptr[i + 1]] = np.sort(c) if sort else c
    nnz = len(colidx)
    val = rng.integers(-8, 9, nnz).astype(np.float64) if integer else rng.random(nnz) * 2 - 1
    return rowptr, colidx, val


def transpose_csr(rows, cols, rowptr, colidx, val):
    """the transpose as a CSR with ascending rows (stable: equal columns keep their row order)"""
    r = np.repeat(np.arange(rows, dtype=np.int32), np.diff(np.asarray(rowptr, np.int64)))
    order = np.argsort(np.asarray(colidx), kind="stable")
    rp = np.searchsorted(np.asarray(colidx)[order], np.arange(cols + 1), side="left").astype(np.int32)
    return rp, r[order].astype(np.int32), np.asarray(val)[order]
