"""The narrow SDDMM's host side (sddmm_narrow_rule.cpp; no GPU): the new header against its export list, the scalar
reference sblas_sddmm_narrow_ref against the Python restatement of the contract (tests/sddmm_narrow_numerics.py) with ==,
the exact grids and the error bound of sddmm_numerics.py, the rows an entry outside the part never reads, the limits, the
refusals, and the adjoint formulas of the solves with the reference as their values gradient under torch's gradcheck."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sddmm_narrow_numerics as NN
import sddmm_numerics as SN
from conftest import ROOT

INVALID = 1
PAT = NN.small_pattern()


def test_the_library_exports_what_the_new_header_declares(sblas):
    hdr = open(os.path.join(ROOT, "include", "sblas_hip_sddmm_narrow.h")).read()
    declared = set(re.findall(r"\b(sblas_[A-Za-z0-9_]+)\s*\(", hdr))
    others = set(sblas.EXPORTS + sblas.EXPORTS_AMG_SA + sblas.EXPORTS_AMG_DEV + sblas.EXPORTS_CHEBY + sblas.EXPORTS_KRYLOV_MULTI +
                 sblas.EXPORTS_AMG_MULTI + sblas.EXPORTS_SPTRSM_TILE + sblas.EXPORTS_GMRES_MULTI + sblas.EXPORTS_GEAM +
                 sblas.EXPORTS_MSPGEMM)
    assert declared == set(sblas.EXPORTS_SDDMM_NARROW) and not declared & others, declared ^ set(sblas.EXPORTS_SDDMM_NARROW)
    assert len(set(sblas.EXPORTS_SDDMM_NARROW)) == len(sblas.EXPORTS_SDDMM_NARROW)
    assert '#include "sblas_hip_sddmm_narrow.h"' in open(os.path.join(ROOT, "include", "sblas_hip.h")).read()
    for name in declared:
        assert hasattr(sblas.lib(), name), name


def test_limits(sblas):
    lim = sblas.sddmm_narrow_limits()
    assert lim["max_k"] == 8 and lim["chunk"] == lim["threads"] * lim["entries_per_lane"] and lim["threads"] % 64 == 0
    assert sblas.lib().sblas_sddmm_narrow_limits(None) == INVALID


@pytest.mark.parametrize("k", range(1, 9))
def test_the_reference_equals_the_restatement(sblas, k):
    rows, cols, rp, ci = PAT
    assert (np.diff(rp) == 0).any() and len(ci) > 20
    rng = np.random.default_rng(k)
    X, Y, old = SN.log_uniform(rng, (rows, k), 12), SN.log_uniform(rng, (cols, k), 12), SN.log_uniform(rng, len(ci), 12)
    for alpha in (1.0, -1.0, 0.5):
        for beta in (0.0, 1.0, -2.0):
            for part in NN.PARTS:
                got = sblas.sddmm_narrow_ref(rows, cols, rp, ci, X, Y, old if beta else None, alpha, beta, part)
                want = NN.restate(rp, ci, X, Y, old, alpha, beta, part)
                assert got.dtype == np.float64 and (got == want).all(), (k, alpha, beta, part)


@pytest.mark.parametrize("k", [1, 4, 5, 8])
def test_leading_dimensions_and_aliasing(sblas, k):
    rows, cols, rp, ci = PAT
    rng = np.random.default_rng(40 + k)
    wide = SN.log_uniform(rng, (rows, k + 3), 12)
    X, Y = wide[:, 1:1 + k], SN.log_uniform(rng, (cols, k + 1), 12)[:, :k]         # ld > k, one of them off its base
    assert (sblas.sddmm_narrow_ref(rows, cols, rp, ci, X, Y) == NN.restate(rp, ci, X, Y, None, 1.0, 0.0)).all()
    assert rows == cols                                                             # X aliasing Y on a square pattern
    for part in NN.PARTS:
        assert (sblas.sddmm_narrow_ref(rows, cols, rp, ci, X, X, part=part) == NN.restate(rp, ci, X, X, None, 1.0, 0.0, part)).all()


def test_degenerate_sizes(sblas):
    z = np.zeros(1, np.int32)
    assert len(sblas.sddmm_narrow_ref(0, 0, z, [], np.zeros((0, 3)), np.zeros((0, 3)))) == 0          # rows = 0
    assert len(sblas.sddmm_narrow_ref(3, 2, np.zeros(4, np.int32), [], np.ones((3, 2)), np.ones((2, 2)))) == 0   # nnz = 0
    out = sblas.sddmm_narrow_ref(2, 2, [0, 0, 1], [0], [3.0, 5.0], [7.0, 9.0], part="strict_lower")   # 1-D operands: k = 1
    assert out.tolist() == [35.0]


@pytest.mark.parametrize("k", range(1, 9))
def test_exact_grid(sblas, k):
    rows, cols, rp, ci = PAT
    for alpha, beta in ((1.0, 0.0), (-2.0, 0.5), (0.5, -1.0)):
        g = SN.grid_problem(rp, ci, rows, cols, k, alpha, beta, seed=k)
        got = sblas.sddmm_narrow_ref(rows, cols, rp, ci, g.X, g.Y, g.old if beta else None, alpha, beta)
        assert (got == g.expected).all(), (k, alpha, beta)


@pytest.mark.parametrize("k", range(1, 9))
def test_error_bound_on_log_uniform_data(sblas, k):
    rows, cols, rp, ci = PAT
    rng = np.random.default_rng(70 + k)
    X, Y, old = SN.log_uniform(rng, (rows, k), 40), SN.log_uniform(rng, (cols, k), 40), SN.log_uniform(rng, len(ci), 40)
    for alpha, beta in ((1.0, 0.0), (-0.7, 1.3)):
        got = sblas.sddmm_narrow_ref(rows, cols, rp, ci, X, Y, old if beta else None, alpha, beta)
        ok, worst, where, over = SN.check_general(got, rp, ci, X, Y, old, alpha, beta)
        assert ok, (k, alpha, beta, worst, where, over)


@pytest.mark.parametrize("part", ["lower", "strict_lower", "upper", "strict_upper"])
def test_rows_outside_the_part_are_never_read(sblas, part):
    rows = cols = 6                                        # every part leaves rows and columns that only outside entries name
    rp, ci = np.array([0, 2, 4, 4, 5, 7, 10], np.int32), np.array([3, 5, 1, 0, 4, 0, 1, 2, 5, 2], np.int32)
    r, c = SN.entry_rows(rp, ci)
    mask = np.array([NN.in_part(part, int(a), int(b)) for a, b in zip(r, c)])
    rng = np.random.default_rng(9)
    X, Y, old = SN.log_uniform(rng, (rows, 3), 12), SN.log_uniform(rng, (cols, 3), 12), SN.log_uniform(rng, len(ci), 12)
    bad_x, bad_y = np.setdiff1d(r[~mask], r[mask]), np.setdiff1d(c[~mask], c[mask])
    assert len(bad_x) and len(bad_y)
    X[bad_x], Y[bad_y] = np.nan, np.inf
    for beta in (0.0, 0.5):
        got = sblas.sddmm_narrow_ref(rows, cols, rp, ci, X, Y, old, 1.0, beta, part)
        assert np.isfinite(got).all()
        assert (got[~mask] == (beta * old[~mask] if beta else 0.0)).all() and (beta or not np.signbit(got[~mask]).any())
    e = int(np.flatnonzero(mask)[0])                       # inside the part the classes follow the operands
    X[r[e]] = -np.inf
    got = sblas.sddmm_narrow_ref(rows, cols, rp, ci, X, Y, None, 1.0, 0.0, part)
    clean_x, clean_y = X.copy(), Y.copy()
    clean_x[bad_x], clean_y[bad_y] = 1.0, 1.0              # what the prediction may read: only rows of inside entries matter
    cls = SN.predict_class(rp, ci, clean_x, clean_y, None, 1.0, 0.0)
    seen = np.where(np.isnan(got), 1, np.where(got == np.inf, 2, np.where(got == -np.inf, 3, 0)))
    assert (seen[mask] == cls[mask]).all() and (seen[~mask] == 0).all() and seen[e] != 0


def test_refusals(sblas):
    L = sblas.lib()
    rp, ci = np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32)
    X, Y, out = np.ones((2, 8)), np.ones((2, 8)), np.zeros(2)
    p = lambda a: a.ctypes.data

    def call(rows=2, cols=2, nnz=2, rowptr=rp, colidx=ci, ldx=8, ldy=8, k=2, part=0):
        return L.sblas_sddmm_narrow_ref(-1, None, rows, cols, nnz, p(rowptr), p(colidx), p(X), ldx, p(Y), ldy, k, 1.0, 0.0, part, p(out))
    assert call() == 0
    for bad in (dict(k=0), dict(k=9), dict(k=-1), dict(ldx=1), dict(ldy=1), dict(part=5), dict(part=-1), dict(rows=-1),
                dict(nnz=1 << 31), dict(rows=1 << 31), dict(cols=1 << 31), dict(cols=0), dict(cols=1),
                dict(rowptr=np.array([1, 1, 2], np.int32)), dict(rowptr=np.array([0, 2, 1], np.int32)),
                dict(rowptr=np.array([0, 1, 1], np.int32)), dict(colidx=np.array([0, -1], np.int32))):
        assert call(**bad) == INVALID, bad
    with pytest.raises(sblas.SblasError):
        sblas.sddmm_narrow_ref(2, 2, rp, ci, X, Y, part="diagonal")
    with pytest.raises(sblas.SblasError):
        sblas.sddmm_narrow_ref(2, 2, rp, ci, X, Y[:, :3])
    with pytest.raises(sblas.SblasError):
        sblas.sddmm_narrow_ref(2, 2, rp, ci, X[:, :2], Y[:, :2], beta=1.0)          # beta != 0 needs out


# ---- the adjoint formulas of the solves, with the reference as the values gradient ---------------------------------------
def _solve_function(torch, sblas, n, rp, ci, part, unit, alpha):
    """x = T(val)^-1 (alpha b) as a torch Function over dense CPU solves: T takes the stored entries inside `part`
    (duplicates add up) and, for `unit`, a unit diagonal.  backward: g = T^-T dx, db = alpha g, dval[e] = -<g[row e], x[col e]>
    on the part through sddmm_narrow_ref."""
    r, c = SN.entry_rows(rp, ci)
    keep = torch.from_numpy(np.array([NN.in_part(part, int(a), int(b)) for a, b in zip(r, c)]))
    rt, ct = torch.from_numpy(r), torch.from_numpy(c)

    def dense(val):
        T = torch.zeros(n, n, dtype=torch.float64)
        T.index_put_((rt[keep], ct[keep]), val[keep], accumulate=True)
        return T + torch.eye(n, dtype=torch.float64) if unit else T

    class Solve(torch.autograd.Function):
        @staticmethod
        def forward(ctx, val, b):
            x = torch.linalg.solve(dense(val), alpha * b)
            ctx.save_for_backward(val, x)
            return x

        @staticmethod
        def backward(ctx, dx):
            val, x = ctx.saved_tensors
            g = torch.linalg.solve(dense(val).t(), dx)
            dval = sblas.sddmm_narrow_ref(n, n, rp, ci, g.contiguous().numpy(), x.contiguous().numpy(), None, -1.0, 0.0, part)
            return torch.from_numpy(dval), alpha * g
    return Solve.apply


@pytest.mark.parametrize("kind", ["lower", "unit_upper", "full"])
@pytest.mark.parametrize("s", [0, 3])
def test_adjoint_formulas_pass_gradcheck(sblas, kind, s):
    import torch
    n = 12
    rng = np.random.default_rng(3)
    rows = []
    for i in range(n):                                     # unsorted rows, a duplicated off-diagonal entry, both triangles
        off = rng.choice([j for j in range(n) if j != i], size=4, replace=False).tolist()
        rows.append(off[:2] + [i] + off[2:] + off[:1])
    rp = np.arange(0, 6 * n + 1, 6, dtype=np.int32)
    ci = np.asarray(rows, np.int32).reshape(-1)
    val = rng.uniform(-0.4, 0.4, len(ci))
    val[2::6] = rng.uniform(4.0, 5.0, n)                   # the diagonal
    part, unit, alpha = {"lower": ("lower", False, 0.5), "unit_upper": ("strict_upper", True, 1.0), "full": ("all", False, 1.0)}[kind]
    f = _solve_function(torch, sblas, n, rp, ci, part, unit, alpha)
    v = torch.from_numpy(val).requires_grad_()
    b = torch.from_numpy(rng.standard_normal((n, s) if s else n)).requires_grad_()
    assert torch.autograd.gradcheck(f, (v, b), nondet_tol=0.0)
