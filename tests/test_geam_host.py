"""GEAM's host side (geam_rule.cpp; no GPU): the new header against its export list, the scalar reference sblas_geam_ref
against the numpy restatement of the contract (tests/geam_numerics.py on spgemm_numerics.sum_triplets) in structure,
value bits and both maps, the special values, the nnz(C) limit and the Python refusals that need no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import geam_numerics as AN
import spgemm_numerics as GN
from conftest import ROOT

INVALID = 1
CASES = AN.shape_cases()


def test_the_library_exports_what_the_new_header_declares(sblas):
    hdr = open(os.path.join(ROOT, "include", "sblas_hip_geam.h")).read()
    declared = set(re.findall(r"\b(sblas_[A-Za-z0-9_]+)\s*\(", hdr))
    others = set(sblas.EXPORTS + sblas.EXPORTS_AMG_SA + sblas.EXPORTS_AMG_DEV + sblas.EXPORTS_CHEBY + sblas.EXPORTS_KRYLOV_MULTI +
                 sblas.EXPORTS_AMG_MULTI + sblas.EXPORTS_SPTRSM_TILE + sblas.EXPORTS_GMRES_MULTI)
    assert declared == set(sblas.EXPORTS_GEAM) and not declared & others, declared ^ set(sblas.EXPORTS_GEAM)
    assert len(set(sblas.EXPORTS_GEAM)) == len(sblas.EXPORTS_GEAM)
    assert '#include "sblas_hip_geam.h"' in open(os.path.join(ROOT, "include", "sblas_hip.h")).read()
    for name in declared:
        assert hasattr(sblas.lib(), name), name


def check_against_restatement(sblas, name, rows, cols, A, B, alpha, beta):
    got = sblas.geam_ref(rows, cols, A[0], A[1], A[2], B[0], B[1], B[2], alpha, beta)
    want = AN.restate(rows, A, B, alpha, beta)
    for k, what in ((0, "rowptr_c"), (1, "colidx_c"), (3, "dest_a"), (4, "dest_b")):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (name, what)
    assert GN.same_bits(got[2], want[2]), (name, alpha, beta)
    return got


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_reference_equals_the_restatement(sblas, name):
    rows, cols, A, B = CASES[name]
    alpha, beta = AN.scalars_of(name)
    rp, ci, val, da, db = check_against_restatement(sblas, name, rows, cols, A, B, alpha, beta)
    # (S) and (M) by their own words: ascending distinct rows, and every input entry lands on its own column in its own row
    for i in range(rows):
        assert (np.diff(ci[rp[i]:rp[i + 1]]) > 0).all()
    for M, d in ((A, da), (B, db)):
        assert np.array_equal(ci[d], M[1]) and np.array_equal(AN.rows_of(rp)[d], AN.rows_of(M[0]))


def test_three_terms_are_added_in_the_order_of_the_contract(sblas):
    rows, cols, A, B = CASES["dup_both"]
    rp, ci, val, _, _ = check_against_restatement(sblas, "dup_both_11", rows, cols, A, B, 1.0, 1.0)
    at = rp[0] + list(ci[rp[0]:rp[1]]).index(3)
    assert val[at] == ((1e16 + 1.0) + -1e16) + 5.0 == 5.0                     # B's -1e16 taken before A's 1.0 would give 6.0


@pytest.mark.parametrize("alpha", AN.SCALARS)
@pytest.mark.parametrize("beta", AN.SCALARS)
def test_every_pair_of_scalars_on_special_values(sblas, alpha, beta):
    for k, name in enumerate(("identical", "a_in_b", "unsorted", "dup_both", "random3_sorted")):
        rows, cols, A, B = CASES[name]
        A, B = AN.special_values(A, B, 3410 + k)
        check_against_restatement(sblas, name, rows, cols, A, B, alpha, beta)


def test_zeros_infinities_and_a_zero_alpha(sblas):
    inf, nan, tiny = np.inf, np.nan, 5e-324
    A = AN.csr_of_rows([([2], [-0.0]), ([3], [-0.0]), ([1, 6], [inf, 2.0]), ([0], [tiny]), ([4], [inf]), ([4], [nan])])
    B = AN.csr_of_rows([([5], [1.0]), ([3], [0.0]), ([], []), ([0], [tiny]), ([4], [-inf]), ([1], [1.0])])
    rp, ci, val, _, _ = check_against_restatement(sblas, "special", 6, 7, A, B, 1.0, 1.0)
    row = lambda i: val[rp[i]:rp[i + 1]]
    assert row(0)[0] == 0.0 and np.signbit(row(0)[0])                        # -0.0 alone stays -0.0
    assert row(1)[0] == 0.0 and not np.signbit(row(1)[0])                    # (-0.0) + 0.0 is +0.0
    assert row(3)[0] == 2 * tiny and np.isnan(row(4)[0]) and np.isnan(row(5)[1])
    rp0, ci0, val0, _, _ = check_against_restatement(sblas, "special_alpha0", 6, 7, A, B, 0.0, 1.0)
    assert np.array_equal(rp0, rp) and np.array_equal(ci0, ci)               # alpha = 0 keeps A's pattern
    assert np.isnan(val0[rp0[2]]) and val0[rp0[2] + 1] == 0.0                # 0 * Inf is a stored NaN, 0 * 2 a stored zero
    assert np.signbit(val0[rp0[0]]) and val0[rp0[0]] == 0.0                  # 0 * -0.0 = -0.0, copied


def test_no_product_is_fused_into_the_add(sblas):
    """geam_numerics.FMA_*: the contract's value is +0.0, a contraction of either product gives -+2^-54"""
    A = AN.csr_of_rows([([1], [AN.FMA_A])])
    B = AN.csr_of_rows([([1], [AN.FMA_B])])
    _, _, val, _, _ = check_against_restatement(sblas, "fma", 1, 2, A, B, AN.FMA_ALPHA, AN.FMA_BETA)
    assert val[0] == 0.0 and not np.signbit(val[0])
    from fractions import Fraction as Fr
    assert Fr(AN.FMA_ALPHA) * Fr(AN.FMA_A) + Fr(-1) == Fr(-1, 2 ** 54)        # what fma(alpha, a, fl(beta * b)) would keep
    assert Fr(AN.FMA_BETA) * Fr(AN.FMA_B) + Fr(1) == Fr(1, 2 ** 54)           # and fma(beta, b, fl(alpha * a))
    assert AN.FMA_ALPHA * AN.FMA_A == 1.0 and AN.FMA_BETA * AN.FMA_B == -1.0  # the rounded products


def test_the_nnz_limit(sblas):
    assert sblas.geam_check_nnz(2 ** 31 - 1) == 0 and sblas.geam_check_nnz(2 ** 31) == INVALID
    assert sblas.geam_check_nnz(0) == 0 and sblas.geam_check_nnz(-1) == INVALID


def test_the_reference_refuses_a_bad_structure(sblas):
    L = sblas.lib()
    rows, cols, A, B = CASES["identical"]

    def call(A, B, rows=rows, cols=cols, null=()):
        arrs = [np.ascontiguousarray(A[0], np.int32), np.ascontiguousarray(A[1], np.int32), np.ascontiguousarray(A[2]),
                np.ascontiguousarray(B[0], np.int32), np.ascontiguousarray(B[1], np.int32), np.ascontiguousarray(B[2])]
        n = len(arrs[1]) + len(arrs[4])
        outs = [np.zeros(rows + 1, np.int32), np.zeros(n, np.int32), np.zeros(n), np.zeros(len(arrs[1]), np.int32),
                np.zeros(len(arrs[4]), np.int32)]
        p = [None if j in null else a.ctypes.data for j, a in enumerate(arrs + outs)]
        nnz = C.c_int64(-7)
        rc = L.sblas_geam_ref(rows, cols, *p[:6], 1.0, 1.0, *p[6:], C.byref(nnz))
        return rc, nnz.value

    assert call(A, B)[0] == 0
    for which in (0, 1):
        for mutate in ("late", "down", "col_high", "col_negative"):
            M = [a.copy() for a in (A, B)[which]]
            if mutate == "late":
                M[0][0] = 1
            elif mutate == "down":
                M[0][1] = M[0][2] + 1
            elif mutate == "col_high":
                M[1][3] = cols
            else:
                M[1][5] = -1
            pair = (tuple(M), B) if which == 0 else (A, tuple(M))
            assert call(*pair) == (INVALID, -7), (which, mutate)
    for null in (0, 1, 2, 3, 4, 5, 6):
        assert call(A, B, null=(null,))[0] == INVALID, null
    rc, nnz = call(A, B, null=(7, 8, 9, 10))                                 # count only: every optional output NULL
    assert rc == 0 and nnz == len(A[1])
    assert call(A, B, rows=-1)[0] == INVALID


def test_python_refusals_that_need_no_gpu(sblas):
    import torch
    rows, cols, A, B = CASES["identical"]
    t = lambda a, dt=torch.int32: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
    rpa, cia, rpb, cib = t(A[0]), t(A[1]), t(B[0]), t(B[1])
    with pytest.raises(sblas.SblasError, match="GPU tensor"):
        sblas.GeamPlan(rows, cols, rpa, cia, rpb, cib)
    with pytest.raises(sblas.SblasError, match="int32"):
        sblas.GeamPlan(rows, cols, t(A[0], torch.int64), cia, rpb, cib)
    with pytest.raises(sblas.SblasError, match="int32"):
        sblas.GeamPlan(rows, cols, rpa, cia, rpb, t(B[1], torch.int64))
    with pytest.raises(sblas.SblasError, match="rows \\+ 1"):
        sblas.GeamPlan(rows + 1, cols, rpa, cia, rpb, cib)
    with pytest.raises(sblas.SblasError, match="rows \\+ 1"):
        sblas.GeamPlan(rows, cols, rpa, cia, rpb[:-1].contiguous(), cib)
    with pytest.raises(sblas.SblasError, match="contiguous"):
        sblas.GeamPlan(rows, cols, rpa, cia[::2], rpb, cib)
    with pytest.raises(sblas.SblasError, match="GPU tensor"):
        sblas.GeamPlan(rows, cols, A[0], cia, rpb, cib)                       # a numpy array is no tensor
    dA, dB = (rows, cols, rpa, cia, t(A[2], torch.float64)), (rows, cols + 1, rpb, cib, t(B[2], torch.float64))
    with pytest.raises(sblas.SblasError, match="A is"):
        sblas.csr_add(dA, dB)
    with pytest.raises(sblas.SblasError):
        sblas.geam_ref(rows, cols, A[0], A[1], A[2][:-1], B[0], B[1], B[2])   # val_a shorter than colidx_a
    with pytest.raises(sblas.SblasError):
        sblas.geam_ref(rows + 1, cols, A[0], A[1], A[2], B[0], B[1], B[2])
    import sblas_amd.autograd as AG
    with pytest.raises(sblas.SblasError, match="GeamPlan"):
        AG.csr_add(None, t(A[2], torch.float64), t(B[2], torch.float64))
