"""The masked SpGEMM's host side (mspgemm_rule.cpp; no GPU): the new header against its export list, the scalar reference
sblas_mspgemm_ref against the numpy restatement of the contract (tests/mspgemm_numerics.py) bit for bit, the contraction
pair, the NaN / Inf classes, the identity with SpGEMM on the restatements, the limits and the refusals that need no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mspgemm_numerics as MN
import spgemm_numerics as GN
from conftest import ROOT

INVALID = 1
CASES = MN.host_cases()


def test_the_library_exports_what_the_new_header_declares(sblas):
    hdr = open(os.path.join(ROOT, "include", "sblas_hip_mspgemm.h")).read()
    declared = set(re.findall(r"\b(sblas_[A-Za-z0-9_]+)\s*\(", hdr))
    others = set(sblas.EXPORTS + sblas.EXPORTS_AMG_SA + sblas.EXPORTS_AMG_DEV + sblas.EXPORTS_CHEBY + sblas.EXPORTS_KRYLOV_MULTI +
                 sblas.EXPORTS_AMG_MULTI + sblas.EXPORTS_SPTRSM_TILE + sblas.EXPORTS_GMRES_MULTI + sblas.EXPORTS_GEAM)
    assert declared == set(sblas.EXPORTS_MSPGEMM) and not declared & others, declared ^ set(sblas.EXPORTS_MSPGEMM)
    assert len(set(sblas.EXPORTS_MSPGEMM)) == len(sblas.EXPORTS_MSPGEMM)
    assert '#include "sblas_hip_mspgemm.h"' in open(os.path.join(ROOT, "include", "sblas_hip.h")).read()
    for name in declared:
        assert hasattr(sblas.lib(), name), name


def ref_of(sblas, case):
    m, n, k, M, X, Y = case
    return sblas.mspgemm_ref(m, n, k, M[0], M[1], X[0], X[1], X[2], Y[0], Y[1], Y[2])


def check_against_restatement(sblas, name, case):
    got, want = ref_of(sblas, case), MN.restate(case[3], case[4], case[5])
    assert got.dtype == np.float64 and GN.same_bits(got, want), name
    return got


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_reference_equals_the_restatement(sblas, name):
    got = check_against_restatement(sblas, name, CASES[name])
    assert len(got) == len(CASES[name][3][1])


def test_an_entry_without_a_pair_is_plus_zero_and_a_single_product_is_copied(sblas):
    out = check_against_restatement(sblas, "no_pair", CASES["no_pair"])
    assert out[0] == 1.0 and out[1] == 2.0 - 3.0                                 # (2 * 1) + (-3 * 1): X's order
    assert out[2] == 0.0 and not np.signbit(out[2])
    out = check_against_restatement(sblas, "minus_zero", CASES["minus_zero"])
    assert out[0] == 0.0 and np.signbit(out[0])                                  # -0.0 * 5 alone stays -0.0
    assert out[1] == 0.0 and np.signbit(out[1])                                  # (-0.0 * 1) + (-1 * 0.0) = -0.0 + -0.0
    out = check_against_restatement(sblas, "one_by_one", CASES["one_by_one"])
    assert out[0] == 1.0                                                         # fl(fl(1/3) * 3)


def test_the_products_are_added_in_the_order_of_the_contract(sblas):
    out = check_against_restatement(sblas, "dup_order", CASES["dup_order"])
    # X stores (3: 1e16), (1: 1), (3: -1e16): (1e16 + 1) + -1e16 = 0; taking column 3's two entries together would give 1
    assert out[0] == (1e16 + 1.0) + -1e16 == 0.0 and GN.bits(out)[0] == GN.bits(out)[1]
    out = check_against_restatement(sblas, "dup_order_y", CASES["dup_order_y"])
    assert out[0] == (1e16 + 1.0) + -1e16 == 0.0                                 # Y's stored order inside one X entry


@pytest.mark.parametrize("q", range(len(MN.FMA_CASES)))
def test_no_product_is_fused_into_the_add(sblas, q):
    """mspgemm_numerics.FMA_CASES: either contraction would change the last bit"""
    x1, y1, x2, y2 = MN.FMA_CASES[q]
    p1, p2 = x1 * y1, x2 * y2
    want = p1 + p2
    assert MN.fma(x2, y2, p1) != want and MN.fma(x1, y1, p2) != want             # the pair is what it claims to be
    out = check_against_restatement(sblas, "fma%d" % q, MN.fma_case(q))
    assert GN.bits(out)[0] == GN.bits(np.array([want]))[0]


def test_the_pair_is_found_by_a_search_over_random_triples():
    rng = np.random.default_rng(3501)
    hits = 0
    for _ in range(300):
        x, y, acc = (float(v) for v in rng.random(3) * 2 - 1)
        hits += MN.fma(x, y, acc) != x * y + acc
    assert hits > 10                                                             # a contraction shows on random data at once


def test_nan_and_inf_classes(sblas):
    inf = np.inf
    M = MN.pattern_of_rows([[0, 1, 2, 3]])
    X = MN.csr_of_rows([([0, 2, 5], [inf, 2.0, 0.0])])
    Y = MN.csr_of_rows([([2, 1], [3.0, inf]),            # Inf of X at column 0, Inf of Y at column 1: unmatched, never read
                        ([5, 3], [inf, np.nan]),         # 0 * Inf matched: NaN; the NaN at column 3 is unmatched
                        ([0, 0], [1.0, -1.0]),           # Inf * 1 + Inf * -1: Inf - Inf = NaN
                        ([0, 2], [-1.0, 1e308])])        # -Inf + 2e308 -> -Inf + Inf (the product overflows): NaN
    out = check_against_restatement(sblas, "classes", (1, 4, 6, M, X, Y))
    assert out[0] == 6.0 and np.isnan(out[1]) and np.isnan(out[2]) and np.isnan(out[3])
    with np.errstate(all="ignore"):
        dense = GN.to_dense(1, 6, *X) @ GN.to_dense(4, 6, *Y).T                   # a dense product would poison entry 0
    assert np.isnan(dense[0, 0])
    for k, name in enumerate(("rect", "unsorted", "dup_x", "dup_y")):
        m, n, kk, Mk, Xk, Yk = CASES[name]
        Xs, Ys = MN.special_values(Xk, Yk, 3510 + k)
        check_against_restatement(sblas, name + "_special", (m, n, kk, Mk, Xs, Ys))


@pytest.mark.parametrize("kind", ["sorted", "unsorted_dups"])
def test_on_the_product_s_pattern_the_restatement_is_spgemm(sblas, kind):
    """mask = C's pattern, X = A, Y = the stable transpose of B: SpGEMM's values, bit for bit"""
    rng = np.random.default_rng(3520)
    m, k, n = 30, 22, 35
    if kind == "sorted":
        A, B = GN.random_csr(rng, m, k, 4, empty_every=7), GN.random_csr(rng, k, n, 4, empty_every=5)
    else:
        _, _, _, _, A, _ = MN.random_case(rng, m, n, k, 3, 4, 3, sort=False, dup="x")
        _, _, _, _, B, _ = MN.random_case(rng, k, m, n, 3, 4, 3, sort=False, dup="x")
        assert not MN.ascending(A[0], A[1]) and not MN.ascending(B[0], B[1])
    rpc, cic, vc = GN.reference(m, n, A[0], A[1], A[2], B[0], B[1], B[2])
    Bt = GN.transpose_csr(k, n, B[0], B[1], B[2])
    assert len(vc) > 50
    assert GN.same_bits(MN.restate((rpc, cic), A, Bt), vc)
    assert GN.same_bits(sblas.mspgemm_ref(m, n, k, rpc, cic, A[0], A[1], A[2], Bt[0], Bt[1], Bt[2]), vc)


def test_the_limits(sblas):
    lim = sblas.mspgemm_limits()
    assert lim["threads"] % 64 == 0 and lim["threads"] >= 64 and lim["lds_row"] >= 64
    out = (C.c_int64 * 4)(-1, -1, -1, -1)
    assert sblas.lib().sblas_mspgemm_limits(out) == 0 and list(out) == [lim["lds_row"], lim["threads"], 0, 0]
    assert sblas.lib().sblas_mspgemm_limits(None) == INVALID


def test_the_reference_refuses_a_bad_structure(sblas):
    L = sblas.lib()
    m, n, k, M, X, Y = CASES["rect"]

    def call(M, X, Y, m=m, n=n, k=k, null=()):
        arrs = [np.ascontiguousarray(M[0], np.int32), np.ascontiguousarray(M[1], np.int32), np.ascontiguousarray(X[0], np.int32),
                np.ascontiguousarray(X[1], np.int32), np.ascontiguousarray(X[2]), np.ascontiguousarray(Y[0], np.int32),
                np.ascontiguousarray(Y[1], np.int32), np.ascontiguousarray(Y[2])]
        out = np.full(len(arrs[1]), -7.0)
        p = [None if j in null else a.ctypes.data for j, a in enumerate(arrs + [out])]
        return L.sblas_mspgemm_ref(m, n, k, *p), out

    rc, out = call(M, X, Y)
    assert rc == 0 and not (out == -7.0).any()
    for which, cols in ((0, n), (1, k), (2, k)):
        for mutate in ("late", "down", "col_high", "col_negative"):
            ops = [[a.copy() for a in op] for op in (M, X, Y)]
            if mutate == "late":
                ops[which][0][0] = 1
            elif mutate == "down":
                ops[which][0][1] = ops[which][0][2] + 1
            elif mutate == "col_high":
                ops[which][1][3] = cols
            else:
                ops[which][1][5] = -1
            rc, out = call(*ops)
            assert rc == INVALID and (out == -7.0).all(), (which, mutate)            # nothing is written
    for null in range(9):
        assert call(M, X, Y, null=(null,))[0] == INVALID, null
    assert call(M, X, Y, m=-1)[0] == INVALID and call(M, X, Y, k=-1)[0] == INVALID
    assert call(M, X, Y, n=int(M[1].max()))[0] == INVALID                            # the mask's largest column is out of range


def test_python_refusals_that_need_no_gpu(sblas):
    import torch
    m, n, k, M, X, Y = CASES["rect"]
    t = lambda a, dt=torch.int32: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
    rpm, cim, rpx, cix, rpy, ciy = t(M[0]), t(M[1]), t(X[0]), t(X[1]), t(Y[0]), t(Y[1])
    with pytest.raises(sblas.SblasError, match="GPU tensor"):
        sblas.MaskedSpgemmPlan(m, n, k, rpm, cim, rpx, cix, rpy, ciy)
    with pytest.raises(sblas.SblasError, match="int32"):
        sblas.MaskedSpgemmPlan(m, n, k, t(M[0], torch.int64), cim, rpx, cix, rpy, ciy)
    with pytest.raises(sblas.SblasError, match="int32"):
        sblas.MaskedSpgemmPlan(m, n, k, rpm, cim, rpx, cix, rpy, t(Y[1], torch.int64))
    with pytest.raises(sblas.SblasError, match="m \\+ 1"):
        sblas.MaskedSpgemmPlan(m + 1, n, k, rpm, cim, rpx, cix, rpy, ciy)
    with pytest.raises(sblas.SblasError, match="n \\+ 1"):
        sblas.MaskedSpgemmPlan(m, n, k, rpm, cim, rpx, cix, rpy[:-1].contiguous(), ciy)
    with pytest.raises(sblas.SblasError, match="contiguous"):
        sblas.MaskedSpgemmPlan(m, n, k, rpm, cim[::2], rpx, cix, rpy, ciy)
    with pytest.raises(sblas.SblasError, match="GPU tensor"):
        sblas.MaskedSpgemmPlan(m, n, k, M[0], cim, rpx, cix, rpy, ciy)               # a numpy array is no tensor
    fx, fy = t(X[2], torch.float64), t(Y[2], torch.float64)
    with pytest.raises(sblas.SblasError, match="the mask is"):
        sblas.masked_spgemm((m, n, rpm, cim), (m, k, rpx, cix, fx), (n, k + 1, rpy, ciy, fy))
    with pytest.raises(sblas.SblasError, match="GPU tensor"):
        sblas.masked_spgemm((m, n, rpm, cim), (m, k, rpx, cix, fx), (n, k, rpy, ciy, fy))
    with pytest.raises(sblas.SblasError):
        sblas.mspgemm_ref(m, n, k, M[0], M[1], X[0], X[1], X[2][:-1], Y[0], Y[1], Y[2])   # val_x shorter than colidx_x
    with pytest.raises(sblas.SblasError):
        sblas.mspgemm_ref(m + 1, n, k, M[0], M[1], X[0], X[1], X[2], Y[0], Y[1], Y[2])
    with pytest.raises(sblas.SblasError):
        sblas.mspgemm_ref(m, n, k, M[0], M[1][:-1], X[0], X[1], X[2], Y[0], Y[1], Y[2])   # the mask's rowptr ends beyond its colidx
    import sblas_amd.autograd as AG
    with pytest.raises(sblas.SblasError, match="GPU tensor"):
        AG.SpgemmOperator(m, k, n, rpx, cix, rpy, ciy)
    with pytest.raises(sblas.SblasError, match="SpgemmOperator"):
        AG.spgemm_multiply(None, fx, fy)
