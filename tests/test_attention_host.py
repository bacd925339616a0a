"""Fused attention on a CSR pattern without a GPU: the exact reference and the bound of attention_numerics against
independent evaluations, the inputs of the GPU tests, the refusals that return before the device is touched, the
workspace size, and the Python layer's argument checks."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import attention_numerics as AN

INVALID, WORKSPACE = 1, 3


# ---- the reference and the bound -----------------------------------------------------------------------------------
def test_exact_weighted_sum_agrees_with_fractions():
    rng = np.random.default_rng(0)
    w = rng.uniform(-1, 1, 9) * np.exp2(rng.integers(-40, 40, 9))
    Y = rng.uniform(-1, 1, (9, 4)) * np.exp2(rng.integers(-30, 30, (9, 4)))
    w[3], Y[5, 2] = 0.0, 2.0 ** -1070                                  # a zero and a subnormal
    ref, mag = AN.exact_weighted_sum(w, Y)
    for c in range(4):
        assert ref[c] == sum(Fraction(float(a)) * Fraction(float(b)) for a, b in zip(w, Y[:, c]))
        assert mag[c] == sum(abs(Fraction(float(a)) * Fraction(float(b))) for a, b in zip(w, Y[:, c]))
    assert AN.exact_weighted_sum(w[:0], Y[:0]) == ([Fraction(0)] * 4, [Fraction(0)] * 4)


def test_bound_factor_counts_the_supercell_folds():
    u = Fraction(1, 2 ** 53)
    assert AN.bound_factor(1) == AN.gamma(4) == 4 * u / (1 - 4 * u)
    assert AN.bound_factor(4096) == AN.gamma(4099) and AN.bound_factor(4097) == AN.gamma(4101)
    assert AN.bound_factor(0) == AN.gamma(2)


@pytest.mark.parametrize("name", ["small", "edges"])
def test_a_plain_evaluation_meets_the_bound_and_a_few_hundred_ulps_do_not(name):
    rows, cols, rp, ci = AN.pattern(name)
    Q, K, V, dO = AN.operands(rows, cols, 5, 3)
    V = np.abs(V) + 0.5                                                  # no cancellation: |O| is the sum of the magnitudes
    O, P, m, z = AN.numpy_attention(rp, ci, Q, K, V, 0.125)
    sample = AN.sample_rows(rp)
    lens = np.diff(rp.astype(np.int64))
    assert int(lens.argmax()) in sample and any(lens[r] == 0 for r in sample)
    res = AN.check_rows(O, rp, ci, P, V, sample)
    assert res["ok"] and res["outputs"] == 3 * len(sample), res
    short = min((r for r in sample if lens[r] > 0), key=lambda r: lens[r])
    bad = O.copy()
    bad[short, 1] *= 1 + 400 * 2.0 ** -53
    res = AN.check_rows(bad, rp, ci, P, V, sample)
    assert not res["ok"] and res["where"] == (short, 1), res
    if name == "edges":                                                  # on the longest row the bound is ~12000 u wide:
        long = int(lens.argmax())                                        # an error of 3 L u shows, one of 400 u cannot
        bad = O.copy()
        bad[long, 0] *= 1 + 3 * int(lens[long]) * 2.0 ** -53
        assert not AN.check_rows(bad, rp, ci, P, V, [long])["ok"]
    # an empty row: exactly zero, and nothing else passes
    empty = int(np.flatnonzero(lens == 0)[0])
    assert (O[empty] == 0).all()
    bad = O.copy()
    bad[empty, 0] = 2.0 ** -1060
    assert not AN.check_rows(bad, rp, ci, P, V, [empty])["ok"]


def test_the_patterns_are_what_the_gpu_tests_rely_on():
    rows, cols, rp, ci = AN.pattern("small")
    assert (rows, cols) == (12, 9) and (np.diff(rp) == 0).sum() == 2
    rows, cols, rp, ci = AN.pattern("edges")
    lens = np.diff(rp.astype(np.int64))
    assert list(lens[:3]) == [0, 1, 2] and lens.max() == 12353 and cols == 600
    assert 0.9e5 < rp[-1] < 1.2e5 and ci.max() < cols and len(np.unique(ci[rp[-2]:])) < lens[-1]     # repeats
    for edge in (512, 513, 4096, 4097, 8192, 8193):                      # both sides of every change of path
        assert edge in lens
    rows, cols, rp, ci = AN.pattern("big")
    lens = np.diff(rp.astype(np.int64))
    assert rows == 20000 and lens[17] == 9000 and (lens == 0).sum() > 1000
    assert AN.pattern("big")[2] is rp                                    # made once
    # scores stay small: no probability underflows, so the classes of O are those of the sums
    Q, K, V, dO = AN.operands(rows, cols, 128, 128)
    assert np.abs(Q).max() < 1 and np.abs(K).max() < 1


# ---- the C ABI -----------------------------------------------------------------------------------------------------
def test_refusals_return_before_the_device_is_touched(sblas):
    L = sblas.lib()
    fwd, bwd = L.sblas_hip_csr_attention_f64_i32, L.sblas_hip_csr_attention_backward_f64_i32
    one = C.c_void_p(16)                          # never dereferenced: validation fails first
    rows, cols, nnz = 6, 7, 5000
    need = L.sblas_hip_csr_attention_workspace(rows, nnz, 8, 4)
    assert need > 0
    big = 1 << 24
    base = dict(rows=rows, cols=cols, nnz=nnz, rowptr=one, colidx=one, Q=one, ldq=8, K=one, ldk=8, V=one, ldv=4, d=8, dv=4,
                ws=one, wsb=big)

    def f(O=one, ldo=4, row_max=one, row_sum=one, **kw):
        a = dict(base, **kw)
        return fwd(-1, None, a["rows"], a["cols"], a["nnz"], a["rowptr"], a["colidx"], a["Q"], a["ldq"], a["K"], a["ldk"], a["V"],
                   a["ldv"], a["d"], a["dv"], 1.0, O, ldo, row_max, row_sum, a["ws"], a["wsb"])

    def b(dO=one, lddo=4, row_max=one, row_sum=one, dQ=one, lddq=8, P=one, dS=one, **kw):
        a = dict(base, **kw)
        return bwd(-1, None, a["rows"], a["cols"], a["nnz"], a["rowptr"], a["colidx"], a["Q"], a["ldq"], a["K"], a["ldk"], a["V"],
                   a["ldv"], a["d"], a["dv"], 1.0, dO, lddo, row_max, row_sum, dQ, lddq, P, dS, a["ws"], a["wsb"])

    for call in (f, b):
        for missing in ("rowptr", "colidx", "Q", "K", "V"):
            assert call(**{missing: None}) == INVALID, missing
        for width in ("d", "dv"):
            assert call(**{width: 0}) == INVALID and call(**{width: 129}) == INVALID and call(**{width: -1}) == INVALID
        assert call(d=128, ldq=128, ldk=128, lddq=128, ws=None, wsb=0) == WORKSPACE          # 128 is inside the limits
        assert call(ldq=7) == INVALID and call(ldk=7) == INVALID and call(ldv=3) == INVALID
        assert call(rows=-1) == INVALID and call(cols=-1) == INVALID and call(nnz=-1) == INVALID
        assert call(nnz=2 ** 31) == INVALID and call(rows=2 ** 31) == INVALID
        assert call(rows=0) == INVALID and call(cols=0) == INVALID                 # entries without a place
        assert call(ws=None, wsb=0) == WORKSPACE and call(ws=None, wsb=big) == WORKSPACE
        assert call(wsb=need - 1) == WORKSPACE
        assert call(ws=C.c_void_p(24), wsb=need) == INVALID                        # not 16-byte aligned
    assert f(O=None) == INVALID and f(ldo=3) == INVALID
    assert f(row_max=None) == INVALID and f(row_sum=None) == INVALID               # both or neither
    assert b(row_max=None) == INVALID and b(row_sum=None) == INVALID
    assert b(dO=None) == INVALID and b(lddo=3) == INVALID and b(lddq=7) == INVALID
    assert b(dO=None, dQ=None, P=one, dS=one) == INVALID                           # dS needs dO too
    # nothing to do: valid, nothing launched
    assert f(rows=0, nnz=0, ws=None, wsb=0) == 0 and b(rows=0, nnz=0, ws=None, wsb=0) == 0
    assert b(dO=None, dQ=None, P=None, dS=None) == 0                               # nothing asked for


def test_workspace_follows_rows_nnz_d_dv_only_and_is_a_multiple_of_16(sblas):
    W = sblas.csr_attention_workspace_bytes
    assert W(0, 0, 8, 8) == 0 and W(10, 0, 8, 8) == 0 and W(0, 10 ** 6, 8, 8) == 0 and W(5, 4096, 128, 128) == 0
    assert W(2048, 2 ** 20, 8, 8) < 2 ** 20
    prev = 0
    for nnz in (4097, 5000, 10 ** 5, 10 ** 6, 28728000, 2 ** 31 - 1):
        w = W(1000, nnz, 64, 64)
        assert w > 0 and w % 16 == 0 and w >= prev and W(1000, nnz, 64, 64) == w
        # partial rows of supercells, never a copy of the values: ceil(nnz / 4096) * (width + 2), twice, plus two slots
        assert w <= 2 * (nnz // 4096 + 2) * (64 + 2) * 8 + 16
        prev = w
    for nnz in (5000, 10 ** 6):
        sizes = [W(1000, nnz, d, dv) for d, dv in ((1, 1), (8, 8), (64, 16), (16, 64), (64, 64), (64, 128), (128, 128))]
        assert all(s % 16 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[2] == sizes[3]
    assert W(1, 10 ** 6, 8, 8) == W(10 ** 6, 10 ** 6, 8, 8)      # long rows are found by position, not counted by rows


# ---- the Python layer ----------------------------------------------------------------------------------------------
def test_csr_attention_rejects_what_no_kernel_reads(sblas):
    import torch
    rows, cols, rp, ci = AN.pattern("small")
    R, Ci = torch.from_numpy(np.array(rp)), torch.from_numpy(np.array(ci))
    Z = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    A = (rows, cols, R, Ci)
    E = sblas.SblasError
    with pytest.raises(E, match="GPU tensor"):
        sblas.csr_attention(A, Z(rows, 4), Z(cols, 4), Z(cols, 3))                    # CPU tensors
    with pytest.raises(E, match="GPU tensor"):
        sblas.csr_attention_backward(A, Z(rows, 4), Z(cols, 4), Z(cols, 3), Z(rows, 3), Z(rows), Z(rows), dQ=Z(rows, 4))
    with pytest.raises(E, match="float64"):
        sblas.csr_attention(A, Z(rows, 4).float(), Z(cols, 4), Z(cols, 3))
    with pytest.raises(E, match="int32"):
        sblas.csr_attention((rows, cols, R.long(), Ci), Z(rows, 4), Z(cols, 4), Z(cols, 3))
    with pytest.raises(E, match="K must be"):
        sblas.csr_attention(A, Z(rows, 4), Z(cols, 5), Z(cols, 3))                    # d of Q and K differ
    with pytest.raises(E, match="Q must be"):
        sblas.csr_attention(A, Z(rows + 1, 4), Z(cols, 4), Z(cols, 3))
    with pytest.raises(E, match="out must be"):
        sblas.csr_attention(A, Z(rows, 4), Z(cols, 4), Z(cols, 3), out=Z(rows, 4))
    with pytest.raises(E, match="1 .. 128"):
        sblas.csr_attention(A, Z(rows, 129), Z(cols, 129), Z(cols, 3))
    with pytest.raises(E, match="row-major"):
        sblas.csr_attention(A, Z(4, rows).t(), Z(cols, 4), Z(cols, 3))
    with pytest.raises(E, match="both or neither"):
        sblas.csr_attention(A, Z(rows, 4), Z(cols, 4), Z(cols, 3), row_max=Z(rows))
    with pytest.raises(E, match="rowptr"):
        sblas.csr_attention((rows + 1, cols, R, Ci), Z(rows + 1, 4), Z(cols, 4), Z(cols, 3))
    with pytest.raises(E, match="dO must be"):
        sblas.csr_attention_backward(A, Z(rows, 4), Z(cols, 4), Z(cols, 3), Z(rows, 4), Z(rows), Z(rows), dQ=Z(rows, 4))
    with pytest.raises(E, match="one value per stored entry"):
        sblas.csr_attention_backward(A, Z(rows, 4), Z(cols, 4), Z(cols, 3), Z(rows, 3), Z(rows), Z(rows), P=Z(len(ci) + 1))
    for name in ("sblas_hip_csr_attention_workspace", "sblas_hip_csr_attention_f64_i32", "sblas_hip_csr_attention_backward_f64_i32"):
        assert name in sblas.EXPORTS


def test_csr_operator_attention_rejects_wrong_arguments(sblas):
    import torch
    from sblas_amd.autograd import CsrOperator
    rows, cols, nnz = 5, 4, 9
    E = sblas.SblasError
    op = CsrOperator.__new__(CsrOperator)                                        # the checks of a made operator, without a device
    op.rows, op.cols, op.nnz = rows, cols, nnz
    Z = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    with pytest.raises(E, match="GPU"):
        op.attention(Z(rows, 3), Z(cols, 3), Z(cols, 2))
    with pytest.raises(E, match="GPU"):
        op.attention(np.zeros((rows, 3)), Z(cols, 3), Z(cols, 2))
    assert "composition" in CsrOperator.attention.__doc__ and "128" in CsrOperator.attention.__doc__
