"""SDDMM without a GPU: the numerics helper against rationals, the refusals that return before the device is touched, the
workspace sizes, and the Python layer's argument checks."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import sddmm_numerics as SN

ROW, COL = 1, 0
INVALID, WORKSPACE = 1, 3


def small_pattern():
    # 5 x 4: unsorted columns, a duplicate (row 0 lists column 2 twice), an empty row
    rp = np.array([0, 3, 3, 5, 6, 9], np.int32)
    ci = np.array([2, 0, 2, 3, 1, 0, 3, 2, 1], np.int32)
    return 5, 4, rp, ci


@pytest.mark.parametrize("k", [0, 1, 2, 5, 16, 33])
def test_double_double_reference_and_bound_against_rationals(k):
    rows, cols, rp, ci = small_pattern()
    rng = np.random.default_rng(k)
    X = SN.log_uniform(rng, (rows, k), 30)
    Y = SN.log_uniform(rng, (cols, k), 30)
    old = SN.log_uniform(rng, len(ci), 30)
    for alpha, beta in ((1.0, 0.0), (-1.75, 0.3), (0.5, 1.0)):
        exact = SN.exact_fraction(rp, ci, X, Y, old, alpha, beta)
        hi, lo = SN.reference_dd(rp, ci, X, Y, old, alpha, beta)
        r, c = SN.entry_rows(rp, ci)
        mag = [abs(Fraction(alpha)) * sum((abs(Fraction(float(a)) * Fraction(float(b))) for a, b in zip(X[r[e]], Y[c[e]])), Fraction(0)) +
               abs(Fraction(beta) * Fraction(float(old[e]))) for e in range(len(ci))]
        for e in range(len(ci)):
            err = abs(Fraction(float(hi[e])) + Fraction(float(lo[e])) - exact[e])
            assert err <= mag[e] * Fraction(1, 2 ** 95) + Fraction(1, 2 ** 1070), (k, e)
        bnd = SN.bound(rp, ci, X, Y, old, alpha, beta)
        assert all(Fraction(float(bnd[e])) >= Fraction(float(SN.gamma(k + 2, np.float64))) * mag[e] for e in range(len(ci)))
        # a plain float64 evaluation in two orders stays inside the bound
        for order in (slice(None), slice(None, None, -1)):
            got = np.array([alpha * sum(float(a) * float(b) for a, b in zip(X[r[e]][order], Y[c[e]][order])) +
                            (beta * old[e] if beta else 0.0) for e in range(len(ci))])
            ok, worst, _, _ = SN.check_bound(got, (hi, lo), bnd)
            assert ok and worst < 1.0


@pytest.mark.parametrize("k", [0, 1, 3, 64, 300])
def test_exact_grid_is_exact_in_any_order(k):
    rows, cols, rp, ci = small_pattern()
    for alpha, beta in ((1.0, 0.0), (-2.0, 0.5), (0.5, 1.0)):
        g = SN.grid_problem(rp, ci, rows, cols, k, alpha, beta, seed=k)
        exact = SN.exact_fraction(rp, ci, g.X, g.Y, g.old, alpha, beta)
        assert all(Fraction(float(v)) == f for v, f in zip(g.expected, exact))
        r, c = SN.entry_rows(rp, ci)
        fwd = alpha * (g.X[r] * g.Y[c]).sum(axis=1) + (beta * g.old if beta else 0.0)
        bwd = alpha * (g.X[r][:, ::-1] * g.Y[c][:, ::-1]).sum(axis=1) + (beta * g.old if beta else 0.0)
        assert (fwd == g.expected).all() and (bwd == g.expected).all()


def test_predicted_classes():
    rows, cols, rp, ci = small_pattern()
    X = np.ones((rows, 3))
    Y = np.ones((cols, 3))
    old = np.zeros(len(ci))
    X[0, 1] = np.inf          # row 0: +Inf everywhere ...
    Y[0, 1] = 0.0             # ... but 0 * Inf = NaN against column 0
    Y[3, 2] = -np.inf         # column 3: -Inf; with row 0's +Inf: NaN
    old[4] = np.nan
    want0 = SN.predict_class(rp, ci, X, Y, old, 1.0, 0.0)
    assert list(want0) == [2, 1, 2, 3, 0, 0, 3, 0, 0]
    assert SN.predict_class(rp, ci, X, Y, old, 1.0, 0.5)[4] == 1
    assert list(SN.predict_class(rp, ci, X, Y, old, -1.0, 0.0)[:4]) == [3, 1, 3, 2]


def test_refusals_return_before_the_device_is_touched(sblas):
    L = sblas.lib()
    f = L.sblas_hip_sddmm_csr_f64_i32
    one = C.c_void_p(16)                          # never dereferenced: validation fails first
    rows, cols, nnz, k = 6, 9, 5, 4
    big = 1 << 20
    ok_args = dict(ldx=k, ox=ROW, ldy=k, oy=ROW)

    def call(rowptr=one, colidx=one, X=one, Y=one, out=one, ws=one, wsb=big, k_=k, nnz_=nnz, **kw):
        a = dict(ok_args, **kw)
        return f(-1, None, rows, cols, nnz_, rowptr, colidx, X, a["ldx"], a["ox"], Y, a["ldy"], a["oy"], k_, 1.0, 0.0, out, ws, wsb)

    for bad in (-1, 2, 7):
        assert call(ox=bad) == INVALID and call(oy=bad) == INVALID
    assert call(ldx=k - 1) == INVALID and call(ldy=k - 1) == INVALID                      # row-major: ld >= k
    assert call(ox=COL, ldx=rows - 1) == INVALID and call(oy=COL, ldy=cols - 1) == INVALID  # column-major: ld >= rows / cols
    assert call(oy=COL, ldy=rows) == INVALID                                               # Y's minimum is cols, not rows
    for missing in ("rowptr", "colidx", "X", "Y", "out"):
        assert call(**{missing: None}) == INVALID, missing
    assert call(k_=-1) == INVALID and call(nnz_=-1) == INVALID
    # a column-major operand needs the workspace: missing, or one byte short
    for kw in (dict(ox=COL, ldx=rows), dict(oy=COL, ldy=cols), dict(ox=COL, ldx=rows, oy=COL, ldy=cols)):
        need = L.sblas_hip_sddmm_csr_workspace(rows, cols, nnz, k, kw.get("ox", ROW), kw.get("oy", ROW))
        assert need > 0
        assert call(ws=None, wsb=0, **kw) == WORKSPACE
        assert call(ws=one, wsb=need - 1, **kw) == WORKSPACE
        assert call(ws=C.c_void_p(24), wsb=need, **kw) == INVALID                          # not 16-byte aligned
    # nothing to do: valid, and nothing is launched (no pointer is read)
    assert f(-1, None, rows, cols, 0, one, None, None, k, ROW, None, k, ROW, k, 1.0, 0.0, None, None, 0) == 0
    assert f(-1, None, 0, 0, 0, one, None, None, k, ROW, None, k, ROW, k, 1.0, 0.0, None, None, 0) == 0
    assert f(-1, None, 0, cols, 3, one, one, one, k, ROW, one, k, ROW, k, 1.0, 0.0, one, None, 0) == INVALID   # entries, no rows


def test_workspace_is_zero_for_row_major_and_grows_only_with_column_major_operands(sblas):
    W = sblas.sddmm_workspace_bytes
    rows, cols, nnz = 1000, 3000, 5000
    for k in (1, 8, 9, 33, 64, 100, 300):
        assert W(rows, cols, nnz, k, ROW, ROW) == 0
        wx, wy, wxy = W(rows, cols, nnz, k, COL, ROW), W(rows, cols, nnz, k, ROW, COL), W(rows, cols, nnz, k, COL, COL)
        assert wx >= (rows + 1) * k * 8 and wy >= (cols + 1) * k * 8 and wxy == wx + wy
        assert wx < wy                                           # each part follows its own operand's rows
        assert wx % 16 == 0 and wy % 16 == 0
        assert W(rows, 2 * cols, nnz, k, COL, ROW) == wx and W(2 * rows, cols, nnz, k, ROW, COL) == wy
    assert W(rows, cols, nnz, 0, COL, COL) == 0 and W(rows, cols, 0, 8, COL, COL) == 0
    assert sblas.sddmm_workspace_bytes(rows, cols, nnz, 8) == 0  # the default orders are row-major


def test_sddmm_tensor_rejects_what_no_kernel_reads(sblas):
    import torch
    rows, cols, rp, ci = small_pattern()
    R, Cx = torch.from_numpy(rp), torch.from_numpy(ci)
    A = (rows, cols, R, Cx)
    X = torch.zeros(rows, 4, dtype=torch.float64)
    Y = torch.zeros(cols, 4, dtype=torch.float64)
    out = torch.zeros(len(ci), dtype=torch.float64)
    E = sblas.SblasError
    with pytest.raises(E, match="GPU tensor"):
        sblas.sddmm_tensor(A, X, Y, out)                                         # CPU tensors
    with pytest.raises(E, match="float64"):
        sblas.sddmm_tensor(A, X.float(), Y, out)
    with pytest.raises(E, match="int32"):
        sblas.sddmm_tensor((rows, cols, R.long(), Cx), X, Y, out)
    with pytest.raises(E, match="2-D"):
        sblas.sddmm_tensor(A, X[:, 0], Y, out)
    Z = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    for Xb, Yb in ((Z(rows + 1, 4), Z(cols, 4)), (Z(rows, 4), Z(cols, 5)), (Z(cols, 4), Z(cols, 4))):
        with pytest.raises(E, match="got shape"):
            sblas.sddmm_tensor(A, Xb, Yb, out)
    with pytest.raises(E, match="strides"):
        Xs = torch.zeros(rows, 8, dtype=torch.float64)[:, ::2]                   # strides (8, 2)
        sblas.sddmm_tensor(A, Xs, Y, out)


def test_csr_operator_rejects_wrong_arguments(sblas):
    import torch
    from sblas_amd.autograd import CsrOperator
    rows, cols, rp, ci = small_pattern()
    E = sblas.SblasError
    with pytest.raises(E, match="GPU"):
        CsrOperator(rows, cols, torch.from_numpy(rp), torch.from_numpy(ci))
    with pytest.raises(E):
        CsrOperator(rows, cols, rp, ci)                                          # numpy arrays
    op = CsrOperator.__new__(CsrOperator)                                        # the checks of a made operator, without a device
    op.rows, op.cols, op.nnz = rows, cols, len(ci)
    val = torch.zeros(len(ci), dtype=torch.float64)
    with pytest.raises(E, match="GPU"):
        op.matmul(val, torch.zeros(cols, 3, dtype=torch.float64))
    with pytest.raises(E, match="GPU"):
        op.matvec(val, torch.zeros(cols, dtype=torch.float64))
    for bad in (torch.zeros(len(ci) + 1, dtype=torch.float64), torch.zeros(len(ci), dtype=torch.float32)):
        with pytest.raises(E):
            op._check_val(bad)
