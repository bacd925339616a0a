"""Row-wise softmax on a CSR pattern without a GPU: the Decimal references against independent evaluations, the class
rules on hand-written rows, the inputs of the GPU tests against the conditions those tests rely on, the refusals that
return before the device is touched, the workspace size, and the Python layer's argument checks."""
import ctypes as C
import math
from decimal import Decimal, localcontext

import numpy as np
import pytest

import softmax_numerics as XN

INVALID, WORKSPACE = 1, 3


# ---- the references ------------------------------------------------------------------------------------------------
def test_forward_reference_on_the_five_row_pattern():
    rp, x = XN.small_pattern()
    for scale in (1.0, 0.125, -1.75):
        ref = XN.forward_reference(rp, x, scale)
        assert ref[1] == ([], [])                                    # the empty row
        assert ref[3][0] == [Decimal(1)]                             # a one-entry row is exactly 1
        assert ref[0][0][0] == ref[0][0][2]                          # duplicate values get one result
        for r, (p, d) in ref.items():
            if p:
                assert abs(sum(p) - 1) < Decimal(10) ** -55 and max(d) == 0
        # against the textbook form without the max shift, in Decimal: exp(t_i) / sum exp(t_j)
        with localcontext() as ctx:
            ctx.prec = 80
            t = [Decimal(float(v)) for v in XN.scaled(x, scale)]
            for r in range(5):
                e = [v.exp() for v in t[rp[r]:rp[r + 1]]]
                for a, b in zip(ref[r][0], e):
                    assert abs(a - b / sum(e)) < Decimal(10) ** -55
        # a plain float64 evaluation sits inside the bound
        res = XN.check_forward(XN.numpy_forward(rp, x, scale), rp, x, scale)
        assert res["ok"] and res["entries"] == 9, res


def test_backward_reference_is_the_derivative_of_the_forward_reference():
    rp, x = XN.small_pattern()
    rng = np.random.default_rng(0)
    dp = rng.uniform(-1, 1, len(x))
    scale = 0.75
    p = XN.numpy_forward(rp, x, scale)
    ref = XN.backward_reference(rp, p, dp, scale)
    assert ref[1] == ([], Decimal(0))
    h = Decimal(10) ** -20
    with localcontext() as ctx:
        ctx.prec = XN.PREC
        for r in (0, 2, 3, 4):
            lo, hi = rp[r], rp[r + 1]
            xs = [Decimal(float(v)) for v in x[lo:hi]]
            sc = Decimal(scale)
            # the backward of the EXACT softmax at these scores; p above is its float64 rounding, so the two agree to ~1e-15
            pe, _ = XN.forward_row_decimal([sc * v for v in xs])
            exact, _ = XN.backward_row_decimal(pe, [Decimal(float(v)) for v in dp[lo:hi]], sc)
            for j in range(hi - lo):                                  # column j of the Jacobian by central differences
                up, _ = XN.forward_row_decimal([sc * (v + (h if i == j else 0)) for i, v in enumerate(xs)])
                dn, _ = XN.forward_row_decimal([sc * (v - (h if i == j else 0)) for i, v in enumerate(xs)])
                fd = sum(((a - b) / (2 * h)) * Decimal(float(w)) for a, b, w in zip(up, dn, dp[lo:hi]))
                assert abs(fd - exact[j]) < Decimal(10) ** -30, (r, j)
                assert abs(ref[r][0][j] - exact[j]) < Decimal(10) ** -14
    res = XN.check_backward(XN.numpy_backward(rp, p, dp, scale), rp, p, dp, scale)
    assert res["ok"] and res["entries"] == 9, res
    res = XN.check_backward(XN.emulate_backward(rp, p, dp, scale), rp, p, dp, scale)
    assert res["ok"], res


def test_the_bounds_notice_an_error_of_a_few_hundred_ulps():
    rp, x = XN.small_pattern()
    got = XN.numpy_forward(rp, x, 1.0)
    bad = got.copy()
    bad[7] *= 1 + 400 * XN.U
    assert not XN.check_forward(bad, rp, x, 1.0)["ok"]
    dp = np.linspace(-1, 1, len(x))
    gb = XN.numpy_backward(rp, got, dp, 1.0)
    gb[0] += 400 * XN.U * abs(got[0])
    assert not XN.check_backward(gb, rp, got, dp, 1.0)["ok"]


def test_ordered_row_sum_is_the_documented_tree():
    # exact integers: any order gives the same sum; and one case where the order shows
    v = np.arange(1, 131, dtype=np.float64)
    assert XN.ordered_row_sum(v) == v.sum() == 130 * 131 / 2
    big = np.array([1.0, 2.0 ** -53, 2.0 ** -53, 0.0])
    assert XN.ordered_row_sum(big) == (1.0 + 2.0 ** -53) + (2.0 ** -53 + 0.0) == 1.0     # pairs first
    assert XN.ordered_row_sum(big[[1, 2, 0, 3]]) == 1.0 + 2.0 ** -52                     # the small pair meets first
    # cells and supercells: 4097 leaves = a supercell of 64 cells plus one leaf, added left to right
    w = np.random.default_rng(0).uniform(0, 1, 4097)
    cells = [XN.ordered_row_sum(w[i:i + 64]) for i in range(0, 4096, 64)]
    first = XN._fold64(np.array(cells))[0]
    assert XN.ordered_row_sum(w) == (0.0 + first) + w[4096]


def test_predicted_classes_on_hand_written_rows():
    inf, nan = np.inf, np.nan
    rows = [([1.0, nan, 2.0], [XN.NAN] * 3),                  # a NaN anywhere: the whole row
            ([1.0, -inf, 3.0], [XN.FINITE, XN.ZERO, XN.FINITE]),  # -Inf beside a finite entry: +0
            ([1.0, inf, -inf], [XN.NAN] * 3),                 # max +Inf
            ([-inf, -inf], [XN.NAN] * 2),                     # -Inf only
            ([-inf], [XN.NAN]),
            ([0.0, -800.0], [XN.FINITE] * 2),                 # underflow is ordinary
            ([], [])]
    x = np.array([v for r, _ in rows for v in r])
    rp = np.concatenate([[0], np.cumsum([len(r) for r, _ in rows])]).astype(np.int32)
    want = np.array([c for _, w in rows for c in w])
    assert (XN.predict_class(rp, x, 1.0) == want).all()
    assert (XN.predict_class(rp, x, 2.5) == want).all()
    # scale == 0 is no shortcut: 0 * Inf = NaN reaches rows 1 .. 4, row 0 keeps its NaN, row 5 is finite
    z = XN.predict_class(rp, x, 0.0)
    assert (z[:12] == XN.NAN).all() and (z[12:] == XN.FINITE).all()
    # a negative scale turns -Inf into the +Inf max
    assert (XN.predict_class(rp, x, -1.0)[3:6] == XN.NAN).all()
    with np.errstate(all="ignore"):
        got = np.array([nan, nan, nan, 0.1, 0.0, 0.9, nan, nan, nan, nan, nan, nan, 1.0, 0.0])
    assert len(XN.class_mismatches(want, got)) == 0
    got[4] = -0.0                                             # a -Inf entry gets +0, not -0
    assert list(XN.class_mismatches(want, got)) == [4]
    got[4], got[0] = 0.0, 0.5
    assert list(XN.class_mismatches(want, got)) == [0]


# ---- the GPU tests' inputs meet the conditions those tests rely on -------------------------------------------------
@pytest.mark.parametrize("name", ["small", "mixed", "ash85", "banded", "powerlaw", "nd24k_slice"])
def test_general_inputs_have_a_spread_of_at_most_60_and_no_subnormal_output(name):
    rp = XN.pattern(name)
    lens = np.diff(rp.astype(np.int64))
    rows = XN.sample_rows(rp)
    assert int(lens.argmax()) in rows
    if name in ("banded", "powerlaw", "nd24k_slice", "mixed"):
        assert any(lens[r] == 1 for r in rows)
    if name == "powerlaw":
        assert lens.max() >= 10 ** 5
    for scale in (1.0, 0.125):
        x = XN.scores(rp, seed=3, scale=scale)
        t = XN.scaled(x, scale)
        hi = np.maximum.reduceat(t, rp[:-1][lens > 0])
        lo = np.minimum.reduceat(t, rp[:-1][lens > 0])
        assert (hi - lo).max() <= 60.0
        if scale == 0.125 and name in ("powerlaw", "mixed"):
            continue                                           # the Decimal pass over the long row once is enough
        ref = XN.forward_reference(rp, x, scale, rows)
        smallest = min((min(p) for p, _ in ref.values() if p))
        assert smallest >= Decimal(2) ** -1022
        # a plain numpy evaluation meets the relative bound and the row-sum condition on these inputs
        res = XN.check_forward(XN.numpy_forward(rp, x, scale), rp, x, scale, rows)
        assert res["ok"], res


def test_wide_row_underflows_and_a_plain_evaluation_meets_the_absolute_bound():
    rp, x = XN.wide_row()
    assert x.max() - x.min() == 1500.0
    ref = XN.forward_reference(rp, x, 1.0)[0][0]
    assert min(ref) < Decimal(2) ** -1080 and sum(1 for p in ref if p < Decimal(2) ** -1022) > 100
    got = XN.numpy_forward(rp, x, 1.0)
    assert (got == 0.0).sum() > 100
    res = XN.check_forward(got, rp, x, 1.0, absolute=True)
    assert res["ok"], res
    assert not XN.check_forward(got, rp, x, 1.0, absolute=False)["ok"]      # the relative form alone cannot hold here


# ---- the C ABI -----------------------------------------------------------------------------------------------------
def test_refusals_return_before_the_device_is_touched(sblas):
    L = sblas.lib()
    fwd, bwd = L.sblas_hip_csr_softmax_f64_i32, L.sblas_hip_csr_softmax_backward_f64_i32
    one = C.c_void_p(16)                          # never dereferenced: validation fails first
    rows, nnz = 6, 5000
    need = L.sblas_hip_csr_softmax_workspace(rows, nnz)
    assert need > 0
    big = 1 << 20

    def f(rows_=rows, nnz_=nnz, rowptr=one, x=one, out=one, ws=one, wsb=big):
        return fwd(-1, None, rows_, nnz_, rowptr, x, 1.0, out, ws, wsb)

    def b(rows_=rows, nnz_=nnz, rowptr=one, p=one, dp=one, dx=one, ws=one, wsb=big):
        return bwd(-1, None, rows_, nnz_, rowptr, p, dp, 1.0, dx, ws, wsb)

    for missing in ("rowptr", "x", "out"):
        assert f(**{missing: None}) == INVALID, missing
    for missing in ("rowptr", "p", "dp", "dx"):
        assert b(**{missing: None}) == INVALID, missing
    for call in (f, b):
        assert call(rows_=-1) == INVALID and call(nnz_=-1) == INVALID
        assert call(nnz_=2 ** 31) == INVALID and call(rows_=2 ** 31) == INVALID      # int32 row pointers
        assert call(ws=None, wsb=0) == WORKSPACE
        assert call(ws=None, wsb=big) == WORKSPACE
        assert call(ws=one, wsb=need - 1) == WORKSPACE
        assert call(ws=C.c_void_p(24), wsb=need) == INVALID                           # not 16-byte aligned
        assert call(rows_=0, nnz_=3) == INVALID                                        # entries, no rows
        assert call(rows_=0, nnz_=nnz) == INVALID
    # nothing to do: valid, and nothing is launched (no pointer but rowptr is looked at, and that only for NULL)
    assert fwd(-1, None, rows, 0, one, None, 1.0, None, None, 0) == 0
    assert bwd(-1, None, rows, 0, one, None, None, 1.0, None, None, 0) == 0
    assert fwd(-1, None, 0, 0, one, None, 1.0, None, None, 0) == 0
    assert bwd(-1, None, 0, 0, one, None, None, 1.0, None, None, 0) == 0


def test_workspace_follows_rows_and_nnz_only_and_is_a_multiple_of_16(sblas):
    W = sblas.csr_softmax_workspace_bytes
    assert W(0, 0) == 0 and W(10, 0) == 0 and W(0, 10 ** 6) == 0 and W(5, 4096) == 0
    prev = 0
    for nnz in (4097, 5000, 10 ** 5, 10 ** 6, 28728000, 2 ** 31 - 1):
        w = W(1000, nnz)
        assert w > 0 and w % 16 == 0 and w >= prev
        assert w <= nnz // 100 + 128                      # partial results of supercells, not a copy of the values
        assert W(1000, nnz) == w                          # a function: the same again
        prev = w
    assert W(1, 10 ** 6) == W(10 ** 6, 10 ** 6)           # long rows are found by position, not counted by rows


# ---- the Python layer ----------------------------------------------------------------------------------------------
def test_csr_softmax_rejects_what_no_kernel_reads(sblas):
    import torch
    rp, x = XN.small_pattern()
    R, X = torch.from_numpy(rp), torch.from_numpy(x)
    E = sblas.SblasError
    with pytest.raises(E, match="GPU tensor"):
        sblas.csr_softmax(R, X)                                                  # CPU tensors
    with pytest.raises(E, match="GPU tensor"):
        sblas.csr_softmax_backward(R, X, X)
    with pytest.raises(E, match="float64"):
        sblas.csr_softmax(R, X.float())
    with pytest.raises(E, match="int32"):
        sblas.csr_softmax(R.long(), X)
    with pytest.raises(E, match="rowptr"):
        sblas.csr_softmax(rp, X)                                                 # a numpy array
    with pytest.raises(E, match="one value per stored entry"):
        sblas.csr_softmax(R, X, torch.empty(X.numel() + 1, dtype=torch.float64))  # x and out of different length
    with pytest.raises(E, match="one value per stored entry"):
        sblas.csr_softmax(R, X, X[:-1])
    with pytest.raises(E, match="one value per stored entry"):
        sblas.csr_softmax(R, X, X.reshape(1, -1))                                # not 1-D
    with pytest.raises(E, match="one value per stored entry"):
        sblas.csr_softmax_backward(R, X, X[:-1])                                 # p and dp
    with pytest.raises(E, match="one value per stored entry"):
        sblas.csr_softmax_backward(R, X, X, torch.empty(X.numel() - 1, dtype=torch.float64))
    with pytest.raises(E):
        sblas.csr_softmax(R, x)
    for name in ("sblas_hip_csr_softmax_workspace", "sblas_hip_csr_softmax_f64_i32", "sblas_hip_csr_softmax_backward_f64_i32"):
        assert name in sblas.EXPORTS


def test_csr_operator_softmax_and_sddmm_reject_wrong_arguments(sblas):
    import torch
    from sblas_amd.autograd import CsrOperator
    rows, cols, nnz = 5, 4, 9
    E = sblas.SblasError
    op = CsrOperator.__new__(CsrOperator)                                        # the checks of a made operator, without a device
    op.rows, op.cols, op.nnz = rows, cols, nnz
    Z = lambda *shape: torch.zeros(*shape, dtype=torch.float64)
    with pytest.raises(E, match="GPU"):
        op.softmax(Z(nnz))
    with pytest.raises(E, match="GPU"):
        op.softmax(np.zeros(nnz))
    with pytest.raises(E, match="GPU"):
        op.sddmm(Z(rows, 3), Z(cols, 3))
    with pytest.raises(E):
        op.sddmm(np.zeros((rows, 3)), Z(cols, 3))
