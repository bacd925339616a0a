"""CPU-only checks of the row-major SpMM entry points (sblas_hip_spmm_csr_ordered & co.): their argument checks return
SBLAS_E_INVALID before anything touches a device, and spmm_tensor refuses layouts and types it cannot pass on."""
import ctypes as C

import pytest

INVALID, WORKSPACE = 1, 3
COL, ROW = 0, 1


def test_ordered_spmm_rejects_bad_arguments_without_a_gpu(sblas):
    L = sblas.lib()
    f = L.sblas_hip_spmm_csr_ordered
    one = C.c_void_p(16)          # never dereferenced: validation fails first

    def call(vt=0, it=0, rows=4, cols=6, nnz=3, rp=one, ci=one, v=one, B=one, ldb=6, ob=COL, n=5, Cm=one, ldc=4, oc=COL,
             ws=one, wsb=1 << 20):
        return f(-1, None, vt, it, rows, cols, nnz, rp, ci, v, B, ldb, ob, n, 1.0, 0.0, Cm, ldc, oc, ws, wsb)

    for vt, it in ((0, 0), (1, 0), (0, 1), (1, 1)):
        for bad in (-1, 2, 7):
            assert call(vt, it, ob=bad) == INVALID
            assert call(vt, it, oc=bad) == INVALID
            assert call(vt, it, ob=bad, rows=0) == INVALID          # the order is checked before the empty shortcut
        # row-major B needs ldb >= n, row-major C ldc >= n (column-major keeps ldb >= cols, ldc >= rows)
        assert call(vt, it, ob=ROW, ldb=4) == INVALID
        assert call(vt, it, oc=ROW, ldc=4) == INVALID
        assert call(vt, it, ob=COL, ldb=5) == INVALID
        assert call(vt, it, oc=COL, ldc=3) == INVALID
        assert call(vt, it, ob=ROW, ldb=5, oc=ROW, ldc=5, ws=None, wsb=0) == WORKSPACE   # exact minimums pass the checks
        # null pointers
        assert call(vt, it, rp=None) == INVALID
        assert call(vt, it, ci=None) == INVALID
        assert call(vt, it, v=None) == INVALID
        assert call(vt, it, ob=ROW, ldb=5, B=None) == INVALID
        assert call(vt, it, oc=ROW, ldc=5, Cm=None) == INVALID
        assert call(vt, it, rows=0, ob=ROW, oc=ROW, ldb=5, ldc=5) == 0    # empty: nothing to do
    assert call(vt=5) == INVALID and call(it=3) == INVALID


def test_ordered_planned_spmm_rejects_bad_arguments_without_a_gpu(sblas):
    L = sblas.lib()
    f = L.sblas_hip_spmm_csr_ordered_f64_i32_planned
    one = C.c_void_p(16)
    args = lambda ob, ldb, oc, ldc, B=one, Cm=one: (-1, None, 4, 6, 3, one, one, one, B, ldb, ob, 5, 1.0, 0.0, Cm, ldc, oc,
                                                    one, 1 << 20)
    assert f(None, *args(ROW, 5, ROW, 5)) == INVALID                      # no plan
    assert f(one, *args(2, 5, ROW, 5)) == INVALID                         # bad orders come back before the plan is read
    assert f(one, *args(ROW, 5, -1, 5)) == INVALID


def test_ordered_merge_rejects_bad_arguments_without_a_gpu(sblas):
    L = sblas.lib()
    f = L.sblas_hip_merge_rowblocks_ordered
    one = C.c_void_p(16)
    st = (C.c_int64 * 2)(0, 2)
    nr = (C.c_int64 * 2)(2, 2)
    ptrs = (C.c_void_p * 2)(16, 16)
    call = lambda vt=0, order=ROW, M=4, N=5, ldc=5, comm=one, s=st, r=nr, part=ptrs, Cs=ptrs: f(
        comm, vt, order, M, N, s, r, part, ptrs, 1.0, 0.0, Cs, ldc, None)
    for vt in (0, 1):
        assert call(vt, order=2) == INVALID
        assert call(vt, order=-1) == INVALID
        assert call(vt, order=ROW, ldc=4) == INVALID                       # row-major C: ldc >= N
        assert call(vt, order=COL, ldc=3) == INVALID                       # column-major C: ldc >= M
        assert call(vt, comm=None) == INVALID
        assert call(vt, s=None) == INVALID
        assert call(vt, r=None) == INVALID
        assert call(vt, part=None) == INVALID
        assert call(vt, Cs=None) == INVALID
    assert call(vt=4) == INVALID


def test_ordered_workspace_is_order_independent(sblas):
    L = sblas.lib()
    # one size serves every order pair: the typed workspace call has no order argument, and <f64, i32> is the tuned size
    assert L.sblas_hip_spmm_csr_workspace(0, 0, 10, 100, 5, 64) == L.sblas_hip_spmm_csr_f64_i32_workspace(10, 100, 5, 64)


def test_layout_of_tensor_views(sblas):
    import torch
    t = torch.zeros(6, 8, dtype=torch.float64)
    assert sblas._layout(t, 6, 8, "B") == (sblas.ROW_MAJOR, 8)
    assert sblas._layout(t.t(), 8, 6, "B") == (sblas.COL_MAJOR, 8)
    assert sblas._layout(t[:, 2:5], 6, 3, "B") == (sblas.ROW_MAJOR, 8)
    assert sblas._layout(t.t()[:, 1:4], 8, 3, "B") == (sblas.COL_MAJOR, 8)
    with pytest.raises(sblas.SblasError):
        sblas._layout(t[:, ::2], 6, 4, "B")                # column stride 2
    assert sblas._layout(t[::2, :], 3, 8, "B") == (sblas.ROW_MAJOR, 16)
    with pytest.raises(sblas.SblasError):
        sblas._layout(t.t()[::2, :], 4, 6, "B")            # row stride 2 of a column-major view
    with pytest.raises(sblas.SblasError):
        sblas._layout(t, 6, 7, "B")                        # wrong shape


def test_a_tensor_without_elements_has_no_strides_to_refuse(sblas):
    """an empty array that comes from numpy carries the strides (0, 0); torch calls it contiguous, and so does the library"""
    import numpy as np
    import torch
    for shape in ((0, 3), (3, 0), (0, 0)):
        t = torch.from_numpy(np.zeros(shape)).as_strided(shape, (0, 0))
        assert t.is_contiguous()
        assert sblas._layout(t, shape[0], shape[1], "B") == (sblas.ROW_MAJOR, max(shape[1], 1))
        assert sblas._layout(torch.zeros(shape, dtype=torch.float64), shape[0], shape[1], "B") == (sblas.ROW_MAJOR, max(shape[1], 1))


def test_spmm_tensor_rejects_strides_and_dtypes(sblas):
    import torch
    rp = torch.zeros(7, dtype=torch.int32)
    ci = torch.zeros(0, dtype=torch.int32)
    v = torch.zeros(0, dtype=torch.float64)
    A = (6, 8, rp, ci, v)
    B = torch.zeros(8, 4, dtype=torch.float64)
    Cm = torch.zeros(6, 4, dtype=torch.float64)
    for bad in ((6, 8, rp, ci, v.float()), (6, 8, rp.long(), ci.long(), v), (6, 8, rp, ci.long(), v)):
        with pytest.raises(sblas.SblasError, match="float64 values and int32 indices"):
            sblas.spmm_tensor(bad, B, Cm, 1.0, 0.0)
    with pytest.raises(sblas.SblasError, match="strides"):
        sblas.spmm_tensor(A, torch.zeros(8, 8, dtype=torch.float64)[:, ::2], Cm, 1.0, 0.0)
    with pytest.raises(sblas.SblasError, match="strides"):
        sblas.spmm_tensor(A, B, torch.zeros(6, 8, dtype=torch.float64)[:, ::2], 1.0, 0.0)
    with pytest.raises(sblas.SblasError, match="float64"):
        sblas.spmm_tensor(A, B.float(), Cm, 1.0, 0.0)
    with pytest.raises(sblas.SblasError, match="2-D"):
        sblas.spmm_tensor(A, B.reshape(-1), Cm, 1.0, 0.0)
    with pytest.raises(sblas.SblasError):
        sblas.spmm_tensor(A, B, Cm, 1.0, 0.0)              # CPU tensors: no CPU path
