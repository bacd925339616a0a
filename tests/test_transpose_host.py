"""CPU-only checks of the transposed products' entry points (sblas_hip_csr_transpose_f64_i32, sblas_hip_gather_f64, the
transpose plan): their argument checks return SBLAS_E_INVALID / SBLAS_E_WORKSPACE before anything touches a device, the
workspace size is monotone, and the Python wrappers refuse tensors they cannot pass on."""
import ctypes as C

import pytest

INVALID, WORKSPACE = 1, 3
COL, ROW = 0, 1
one = C.c_void_p(16)             # never dereferenced: validation fails first


def test_transpose_rejects_bad_arguments_without_a_gpu(sblas):
    L = sblas.lib()
    f = L.sblas_hip_csr_transpose_f64_i32
    need = L.sblas_hip_csr_transpose_workspace(4, 300, 7)
    assert need > 0

    def call(rows=4, cols=300, nnz=7, rp=one, ci=one, v=one, cp=one, ri=one, vt=one, pm=one, ws=one, wsb=need):
        return f(-1, None, rows, cols, nnz, rp, ci, v, cp, ri, vt, pm, ws, wsb)

    for kw in (dict(rows=-1), dict(cols=-1), dict(nnz=-1), dict(nnz=1 << 31), dict(cols=1 << 31), dict(rows=1 << 31)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(rp=None), dict(ci=None), dict(cp=None), dict(ri=None), dict(v=None), dict(vt=None)):
        assert call(**kw) == INVALID, kw                                  # val and valT: both or neither
    assert call(nnz=7, rows=0) == INVALID and call(nnz=7, cols=0) == INVALID   # no row / column to hold a nonzero
    assert call(ws=None) == WORKSPACE
    assert call(wsb=need - 1) == WORKSPACE
    assert call(ws=C.c_void_p(24)) == INVALID                             # 16-byte aligned workspace


def test_transpose_workspace_is_monotone(sblas):
    L = sblas.lib()
    ws = L.sblas_hip_csr_transpose_workspace
    assert ws(-1, 5, 5) == 0 and ws(5, -1, 5) == 0 and ws(5, 5, -1) == 0
    assert ws(5, 5, 0) == 0                        # no nonzeros: nothing to sort
    assert ws(5, 1, 5) == 0                        # one column: the CSR order is the CSC order
    prev = 0
    for nnz in (1, 2, 100, 4095, 4096, 4097, 10 ** 5, 10 ** 7, 2 ** 31 - 1):
        cur = ws(10, 1000, nnz)
        assert cur >= prev and cur >= 16 * nnz, nnz
        prev = cur
    prev = 0
    for cols in (0, 1, 2, 255, 256, 257, 1 << 16, (1 << 24) + 1, 2 ** 31 - 1):
        cur = ws(10, cols, 1000)
        assert cur >= prev, cols
        prev = cur


def test_gather_rejects_bad_arguments_without_a_gpu(sblas):
    f = sblas.lib().sblas_hip_gather_f64
    assert f(-1, None, -1, one, one, one) == INVALID
    assert f(-1, None, 5, None, one, one) == INVALID
    assert f(-1, None, 5, one, None, one) == INVALID
    assert f(-1, None, 5, one, one, None) == INVALID
    assert f(-1, None, 0, None, None, None) == 0


def test_plan_create_rejects_bad_arguments_without_a_gpu(sblas):
    L = sblas.lib()
    f = L.sblas_hip_transpose_plan_create
    h = C.c_void_p()

    def call(rows=4, cols=6, nnz=3, rp=one, ci=one, v=one, n=8, flags=0, out=C.byref(h)):
        return f(-1, None, rows, cols, nnz, rp, ci, v, n, flags, out)

    for kw in (dict(rows=-1), dict(cols=-1), dict(nnz=-1), dict(n=-1), dict(cols=2 ** 31 - 64), dict(nnz=1 << 31)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(rp=None), dict(ci=None), dict(v=None), dict(out=None), dict(flags=2), dict(flags=-1)):
        assert call(**kw) == INVALID, kw
    assert call(cols=0) == INVALID                 # nonzeros without a column
    assert not h.value


def test_plan_calls_reject_bad_arguments_without_a_gpu(sblas):
    L = sblas.lib()
    spmv, spmm = L.sblas_hip_spmv_csr_t_f64_i32_planned, L.sblas_hip_spmm_csr_t_f64_i32_planned
    assert spmv(None, -1, None, one, 1.0, 0.0, one) == INVALID
    args = lambda ob=COL, n=5, oc=COL: (-1, None, one, 8, ob, n, 1.0, 0.0, one, 8, oc, one, 1 << 20)
    assert spmm(None, *args()) == INVALID
    for bad in (-1, 2, 7):                          # orders and a negative width come back before the plan is read
        assert spmm(one, *args(ob=bad)) == INVALID
        assert spmm(one, *args(oc=bad)) == INVALID
    assert spmm(one, *args(n=-1)) == INVALID
    assert L.sblas_hip_transpose_plan_update_values(None, None, one) == INVALID
    out = (C.c_int64 * 8)()
    assert L.sblas_hip_transpose_plan_info(None, out) == INVALID
    assert L.sblas_hip_transpose_plan_csc(None, None, None, None) == INVALID
    assert L.sblas_hip_transpose_plan_destroy(None) == 0


def test_plan_of_a_matrix_without_columns_checks_shapes_without_a_gpu(sblas):
    """A 6 x 0 matrix: A^T has no rows, the plan holds nothing on the device, and the checks of A^T's shape still run
    (B is 6 x n: column-major ldb >= 6, row-major ldb >= n; C is 0 x n: row-major ldc >= n)."""
    L = sblas.lib()
    h = C.c_void_p()
    assert L.sblas_hip_transpose_plan_create(0, None, 6, 0, 0, one, None, None, 5, 0, C.byref(h)) == 0
    try:
        out = (C.c_int64 * 8)()
        assert L.sblas_hip_transpose_plan_info(h, out) == 0
        assert list(out) == [0, 0, 0, 0, 0, 0, 0, 0]
        spmm = L.sblas_hip_spmm_csr_t_f64_i32_planned
        call = lambda ldb=6, ob=COL, n=5, Cm=one, ldc=0, oc=COL, B=one: spmm(h, 0, None, B, ldb, ob, n, 1.0, 0.0, Cm, ldc, oc,
                                                                             None, 0)
        assert call() == 0                                                 # nothing to compute
        assert call(ldb=5) == INVALID                                      # column-major B: ldb >= rows of A
        assert call(ob=ROW, ldb=4) == INVALID                              # row-major B: ldb >= n
        assert call(ob=ROW, ldb=5) == 0
        assert call(oc=ROW, ldc=4) == INVALID                              # row-major C: ldc >= n
        assert call(B=None) == INVALID and call(Cm=None) == INVALID
        assert call(n=0, B=None, Cm=None) == 0
        spmv = L.sblas_hip_spmv_csr_t_f64_i32_planned
        assert spmv(h, 0, None, None, 1.0, 0.0, None) == INVALID           # x has rows entries
        assert spmv(h, 0, None, one, 1.0, 0.0, None) == 0                  # y has none
        assert L.sblas_hip_transpose_plan_update_values(h, None, None) == 0
    finally:
        assert L.sblas_hip_transpose_plan_destroy(h) == 0


def test_python_wrappers_refuse_wrong_tensors(sblas):
    import torch
    rp = torch.zeros(5, dtype=torch.int32)
    ci = torch.zeros(3, dtype=torch.int32)
    v = torch.zeros(3, dtype=torch.float64)
    with pytest.raises(sblas.SblasError):
        sblas.csr_transpose(4, 6, rp, ci, v)                               # CPU tensors: no CPU path
    with pytest.raises(sblas.SblasError, match="int32"):
        sblas.csr_transpose(4, 6, rp.long(), ci, v)
    with pytest.raises(sblas.SblasError, match="int32"):
        sblas.csr_transpose(4, 6, rp, ci.long(), v)
    with pytest.raises(sblas.SblasError, match="float64"):
        sblas.csr_transpose(4, 6, rp, ci, v.float())
    with pytest.raises(sblas.SblasError, match="contiguous"):
        sblas.csr_transpose(4, 6, rp, torch.zeros(6, dtype=torch.int32)[::2], v)
    with pytest.raises(sblas.SblasError, match="float64"):
        sblas.TransposePlan(4, 6, rp, ci, v.float())
    with pytest.raises(sblas.SblasError, match="contiguous"):
        sblas.TransposePlan(4, 6, rp, ci, torch.zeros(6, dtype=torch.float64)[::2])
    with pytest.raises(sblas.SblasError, match="int32"):
        sblas.gather(ci.long(), v, v)
