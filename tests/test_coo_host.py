"""CPU-only checks of the COO -> CSR entry points (sblas_hip_coo_to_csr_f64_i32, the assembly plan): their argument checks
return SBLAS_E_INVALID / SBLAS_E_WORKSPACE before anything touches a device, the workspace size is monotone, the Python
wrappers refuse tensors they cannot pass on, and coo_from_torch extracts the triplets of a sparse tensor as stored."""
import ctypes as C

import numpy as np
import pytest

INVALID, WORKSPACE = 1, 3
KEEP, SUM = 0, 1
one = C.c_void_p(16)             # never dereferenced: validation fails first


def test_conversion_rejects_bad_arguments_without_a_gpu(sblas):
    L = sblas.lib()
    f = L.sblas_hip_coo_to_csr_f64_i32
    need = L.sblas_hip_coo_to_csr_workspace(4, 300, 7)
    assert need > 0

    def call(rows=4, cols=300, nnz=7, r=one, c=one, v=one, dup=KEEP, rp=one, ci=one, out=one, pm=one, ru=one, ws=one, wsb=need):
        return f(-1, None, rows, cols, nnz, r, c, v, dup, rp, ci, out, pm, ru, ws, wsb)

    for kw in (dict(rows=-1), dict(cols=-1), dict(nnz=-1), dict(nnz=1 << 31), dict(cols=1 << 31), dict(rows=1 << 31)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(r=None), dict(c=None), dict(rp=None), dict(ci=None)):
        assert call(**kw) == INVALID, kw
    assert call(v=None) == INVALID and call(out=None) == INVALID          # coo_val and val: both or neither
    for dup in (-1, 2, 7):
        assert call(dup=dup) == INVALID, dup
    assert call(rows=0) == INVALID and call(cols=0) == INVALID            # no row / column to hold a triplet
    for dup in (KEEP, SUM):
        assert call(dup=dup, ws=None) == WORKSPACE
        assert call(dup=dup, wsb=0) == WORKSPACE
        assert call(dup=dup, wsb=need - 1) == WORKSPACE
        assert call(dup=dup, ws=C.c_void_p(24)) == INVALID                # 16-byte aligned workspace


def test_workspace_is_monotone(sblas):
    ws = sblas.lib().sblas_hip_coo_to_csr_workspace
    assert ws(-1, 5, 5) == 0 and ws(5, -1, 5) == 0 and ws(5, 5, -1) == 0
    assert ws(5, 5, 0) == 0 and ws(0, 0, 0) == 0                          # no triplets: nothing to sort
    assert sblas.coo_workspace_bytes(10, 1000, 5000) == ws(10, 1000, 5000)
    prev = 0
    for nnz in (1, 2, 100, 4095, 4096, 4097, 10 ** 5, 10 ** 7, 2 ** 31 - 1):
        cur = ws(10, 1000, nnz)
        assert cur >= prev and cur >= 16 * nnz, nnz
        prev = cur
    for fixed in (dict(rows=10), dict(cols=10)):
        prev = 0
        for dim in (1, 2, 255, 256, 257, 1 << 16, (1 << 24) + 1, 2 ** 31 - 1):
            cur = ws(fixed.get("rows", dim), fixed.get("cols", dim), 1000)
            assert cur >= prev and cur >= 16 * 1000, (fixed, dim)
            prev = cur


def test_plan_create_rejects_bad_arguments_without_a_gpu(sblas):
    f = sblas.lib().sblas_hip_coo_plan_create
    h = C.c_void_p()

    def call(rows=4, cols=6, nnz=3, r=one, c=one, dup=SUM, out=C.byref(h)):
        return f(-1, None, rows, cols, nnz, r, c, dup, out)

    for kw in (dict(rows=-1), dict(cols=-1), dict(nnz=-1), dict(rows=1 << 31), dict(cols=1 << 31), dict(nnz=1 << 31)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(r=None), dict(c=None), dict(out=None), dict(dup=2), dict(dup=-1)):
        assert call(**kw) == INVALID, kw
    assert call(rows=0) == INVALID and call(cols=0) == INVALID            # triplets without a row / column
    assert not h.value


def test_plan_calls_reject_bad_arguments_without_a_gpu(sblas):
    L = sblas.lib()
    assert L.sblas_hip_coo_plan_assemble(None, None, one, one) == INVALID
    out = (C.c_int64 * 8)()
    assert L.sblas_hip_coo_plan_info(None, out) == INVALID
    assert L.sblas_hip_coo_plan_csr(None, None, None, None, None) == INVALID
    assert L.sblas_hip_coo_plan_destroy(None) == 0


def test_python_wrappers_refuse_wrong_tensors(sblas):
    import torch
    r = torch.zeros(3, dtype=torch.int32)
    c = torch.zeros(3, dtype=torch.int32)
    v = torch.zeros(3, dtype=torch.float64)
    for make in (lambda *a, **k: sblas.coo_to_csr(4, 6, *a, **k), lambda r_, c_, v_=None, **k: sblas.CooPlan(4, 6, r_, c_, **k)):
        with pytest.raises(sblas.SblasError, match="GPU tensor"):
            make(r, c, v)                                                  # CPU tensors: no CPU path
        with pytest.raises(sblas.SblasError, match="int32"):
            make(r.long(), c, v)
        with pytest.raises(sblas.SblasError, match="int32"):
            make(r, c.long(), v)
        with pytest.raises(sblas.SblasError, match="contiguous"):
            make(r, torch.zeros(6, dtype=torch.int32)[::2], v)
        with pytest.raises(sblas.SblasError, match="entries"):
            make(r, c[:2], v)
        with pytest.raises(sblas.SblasError, match="dup"):
            make(r, c, v, dup="mean")
    with pytest.raises(sblas.SblasError, match="float64"):
        sblas.coo_to_csr(4, 6, r, c, v.float())
    with pytest.raises(sblas.SblasError, match="entries"):
        sblas.coo_to_csr(4, 6, r, c, v[:2])
    e = torch.zeros(0, dtype=torch.int32)
    with pytest.raises(sblas.SblasError, match="GPU tensor"):
        sblas.coo_to_csr(4, 6, e, e)                                       # nothing to convert, still no CPU path
    with pytest.raises(sblas.SblasError, match="GPU tensor"):
        sblas.CooPlan(4, 6, e, e)


def test_coo_from_torch_extracts_the_triplets_as_stored(sblas):
    import torch
    idx = torch.tensor([[2, 0, 2, 1, 2], [5, 1, 5, 0, 5]])
    val = torch.tensor([1.5, -0.0, 2.25, float("inf"), -4.0], dtype=torch.float64)
    t = torch.sparse_coo_tensor(idx, val, (3, 7))
    assert not t.is_coalesced()
    rows, cols, r, c, v = sblas.coo_from_torch(t)
    assert (rows, cols) == (3, 7)
    assert r.dtype == torch.int32 and c.dtype == torch.int32 and v.dtype == torch.float64
    assert r.is_contiguous() and c.is_contiguous() and v.is_contiguous() and r.device == t.device
    assert r.tolist() == [2, 0, 2, 1, 2] and c.tolist() == [5, 1, 5, 0, 5]
    assert np.array_equal(v.numpy().view(np.uint64), val.numpy().view(np.uint64))     # -0.0 and Inf as stored
    rows, cols, r, c, v = sblas.coo_from_torch(t.coalesce())
    assert r.tolist() == [0, 1, 2] and c.tolist() == [1, 0, 5] and v.tolist() == [-0.0, float("inf"), -0.25]
    rows, cols, r, c, v = sblas.coo_from_torch(torch.sparse_coo_tensor(torch.zeros((2, 0), dtype=torch.long),
                                                                       torch.zeros(0, dtype=torch.float64), (4, 0)))
    assert (rows, cols, r.numel(), c.numel(), v.numel()) == (4, 0, 0, 0, 0)


def test_coo_from_torch_refusals(sblas):
    import torch
    idx = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(sblas.SblasError, match="sparse_coo"):
        sblas.coo_from_torch(torch.zeros(3, 3, dtype=torch.float64))                   # a dense tensor
    with pytest.raises(sblas.SblasError, match="sparse_coo"):
        sblas.coo_from_torch(torch.sparse_coo_tensor(idx, torch.ones(2, dtype=torch.float64), (2, 2)).to_sparse_csr())
    with pytest.raises(sblas.SblasError, match="float64"):
        sblas.coo_from_torch(torch.sparse_coo_tensor(idx, torch.ones(2), (2, 2)))
    with pytest.raises(sblas.SblasError, match="2-D"):
        sblas.coo_from_torch(torch.sparse_coo_tensor(torch.zeros((3, 1), dtype=torch.long), torch.ones(1, dtype=torch.float64),
                                                     (2, 2, 2)))
    with pytest.raises(sblas.SblasError, match="2-D"):                                 # a dense trailing dimension
        sblas.coo_from_torch(torch.sparse_coo_tensor(torch.zeros((1, 1), dtype=torch.long),
                                                     torch.ones((1, 2), dtype=torch.float64), (2, 2)))
    e = torch.zeros((2, 0), dtype=torch.long)
    z = torch.zeros(0, dtype=torch.float64)
    for shape in ((1 << 31, 4), (4, 1 << 31)):
        with pytest.raises(sblas.SblasError, match="2\\^31"):
            sblas.coo_from_torch(torch.sparse_coo_tensor(e, z, shape))
    assert sblas.coo_from_torch(torch.sparse_coo_tensor(e, z, ((1 << 31) - 1, 4)))[0] == (1 << 31) - 1
