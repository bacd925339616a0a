"""Autograd of the sparse products (sblas_amd.autograd.CsrOperator): C = A(val) B and y = A(val) x, differentiable in val
(SDDMM on A's pattern) and in the dense operand (A^T through a TransposePlan)."""
import numpy as np
import pytest

import numerics as N
import sddmm_numerics as SN

pytestmark = pytest.mark.gpu


def small_pattern(seed=0):
    """12 x 9: unsorted columns, duplicates, empty rows"""
    rng = np.random.default_rng(seed)
    parts = []
    for r in range(12):
        if r in (3, 11):
            parts.append(np.zeros(0, np.int64))
            continue
        c = rng.integers(0, 9, int(rng.integers(1, 6)))
        parts.append(np.concatenate([c, c[:1]]) if r % 4 == 0 else c)      # a duplicate in every fourth row
    rp = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)
    return 12, 9, rp, np.concatenate(parts).astype(np.int32)


def operator(torch, dev, rows, cols, rp, ci, **kw):
    from sblas_amd.autograd import CsrOperator
    return CsrOperator(rows, cols, torch.from_numpy(rp).to(dev), torch.from_numpy(ci).to(dev), **kw)


def restate_matmul(torch, rows, rp, ci, val, B):
    """the same product without a sparse kernel: gather, scale, index_add_"""
    r = torch.from_numpy(N.row_of_entries(rp)).to(val.device)
    c = torch.from_numpy(ci.astype(np.int64)).to(val.device)
    return torch.zeros(rows, B.shape[1], dtype=torch.float64, device=val.device).index_add_(0, r, val[:, None] * B[c])


@pytest.mark.parametrize("n", [1, 5, 64])
def test_gradcheck_matmul(sblas, cuda, n):
    import torch
    rows, cols, rp, ci = small_pattern()
    op = operator(torch, cuda, rows, cols, rp, ci, n=n if n == 64 else 0)
    g = torch.Generator(device="cpu").manual_seed(n)
    val = (torch.rand(len(ci), dtype=torch.float64, generator=g) * 2 - 1).to(cuda).requires_grad_()
    B = (torch.rand(cols, n, dtype=torch.float64, generator=g) * 2 - 1).to(cuda).requires_grad_()
    assert torch.autograd.gradcheck(op.matmul, (val, B), nondet_tol=0)
    Bt = (torch.rand(n, cols, dtype=torch.float64, generator=g) * 2 - 1).to(cuda).requires_grad_()
    assert torch.autograd.gradcheck(lambda v, b: op.matmul(v, b.t()), (val, Bt), nondet_tol=0)   # a column-major B


def test_gradcheck_matvec(sblas, cuda):
    import torch
    rows, cols, rp, ci = small_pattern(1)
    op = operator(torch, cuda, rows, cols, rp, ci)
    g = torch.Generator(device="cpu").manual_seed(3)
    val = (torch.rand(len(ci), dtype=torch.float64, generator=g) * 2 - 1).to(cuda).requires_grad_()
    x = (torch.rand(cols, dtype=torch.float64, generator=g) * 2 - 1).to(cuda).requires_grad_()
    assert torch.autograd.gradcheck(op.matvec, (val, x), nondet_tol=0)


def big_case(torch, dev, n, seed=0):
    from sblas_amd import synth
    rows = cols = 20000
    rp, ci, v = synth.random_csr(rows, cols, 8, seed=5, empty_every=11, long_row=(17, 3000))
    rng = np.random.default_rng(seed)
    val = SN.log_uniform(rng, len(ci), 10)
    B = SN.log_uniform(rng, (cols, n), 10)
    W = SN.log_uniform(rng, (rows, n), 10)
    return rows, cols, rp, ci, val, B, W


@pytest.mark.parametrize("n", [1, 8, 64])
def test_gradients_of_a_20000_row_case(sblas, cuda, n):
    """dval against the double-double reference within the SDDMM bound, dB within numerics.check_general's; and both
    against the gradients torch derives for the index_add_ restatement: each side is within its bound of the exact
    value, so the two differ by at most twice the bound."""
    import torch
    rows, cols, rp, ci, val, B, W = big_case(torch, cuda, n)
    op = operator(torch, cuda, rows, cols, rp, ci, n=n)
    d = lambda a: torch.from_numpy(a).to(cuda)
    vd, Bd, Wd = d(val).requires_grad_(), d(B).requires_grad_(), d(W)
    (op.matmul(vd, Bd) * Wd).sum().backward()
    dval, dB = vd.grad.cpu().numpy(), Bd.grad.cpu().numpy()
    ok, worst, where, over = SN.check_general(dval, rp, ci, W, B, None, 1.0, 0.0)
    print("n=%d dval: worst err/bound = %.3g" % (n, worst))
    assert ok, (worst, where, over)
    colptr, rowidx, perm = N.csc_of(rows, cols, rp, ci)
    res = N.check_general(dB, colptr, rowidx, val[perm], W, None, 1.0, 0.0, np.float64)
    print("n=%d dB: %r" % (n, res))
    assert res, repr(res)
    v2, B2 = d(val).requires_grad_(), d(B).requires_grad_()
    (restate_matmul(torch, rows, rp, ci, v2, B2) * Wd).sum().backward()
    bv = SN.bound(rp, ci, W, B, None, 1.0, 0.0)
    assert (np.abs(dval - v2.grad.cpu().numpy()) <= 2 * bv).all()
    bB = N.bound(colptr, rowidx, val[perm], W, None, 1.0, 0.0, np.float64)
    assert (np.abs(dB - B2.grad.cpu().numpy()) <= 2 * bB).all()
    if n == 1:   # the same through matvec
        v3, x3 = d(val).requires_grad_(), d(B[:, 0].copy()).requires_grad_()
        (op.matvec(v3, x3) * Wd[:, 0]).sum().backward()
        ok, worst, where, over = SN.check_general(v3.grad.cpu().numpy(), rp, ci, W, B, None, 1.0, 0.0)
        assert ok, (worst, where, over)
        res = N.check_general(x3.grad.cpu().numpy()[:, None], colptr, rowidx, val[perm], W, None, 1.0, 0.0, np.float64)
        assert res, repr(res)


def test_sum_backward_delivers_an_expanded_gradient(sblas, cuda):
    import torch
    rows, cols, rp, ci = small_pattern(2)
    op = operator(torch, cuda, rows, cols, rp, ci)
    g = torch.Generator(device="cpu").manual_seed(9)
    val = torch.rand(len(ci), dtype=torch.float64, generator=g).to(cuda).requires_grad_()
    B = torch.rand(cols, 6, dtype=torch.float64, generator=g).to(cuda).requires_grad_()
    op.matmul(val, B).sum().backward()
    v2, B2 = val.detach().clone().requires_grad_(), B.detach().clone().requires_grad_()
    restate_matmul(torch, rows, rp, ci, v2, B2).sum().backward()
    assert torch.allclose(val.grad, v2.grad, rtol=1e-13, atol=1e-13) and torch.allclose(B.grad, B2.grad, rtol=1e-13, atol=1e-13)
    x = torch.rand(cols, dtype=torch.float64, generator=g).to(cuda).requires_grad_()
    v3 = val.detach().clone().requires_grad_()
    op.matvec(v3, x).sum().backward()
    assert torch.allclose(v3.grad, x.detach()[torch.from_numpy(ci.astype(np.int64)).to(cuda)], rtol=0, atol=0)
    assert torch.allclose(x.grad, B2.grad.new_zeros(cols).index_add_(0, torch.from_numpy(ci.astype(np.int64)).to(cuda), v3.detach()),
                          rtol=1e-13, atol=1e-13)


def test_only_the_half_that_is_asked_for_is_computed(sblas, cuda):
    import torch
    rows, cols, rp, ci = small_pattern(3)
    g = torch.Generator(device="cpu").manual_seed(4)
    val = torch.rand(len(ci), dtype=torch.float64, generator=g).to(cuda)
    B = torch.rand(cols, 4, dtype=torch.float64, generator=g).to(cuda)
    calls = {"val": 0, "dense": 0}

    def counted(op):
        gv, gd = op._grad_val, op._grad_dense_mm
        op._grad_val = lambda *a: (calls.__setitem__("val", calls["val"] + 1), gv(*a))[1]
        op._grad_dense_mm = lambda *a: (calls.__setitem__("dense", calls["dense"] + 1), gd(*a))[1]
        return op

    op = counted(operator(torch, cuda, rows, cols, rp, ci))
    v = val.clone().requires_grad_()
    op.matmul(v, B).sum().backward()                       # only val
    assert v.grad is not None and calls == {"val": 1, "dense": 0} and op.transpose_plan is None
    op = counted(operator(torch, cuda, rows, cols, rp, ci))
    calls.update(val=0, dense=0)
    b = B.clone().requires_grad_()
    op.matmul(val, b).sum().backward()                     # only B
    assert b.grad is not None and calls == {"val": 0, "dense": 1} and op.transpose_plan is not None
    assert not op.matmul(val, B).requires_grad             # neither: no graph at all


def test_the_second_step_sees_the_new_values(sblas, cuda):
    """The TransposePlan keeps its own copy of the values; dB of step two must be that of step two's values."""
    import torch
    rows, cols, rp, ci = small_pattern(4)
    op = operator(torch, cuda, rows, cols, rp, ci, n=6)
    g = torch.Generator(device="cpu").manual_seed(5)
    val = torch.rand(len(ci), dtype=torch.float64, generator=g).to(cuda).requires_grad_()
    B = torch.rand(cols, 6, dtype=torch.float64, generator=g).to(cuda).requires_grad_()
    W = torch.rand(rows, 6, dtype=torch.float64, generator=g).to(cuda)
    grads = []
    for step in range(2):
        val.grad = B.grad = None
        (op.matmul(val, B) * W).sum().backward()
        v2, B2 = val.detach().clone().requires_grad_(), B.detach().clone().requires_grad_()
        (restate_matmul(torch, rows, rp, ci, v2, B2) * W).sum().backward()
        assert torch.allclose(B.grad, B2.grad, rtol=1e-13, atol=1e-13), step
        assert torch.allclose(val.grad, v2.grad, rtol=1e-13, atol=1e-13), step
        grads.append(B.grad.clone())
        with torch.no_grad():                              # an optimisation step on the values
            val -= 0.5 * val.grad + 0.25
    assert not torch.allclose(grads[0], grads[1])


def test_split_transpose_plan_on_a_long_column(sblas, cuda):
    """A = the transpose of a power-law pattern: one column of 30 000 entries, a row of A^T the split plan cuts up."""
    import torch
    from sblas_amd import synth
    prp, pci, _ = synth.powerlaw(40000, max_len=30000)
    colptr, rowidx, _ = N.csc_of(40000, 40000, prp, pci)
    rows = cols = 40000
    rp, ci = colptr.astype(np.int32), rowidx.astype(np.int32)
    n = 64
    op = operator(torch, cuda, rows, cols, rp, ci, n=n, split=True)
    rng = np.random.default_rng(1)
    val, B, W = SN.log_uniform(rng, len(ci), 8), SN.log_uniform(rng, (cols, n), 8), SN.log_uniform(rng, (rows, n), 8)
    d = lambda a: torch.from_numpy(a).to(cuda)
    vd, Bd = d(val).requires_grad_(), d(B).requires_grad_()
    (op.matmul(vd, Bd) * d(W)).sum().backward()
    print("transpose plan:", op.transpose_plan.info())
    tcolptr, trowidx, perm = N.csc_of(rows, cols, rp, ci)
    assert int(np.diff(tcolptr).max()) == 30000
    res = N.check_general(Bd.grad.cpu().numpy(), tcolptr, trowidx, val[perm], W, None, 1.0, 0.0, np.float64)
    print("dB:", res)
    assert res, repr(res)
    ok, worst, where, over = SN.check_general(vd.grad.cpu().numpy(), rp, ci, W, B, None, 1.0, 0.0)
    assert ok, (worst, where, over)
