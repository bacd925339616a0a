"""The differentiable solves on the GPU (sblas_amd.autograd.TriangularOperator / SolveOperator): torch's gradcheck at its
defaults, the forward against the plans it promises the bits of, both gradients against the composition of public calls
(TransposePlan -> the same plans on csc() -> the solve of xbar, then sddmm_tensor) with ==, and against the gradient
torch derives through a dense float64 solve on the CPU."""
import numpy as np
import pytest

import krylov_numerics as KN
import solver_compose as SC

pytestmark = pytest.mark.gpu


def up(torch, dev, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint64)


def dense_of(n, rp, ci, val):
    A = np.zeros((n, n))
    np.add.at(A, (np.repeat(np.arange(n), np.diff(rp)), ci), val)
    return A


def triangular_matrix(n, per_row, seed):
    """unsorted rows, a duplicated off-diagonal entry, stored entries in both triangles, a diagonal in [4, 5] and
    off-diagonal absolute row sums of at most 2"""
    rng = np.random.default_rng(seed)
    rows, vals = [], []
    for i in range(n):
        others = [j for j in range(max(0, i - 40), min(n, i + 41)) if j != i]
        off = rng.choice(others, size=min(per_row, len(others)), replace=False).tolist()
        cols = off[:2] + [i] + off[2:] + off[:1]                           # the diagonal in the middle, off[0] twice
        v = rng.uniform(-1.0, 1.0, len(cols))
        v *= 2.0 / np.abs(v).sum()
        v[2 if len(off) >= 2 else len(off)] = rng.uniform(4.0, 5.0)
        rows.append(cols), vals.append(v)
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return n, rp, np.concatenate(rows).astype(np.int32), np.concatenate(vals)


def part_mask(rp, ci, lower, unit):
    r = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    return (ci < r if unit else ci <= r) if lower else (ci > r if unit else ci >= r)


# ---- triangular --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [0, 3])
@pytest.mark.parametrize("lower,unit", [(True, False), (False, False), (True, True), (False, True)])
def test_triangular_gradcheck(sblas, cuda, lower, unit, s):
    import torch
    from sblas_amd import autograd as AG
    n, rp, ci, val = triangular_matrix(30, 4, 1)
    drp, dci, dval = up(torch, cuda, rp, ci, val)
    op = AG.TriangularOperator(n, drp, dci, lower=lower, unit_diag=unit)
    rng = np.random.default_rng(2)
    b, = up(torch, cuda, rng.standard_normal((n, s) if s else n))
    v = dval.clone().requires_grad_()
    b.requires_grad_()
    assert torch.autograd.gradcheck(lambda v_, b_: op.solve(v_, b_, alpha=0.5), (v, b), nondet_tol=0.0)
    assert torch.autograd.gradcheck(lambda v_, b_: AG.triangular_solve(op, v_, b_), (v, b), nondet_tol=0.0)
    op.destroy()


@pytest.mark.parametrize("s", ["1d", 1, 8, 9])
@pytest.mark.parametrize("lower,unit", [(True, False), (False, True)])
def test_triangular_equals_the_composition(sblas, cuda, lower, unit, s):
    import torch
    from sblas_amd import autograd as AG
    n, rp, ci, val = triangular_matrix(2000, 5, 3)
    drp, dci, dval = up(torch, cuda, rp, ci, val)
    rng = np.random.default_rng(4)
    shape = (n,) if s == "1d" else (n, s)
    b, w = up(torch, cuda, rng.standard_normal(shape), rng.standard_normal(shape))
    op = AG.TriangularOperator(n, drp, dci, lower=lower, unit_diag=unit)
    v, bb = dval.clone().requires_grad_(), b.clone().requires_grad_()
    x = op.solve(v, bb)
    (x * w).sum().backward()
    # the composition from public calls
    plan = sblas.SptrsvPlan(n, drp, dci, lower=lower, unit_diag=unit)
    want_x = plan.solve(dval, b) if s == "1d" else plan.solve_multi(dval, b)
    assert (bits(x) == bits(want_x)).all()
    tp = sblas.TransposePlan(n, n, drp, dci, dval)
    colptr, rowidx, val_t = tp.csc()
    adj = sblas.SptrsvPlan(n, colptr, rowidx, lower=not lower, unit_diag=unit)
    g = adj.solve(val_t, w) if s == "1d" else adj.solve_multi(val_t, w)
    assert (bits(bb.grad) == bits(g)).all()
    out = torch.empty(len(ci), dtype=torch.float64, device=cuda)
    sblas.sddmm_tensor((n, n, drp, dci), g.view(n, -1), want_x.view(n, -1), out, -1.0, 0.0)
    mask = part_mask(rp, ci, lower, unit)
    want = np.where(mask, out.cpu().numpy(), 0.0)
    assert (~mask).any() and (bits(v.grad) == want.view(np.uint64)).all()
    assert (bits(v.grad)[~mask] == 0).all()                                # ignored entries: exactly +0.0
    for p in (plan, adj, tp):
        p.destroy()
    op.destroy()


def test_triangular_only_the_half_that_is_asked_for(sblas, cuda, monkeypatch):
    import torch
    from sblas_amd import autograd as AG
    n, rp, ci, val = triangular_matrix(30, 4, 5)
    drp, dci, dval = up(torch, cuda, rp, ci, val)
    b, = up(torch, cuda, np.random.default_rng(6).standard_normal(n))
    calls = []
    inner = AG._values_gradient
    monkeypatch.setattr(AG, "_values_gradient", lambda *a: (calls.append(1), inner(*a))[1])
    op = AG.TriangularOperator(n, drp, dci)
    v = dval.clone().requires_grad_()
    op.solve(v, b).sum().backward()                                         # only val
    assert v.grad is not None and len(calls) == 1
    bb = b.clone().requires_grad_()
    op.solve(dval, bb).sum().backward()                                     # only b
    assert bb.grad is not None and len(calls) == 1
    assert not op.solve(dval, b).requires_grad                              # neither: no graph at all
    op.destroy()


def test_triangular_second_step_sees_the_new_values(sblas, cuda):
    """The TransposePlan keeps its own copy of the values; the gradients of step two must be those of step two's values."""
    import torch
    from sblas_amd import autograd as AG
    n, rp, ci, val = triangular_matrix(30, 4, 7)
    drp, dci, dval = up(torch, cuda, rp, ci, val)
    rng = np.random.default_rng(8)
    b, w = up(torch, cuda, rng.standard_normal((n, 2)), rng.standard_normal((n, 2)))
    op = AG.TriangularOperator(n, drp, dci, lower=False)
    v, bb = dval.clone().requires_grad_(), b.clone().requires_grad_()
    r, c, keep = torch.from_numpy(np.repeat(np.arange(n), np.diff(rp))), torch.from_numpy(ci.astype(np.int64)), torch.from_numpy(part_mask(rp, ci, False, False))
    grads = []
    for step in range(2):
        v.grad = bb.grad = None
        (op.solve(v, bb) * w).sum().backward()
        v2, b2 = v.detach().cpu().requires_grad_(), bb.detach().cpu().requires_grad_()
        T = torch.zeros(n, n, dtype=torch.float64).index_put((r[keep], c[keep]), v2[keep], accumulate=True)
        (torch.linalg.solve(T, b2) * w.cpu()).sum().backward()
        assert torch.allclose(bb.grad.cpu(), b2.grad, rtol=1e-12, atol=1e-13), step
        assert torch.allclose(v.grad.cpu(), v2.grad, rtol=1e-12, atol=1e-13), step
        grads.append(v.grad.clone())
        with torch.no_grad():                                               # an optimisation step on the values
            v -= 0.05 * v.grad
    assert not torch.allclose(grads[0], grads[1])
    op.destroy()


# ---- Krylov ------------------------------------------------------------------------------------------------------------
def small_system(symmetric, n=24, seed=9):
    """ascending rows that store their diagonal (what ILU(0) and the diagonal need); diagonal in [4, 5], off-diagonal
    absolute row sums of at most 2: kappa_2 <= 3.5"""
    rng = np.random.default_rng(seed)
    M = rng.random((n, n)) < 0.12
    M = M | M.T
    np.fill_diagonal(M, True)
    off = rng.uniform(-1.0, 1.0, (n, n))
    if symmetric:
        off = (off + off.T) / 2
    A = off * M
    np.fill_diagonal(A, 0.0)
    A *= 2.0 / max(np.abs(A).sum(1).max(), np.abs(A).sum(0).max())
    A += np.diag(rng.uniform(4.0, 5.0, n))
    r, c = np.nonzero(M)
    rp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int32)
    return n, rp, c.astype(np.int32), A[r, c], A


@pytest.mark.parametrize("s", [0, 2])
@pytest.mark.parametrize("precond", [None, "jacobi", "ilu0"])
@pytest.mark.parametrize("method", ["pcg", "bicgstab", "gmres"])
def test_krylov_gradcheck(sblas, cuda, method, precond, s):
    """The conditions under which the adjoint formulas passed gradcheck on the CPU: rtol = 1e-13 in both solves, kappa_2 <= 4,
    so that the solve noise reaches the finite differences as kappa * 1e-13 / 1e-6 against gradcheck's atol of 1e-5.
    The operator is strict, so a solve that ends other than "converged" fails the test, in every combination but one:
    gradcheck sends unit vectors as xbar, and BiCGStab, whose shadow residual is the right-hand side, then reads one
    component of the residual as rho; behind ILU(0), which is almost the exact factor on this pattern, that component is
    exactly zero after the first iteration -- a true breakdown at |r| = 3.7e-12, short of 1e-13 (seen with b 1-D).  For
    "bicgstab" + "ilu0" alone the operator returns that iterate (strict=False) and gradcheck is the judge of it."""
    import torch
    from sblas_amd import autograd as AG
    n, rp, ci, val, A = small_system(symmetric=method == "pcg")
    kappa = np.linalg.cond(A)
    print("kappa_2 = %.3f, n = %d, nnz = %d" % (kappa, n, len(ci)))
    assert kappa <= 4.0 and 24 <= n <= 40
    drp, dci, dval = up(torch, cuda, rp, ci, val)
    op = AG.SolveOperator(n, drp, dci, method=method, precond=precond, restart=n, rtol=1e-13, max_iter=400,
                          strict=(method, precond) != ("bicgstab", "ilu0"))
    b, = up(torch, cuda, np.random.default_rng(10).standard_normal((n, s) if s else n))
    v = dval.clone().requires_grad_()
    b.requires_grad_()
    assert torch.autograd.gradcheck(op.solve, (v, b), nondet_tol=0.0)
    op.destroy()


BIG = {"gmres-ilu0": ("gmres", "ilu0", "convection"), "bicgstab-amg": ("bicgstab", "amg", "convection"),
       "pcg-amg_smoothed": ("pcg", "amg_smoothed", "laplacian")}
BIG_RTOL = 1e-10
# error / (kappa_2 * rtol) of the host loop on each case's own right-hand sides, the larger of the forward and the adjoint
# system, by the number of columns (0: b 1-D): measured once on a CPU and pinned, so that the bound below is a number one
# can read; the test measures it again and holds the measurement to the pinned figure
BIG_MARGIN = {"gmres-ilu0": {0: 0.0609, 2: 0.0369, 4: 0.0560}, "bicgstab-amg": {0: 0.0374, 2: 0.0143, 4: 0.0380},
              "pcg-amg_smoothed": {0: 0.00247, 2: 0.00271, 4: 0.00284}}


def host_margin(method, A, rhs):
    """error / (kappa_2 * rtol) of the host float64 loop of solver_compose.py (no preconditioner, the same stopping test on
    the recurrence residual) on A y = rhs: the largest over the columns of rhs"""
    n = len(A)
    kappa = np.linalg.cond(A)
    worst = 0.0
    for j in range(rhs.shape[1]):
        mv, ident, z = (lambda v: A @ v), (lambda v: v.copy()), np.zeros(n)
        if method == "pcg":
            y = SC.composed_pcg(mv, ident, KN.dot_np, rhs[:, j], z, BIG_RTOL, 1000).x
        elif method == "bicgstab":
            y = SC.composed_bicgstab(mv, ident, KN.dot_np, rhs[:, j], z, BIG_RTOL, 1000).x
        else:
            y = SC.composed_gmres(mv, ident, KN.dot_np, lambda V, w: [KN.dot_np(u, w) for u in V], rhs[:, j], z, 30, BIG_RTOL, 1000)["x"]
        exact = np.linalg.solve(A, rhs[:, j])
        worst = max(worst, np.linalg.norm(y - exact) / np.linalg.norm(exact) / (kappa * BIG_RTOL))
    return worst, kappa


@pytest.mark.parametrize("s", [0, 2, 4])
@pytest.mark.parametrize("case", sorted(BIG))
def test_krylov_equals_the_composition_and_the_dense_gradient(sblas, cuda, case, s):
    """Both gradients equal the composition of public calls with ==, and agree with the gradient torch derives through a
    dense solve within allow * kappa_2 * rtol, relative, in the 2-norm.  allow = min(100, 4 * margin), margin the host
    loop's error / (kappa_2 * rtol) on the forward and the adjoint system with this test's right-hand sides, pinned in
    BIG_MARGIN, measured again in the test and printed.  Measured at rtol = 1e-10 with these right-hand sides: GMRES(30) 0.037 - 0.061 and BiCGStab
    0.014 - 0.038 on the 24 x 24 upwind convection-diffusion matrix (kappa_2 = 95.6), CG 0.0025 - 0.0028 on the 24 x 24
    Laplacian (kappa_2 = 253), so allow is 0.15 - 0.24, 0.057 - 0.15 and 0.0099 - 0.011.  The gradients on one MI355X, as
    error / (kappa_2 * rtol): bbar 0.0072 - 0.028 and valbar 0.017 - 0.035 for "gmres" + "ilu0", 0.0018 - 0.012 and
    0.0051 - 0.014 for "bicgstab" + "amg", 0.00044 - 0.00060 and 0.00050 - 0.00086 for "pcg" + "amg_smoothed"."""
    import torch
    from sblas_amd import autograd as AG
    method, precond, which = BIG[case]
    n, rp, ci, val = KN.convection_diffusion(24) if which == "convection" else KN.laplacian(24)
    val = np.asarray(val, np.float64)
    drp, dci, dval = up(torch, cuda, rp, ci, val)
    rng = np.random.default_rng(12)
    shape = (n, s) if s else (n,)
    bh, wh = rng.standard_normal(shape), rng.standard_normal(shape)
    b, w = up(torch, cuda, bh, wh)
    op = AG.SolveOperator(n, drp, dci, method=method, precond=precond, rtol=BIG_RTOL)
    v, bb = dval.clone().requires_grad_(), b.clone().requires_grad_()
    x = op.solve(v, bb)
    (x * w).sum().backward()
    assert op.last["forward"] is not None and op.last["backward"] is not None
    for phase in ("forward", "backward"):
        st = op.last[phase]["status"]
        assert (st if isinstance(st, list) else [st]) == ["converged"] * max(s, 1), (phase, st)

    # ---- the composition from public calls: the same plans on A, then on TransposePlan.csc() ----
    def solve_on(rowptr, colidx, values, rhs):
        if precond == "ilu0":
            pre = sblas.Ilu0Plan(n, rowptr, colidx)
            kw, seat = dict(lu=pre.factor(values)), (pre if s == 0 else pre.solvers())
        else:
            pre = sblas.AmgPlan(n, rowptr, colidx, prolongator="smoothed" if precond == "amg_smoothed" else "plain")
            pre.setup(values)
            kw, seat = {}, pre
        if method == "gmres":
            plan = sblas.GmresMultiPlan(n, rowptr, colidx, s, precond=seat) if s else sblas.GmresPlan(n, rowptr, colidx, precond=seat)
        else:
            plan = (sblas.KrylovMultiPlan(n, rowptr, colidx, s, method=method, precond=seat) if s else
                    sblas.KrylovPlan(n, rowptr, colidx, method=method, precond=seat))
        y, st = plan.solve(values, rhs, None, rtol=BIG_RTOL, **kw)
        plan.destroy()
        return y, pre
    want_x, pre1 = solve_on(drp, dci, dval, b)
    assert (bits(x) == bits(want_x)).all()
    tp = sblas.TransposePlan(n, n, drp, dci, dval)
    colptr, rowidx, val_t = tp.csc()
    g, pre2 = solve_on(drp, dci, dval, w) if method == "pcg" else solve_on(colptr, rowidx, val_t, w)
    want_val = torch.empty(len(ci), dtype=torch.float64, device=cuda)
    sblas.sddmm_tensor((n, n, drp, dci), g.view(n, -1), want_x.view(n, -1), want_val, -1.0, 0.0)
    assert (bits(bb.grad) == bits(g)).all() and (bits(v.grad) == bits(want_val)).all()

    # ---- the dense gradient on the CPU ----
    A = dense_of(n, rp, ci, val)
    r, c = torch.from_numpy(np.repeat(np.arange(n), np.diff(rp))), torch.from_numpy(ci.astype(np.int64))
    v2, b2 = torch.from_numpy(val).requires_grad_(), torch.from_numpy(bh).requires_grad_()
    Ad = torch.zeros(n, n, dtype=torch.float64).index_put((r, c), v2, accumulate=True)
    (torch.linalg.solve(Ad, b2) * torch.from_numpy(wh)).sum().backward()
    m_fwd, kappa = host_margin(method, A, bh.reshape(n, -1))
    m_adj, _ = host_margin(method, A.T, wh.reshape(n, -1))
    margin = BIG_MARGIN[case][s]
    assert abs(max(m_fwd, m_adj) - margin) <= 0.05 * margin, (m_fwd, m_adj, margin)      # the pinned figure is this loop's
    allow = min(100.0, 4.0 * margin)
    rel = lambda got, ref: float(np.linalg.norm(got.cpu().numpy() - ref.numpy()) / np.linalg.norm(ref.numpy()))
    e_b, e_v = rel(bb.grad, b2.grad), rel(v.grad, v2.grad)
    print("%s s=%d: kappa_2 %.4g, host margin %.4g (forward %.4g, adjoint %.4g), allow %.4g; db err / (kappa rtol) = %.4g, dval err / (kappa rtol) = %.4g"
          % (case, s, kappa, margin, m_fwd, m_adj, allow, e_b / (kappa * BIG_RTOL), e_v / (kappa * BIG_RTOL)))
    assert e_b <= allow * kappa * BIG_RTOL and e_v <= allow * kappa * BIG_RTOL
    for p in (pre1, pre2, tp):
        p.destroy()
    op.destroy()


def test_strict_names_the_phase(sblas, cuda):
    import torch
    from sblas_amd import autograd as AG
    n, rp, ci, val = KN.convection_diffusion(24)
    drp, dci, dval = up(torch, cuda, rp, ci, np.asarray(val, np.float64))
    b, = up(torch, cuda, np.random.default_rng(13).standard_normal(n))
    op = AG.SolveOperator(n, drp, dci, method="bicgstab", max_iter=2)
    with pytest.raises(sblas.SblasError, match="forward.*limit"):
        op.solve(dval, b)
    assert op.last["forward"]["status"] == "limit"
    op.destroy()
    op = AG.SolveOperator(n, drp, dci, method="bicgstab")
    op.backward_max_iter = 2                                                # only the backward's limit is short
    v = dval.clone().requires_grad_()
    x = op.solve(v, b)
    with pytest.raises(sblas.SblasError, match="backward.*limit"):
        x.sum().backward()
    op.destroy()
    op = AG.SolveOperator(n, drp, dci, method="bicgstab", max_iter=2, strict=False)
    v = dval.clone().requires_grad_()
    op.solve(v, b).sum().backward()                                         # returns what the solves left
    assert op.last["forward"]["status"] == "limit" and op.last["backward"]["status"] == "limit" and torch.isfinite(v.grad).all()
    op.destroy()


@pytest.mark.parametrize("method", ["pcg", "gmres"])
def test_a_zero_gradient_gives_zeros(sblas, cuda, method):
    import torch
    from sblas_amd import autograd as AG
    n, rp, ci, val, _ = small_system(symmetric=method == "pcg")
    drp, dci, dval = up(torch, cuda, rp, ci, val)
    op = AG.SolveOperator(n, drp, dci, method=method, precond="jacobi")
    b, w = up(torch, cuda, np.random.default_rng(14).standard_normal((n, 2)), np.array([[0.0, 1.0]] * n))
    v, bb = dval.clone().requires_grad_(), b.clone().requires_grad_()
    (op.solve(v, bb) * w).sum().backward()                                  # a zero column of xbar
    assert (bb.grad[:, 0] == 0).all() and (bb.grad[:, 1] != 0).any() and torch.isfinite(v.grad).all()
    v.grad = bb.grad = None
    (op.solve(v, bb[:, 0].contiguous()) * 0.0).sum().backward()             # a zero xbar
    assert (v.grad == 0).all() and (bb.grad == 0).all()
    op.destroy()


def test_refusals_come_before_any_launch(sblas, cuda):
    import torch
    from sblas_amd import autograd as AG
    n, rp, ci, val, _ = small_system(True)
    drp, dci, dval = up(torch, cuda, rp, ci, val)
    with pytest.raises(sblas.SblasError, match="chebyshev"):
        AG.SolveOperator(n, drp, dci, precond="chebyshev")
    with pytest.raises(sblas.SblasError):
        AG.SolveOperator(n, drp, dci, method="cg")
    op = AG.SolveOperator(n, drp, dci)
    b = torch.ones(n, dtype=torch.float64, device=cuda)
    for bad_val, bad_b in ((dval, b.cpu()), (dval.cpu(), b), (dval, b.float()), (dval.float(), b), (dval[:-1], b),
                           (dval, torch.ones(n, 65, dtype=torch.float64, device=cuda)), (dval, torch.ones(n + 1, dtype=torch.float64, device=cuda))):
        with pytest.raises(sblas.SblasError):
            op.solve(bad_val, bad_b)
    assert op.last == dict(forward=None, backward=None) and not op.forward_side.plans      # nothing ran, no plan was made
    tri = AG.TriangularOperator(n, drp, dci)
    for bad_val, bad_b in ((dval, b.cpu()), (dval, b.float()), (dval[:-1], b)):
        with pytest.raises(sblas.SblasError):
            tri.solve(bad_val, bad_b)
    op.destroy()
    tri.destroy()
