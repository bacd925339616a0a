"""The eigenvalue plan on the GPU (EigshPlan, eigsh, eigsh_rotate, eigsh_ritz) against tests/eigsh_numerics.py.

Every bit is pinned, so the checks of the kernels are ==: the rotation against gmres_combine column by column and against
its host reference, the Ritz kernel against the host Ritz step on every output array, and a whole solve against the loop
composed from SpMV, gmres_dots, gmres_project, krylov_dot, gmres_combine and the host Ritz step.  Only "it finds the
eigenpairs" holds a tolerance, and tests/test_eigsh_host.py says where that one comes from."""
import numpy as np
import pytest

import eigsh_numerics as EN
import krylov_numerics as KN

pytestmark = pytest.mark.gpu

RTOL = 1e-10


@pytest.fixture(scope="module")
def env(sblas, cuda):
    import torch
    return sblas, torch, cuda


def up(torch, cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def same(a, b):
    return KN.same_bits(a, b)


def device_csr(torch, cuda, A):
    n, rp, ci, val = EN.csr_of(A)
    return (n,) + tuple(up(torch, cuda, rp, ci, val))


# ---------------------------------------------------------------------------------------------------------------------
# the rotation kernel
# ---------------------------------------------------------------------------------------------------------------------
def strided(torch, cuda, V, ldv, offset):
    """V's columns in a buffer with column stride ldv >= n, starting at element `offset`: the (k, n) view and the buffer"""
    k, n = V.shape
    buf = torch.full((offset + k * ldv + 2,), -7.0, dtype=torch.float64, device=cuda)
    view = buf[offset:offset + k * ldv].view(k, ldv)[:, :n]
    view.copy_(torch.from_numpy(V).to(cuda))
    return view, buf


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2048, 2049, 4100])
def test_rotate_is_combine_column_by_column(env, n):
    """n at both sides of a rotation workgroup (256 rows) and of a cell of gmres_combine (2048); mm at both sides of every
    tier (8, 16, 32, 64); keep at both ends and the plan's default"""
    S, torch, cuda = env
    rng = np.random.default_rng(n)
    for mm in (1, 2, 7, 8, 9, 16, 17, 20, 32, 33, 63, 64):
        V = rng.standard_normal((mm + 1, n)) * 10.0 ** rng.integers(-3, 4, (mm + 1, n))
        for keep in sorted({1, max(mm - 1, 1), EN.default_keep(max(mm // 5, 1), mm) if mm > 1 else 1, mm}):
            Q = rng.standard_normal((mm, keep))
            dQ, = up(torch, cuda, Q)
            dV, = up(torch, cuda, V)
            want = [S.gmres_combine(dV[:mm], dQ[:, i].contiguous()).cpu().numpy() for i in range(keep)]
            ref = S.eigsh_rotate_ref(V, Q)
            for ldv, off in ((n, 0), (n + 3, 1)):                        # packed; a stride above n from an odd element
                view, buf = strided(torch, cuda, V, ldv, off)
                assert S.eigsh_rotate(view, dQ) is view
                got = view.cpu().numpy()
                for i in range(keep):
                    assert same(got[i], want[i]), (n, mm, keep, ldv, i)
                assert same(got[keep], V[mm]), (n, mm, keep, "moved")
                assert same(got[keep + 1:], V[keep + 1:]), (n, mm, keep, "untouched")
                assert same(got, ref), (n, mm, keep, "host reference")
                flat = buf.cpu().numpy()
                assert (flat[:off] == -7.0).all() and (flat[off + (mm + 1) * ldv:] == -7.0).all()
                if ldv > n:
                    assert (flat[off:off + (mm + 1) * ldv].reshape(mm + 1, ldv)[:, n:] == -7.0).all()   # between the columns


def test_rotate_keeps_a_nan_and_an_inf_in_their_row(env):
    S, torch, cuda = env
    n, mm, keep = 700, 20, 12
    rng = np.random.default_rng(5)
    V, Q = rng.standard_normal((mm + 1, n)), rng.standard_normal((mm, keep))
    V[3, 300], V[7, 555] = np.nan, np.inf
    dV, dQ = up(torch, cuda, V, Q)
    want = S.eigsh_rotate_ref(V, Q)
    got = S.eigsh_rotate(dV, dQ).cpu().numpy()
    assert same(got, want)
    bad = ~np.isfinite(got[:keep])
    assert bad[:, 300].all() and bad[:, 555].all() and bad.sum() == 2 * keep


def test_rotate_refusals(env):
    S, torch, cuda = env
    V = torch.ones((9, 100), dtype=torch.float64, device=cuda)
    Q = torch.ones((8, 4), dtype=torch.float64, device=cuda)
    for call in (lambda: S.eigsh_rotate(V[:8], Q), lambda: S.eigsh_rotate(V, Q.float()), lambda: S.eigsh_rotate(V, Q[:, :0]),
                 lambda: S.eigsh_rotate(V.cpu(), Q), lambda: S.eigsh_rotate(V[:, ::2], Q),
                 lambda: S.eigsh_rotate(torch.ones((66, 10), dtype=torch.float64, device=cuda), torch.ones((65, 3), dtype=torch.float64, device=cuda))):
        with pytest.raises(S.SblasError):
            call()
    L = S.lib()
    assert L.sblas_hip_eigsh_rotate_f64(-1, None, 100, 8, 9, V.data_ptr(), 100, Q.data_ptr(), 8) == 1
    assert L.sblas_hip_eigsh_rotate_f64(-1, None, 100, 8, 4, V.data_ptr(), 99, Q.data_ptr(), 8) == 1
    assert L.sblas_hip_eigsh_rotate_f64(-1, None, 100, 65, 4, V.data_ptr(), 100, Q.data_ptr(), 65) == 1
    torch.cuda.synchronize()
    assert bool((V == 1.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# the Ritz kernel
# ---------------------------------------------------------------------------------------------------------------------
def test_ritz_kernel_is_the_host_ritz_step(env):
    S, torch, cuda = env
    seen = {}
    for label, T, beta, k, keep, which, kw in EN.ritz_cases():
        want = S.eigsh_ritz_ref(T, beta, k, keep, which, **kw)
        got = S.eigsh_ritz(T, beta, k, keep, which, device=cuda, **kw)
        assert np.array_equal(got["blk"], want["blk"]), (label, got["blk"], want["blk"])            # every slot, the status among them
        assert same(got["mat"], want["mat"]), label                                                     # T, Y, theta, rho, Q: every double
        seen[got["status"]] = seen.get(got["status"], 0) + 1
    assert set(seen) == {"running", "converged", "breakdown", "limit"}, seen


# ---------------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------------
_composed = {}


def composed(env, name, which, k, ncv):
    """the composition's result of a case, computed once and shared"""
    S, torch, cuda = env
    key = (name, which, k, ncv)
    if key not in _composed:
        csr = device_csr(torch, cuda, EN.dense(name))
        _composed[key] = (csr, EN.composed_eigsh(S, torch, cuda, csr, k, ncv, which, rtol=RTOL))
    return _composed[key]


def same_solve(st, vals, vecs, want, label):
    k = len(st["theta"])
    assert (st["status"], st["restarts"], st["matvecs"], st["converged"], st["breakdown"]) == \
        (want["status"], want["restarts"], want["matvecs"], want["converged"], want["breakdown"]), (label, st, want)
    assert same(st["theta"], want["theta"]) and same(st["residuals"], want["residuals"]), (label, st, want)
    assert same(vals.cpu().numpy(), want["theta"]), label
    cols = want["V"].shape[0]
    assert same(vecs.cpu().numpy()[:cols], want["V"]), label
    assert k == len(want["theta"])


@pytest.mark.parametrize("name,which,k,ncv", EN.CASES)
def test_solve_is_the_composition_at_every_check_every(env, name, which, k, ncv):
    S, torch, cuda = env
    csr, want = composed(env, name, which, k, ncv)
    assert want["status"] == "converged" and want["restarts"] <= 300, want
    n, drp, dci, dval = csr
    plan = S.EigshPlan(n, drp, dci, k, ncv=ncv, which=which)
    for every in (1, 3, 50):
        vals, vecs, st = plan.solve(dval, rtol=RTOL, check_every=every)
        same_solve(st, vals, vecs, want, (name, which, k, ncv, every))
    assert vecs.data_ptr() == plan.vectors().data_ptr() and vecs.stride() == plan.vectors().stride()      # a view of V, not a copy
    vecs, view = plan.vectors(copy=True), vecs
    assert vecs.data_ptr() != view.data_ptr() and vecs.is_contiguous() and same(vecs.cpu().numpy(), view.cpu().numpy())
    plan.iterate(5)                                                         # behind the end nothing changes
    st2 = plan.status()
    assert st2["status"] == st["status"] and st2["restarts"] == st["restarts"] and st2["matvecs"] == st["matvecs"]
    assert same(plan.vectors().cpu().numpy(), vecs.cpu().numpy()) and same(plan.values().cpu().numpy(), vals.cpu().numpy())
    # the eigenpairs, against LAPACK on the dense matrix (the bounds of tests/test_eigsh_host.py)
    A = EN.dense(name)
    worst = EN.check_pairs(A, np.linalg.eigvalsh(A), which, st["theta"], vecs.cpu().numpy(), RTOL, 0.0)
    # the restart count of the plain numpy loop on the same start vector
    loop = EN.numpy_eigsh(A, k, ncv, which, S.cheby_start_ref(n, seed=0), rtol=RTOL)
    print("%s %s k=%d ncv=%d: %d restarts (numpy loop %d), %d matvecs, worst ratios %.3g %.3g"
          % (name, which, k, ncv, st["restarts"], loop["restarts"], st["matvecs"], worst[0], worst[1]))
    assert loop["status"] == "converged" and loop["restarts"] == st["restarts"], (loop["restarts"], st["restarts"])
    info = plan.info()
    assert info["cycle_launches"] == 9 * (info["ncv"] - info["keep"]) + 2 and info["keep"] == EN.default_keep(k, ncv)
    plan.destroy()


@pytest.mark.parametrize("name,which,k,ncv", EN.CASES)
def test_iterate_replays_in_a_graph(env, name, which, k, ncv):
    S, torch, cuda = env
    csr, want = composed(env, name, which, k, ncv)
    n, drp, dci, dval = csr
    plan = S.EigshPlan(n, drp, dci, k, ncv=ncv, which=which)
    plan.solve(dval, rtol=RTOL)                                             # eager first: loads the code objects
    plan.start(dval, rtol=RTOL)                                             # start runs eagerly
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            plan.iterate(1)
    assert plan.status()["restarts"] == 0                                   # capturing ran nothing
    for replay in range(1, 302):
        g.replay()
        st = plan.status()
        if st["status"] != "running":
            break
    assert replay == want["restarts"]
    same_solve(st, plan.values(), plan.vectors(), want, (name, "graph"))
    plan.destroy()


def test_a_second_start_reuses_the_plan_and_an_spmv_plan_serves(env):
    S, torch, cuda = env
    A = EN.dense("grid")
    csr = device_csr(torch, cuda, A)
    n, drp, dci, dval = csr
    spmv = S.SpmvPlan(n, n, drp, dci)
    plan = S.EigshPlan(n, drp, dci, 4, ncv=20, which="SA", spmv_plan=spmv)
    for scale, seed_vec in ((1.0, None), (2.5, 3)):
        val = dval * scale
        v0 = None if seed_vec is None else up(torch, cuda, S.cheby_start_ref(n, seed=seed_vec))[0]
        want = EN.composed_eigsh(S, torch, cuda, (n, drp, dci, val), 4, 20, "SA", v0=v0, rtol=RTOL, planned=True)
        vals, vecs, st = plan.solve(val, v0=v0, rtol=RTOL, check_every=2)
        same_solve(st, vals, vecs, want, ("second start", scale))
        EN.check_pairs(A * scale, np.linalg.eigvalsh(A * scale), "SA", st["theta"], vecs.cpu().numpy(), RTOL, 0.0)
    plan.destroy()
    # the one shot, and a seed of its own
    vals, vecs, st = S.eigsh(csr, 4, which="SA", rtol=RTOL, seed=5)
    assert st["status"] == "converged"
    EN.check_pairs(A, np.linalg.eigvalsh(A), "SA", st["theta"], vecs.cpu().numpy(), RTOL, 0.0)
    spmv.destroy()


def test_max_restarts_ends_limit_with_the_best_estimates_in_place(env):
    S, torch, cuda = env
    csr = device_csr(torch, cuda, EN.dense("laplace"))
    n, drp, dci, dval = csr
    want = EN.composed_eigsh(S, torch, cuda, csr, 4, 20, "LA", rtol=RTOL, max_restarts=2)
    plan = S.EigshPlan(n, drp, dci, 4, ncv=20, which="LA")
    vals, vecs, st = plan.solve(dval, rtol=RTOL, max_restarts=2, check_every=7)
    assert st["status"] == "limit" and st["restarts"] == 2 and st["converged"] < 4
    same_solve(st, vals, vecs, want, "limit")
    X = vecs.cpu().numpy()
    A = EN.dense("laplace")
    assert np.abs(X @ X.T - np.eye(4)).max() < 1e-12                       # Ritz vectors, rotated into place
    assert np.allclose([X[i] @ A @ X[i] for i in range(4)], st["theta"], rtol=0, atol=1e-12)
    plan.destroy()


def test_an_invariant_subspace_converges_or_breaks_down(env):
    """diag(1 .. 70) and a start vector in the span of three eigenvectors: beta of step 2 is exactly 0 for this vector
    under the pinned dot, so the cycle ends at three columns"""
    S, torch, cuda = env
    n = 70
    csr = device_csr(torch, cuda, np.diag(np.arange(1.0, n + 1.0)))
    _, drp, dci, dval = csr
    v0 = np.zeros(n)
    v0[:3] = (2.0, -1.0, -1.0)
    dv0, = up(torch, cuda, v0)
    for k, status, breakdown in ((2, "converged", None), (4, "breakdown", "invariant")):
        want = EN.composed_eigsh(S, torch, cuda, csr, k, 20, "LA", v0=dv0, rtol=RTOL)
        plan = S.EigshPlan(n, drp, dci, k, ncv=20, which="LA")
        vals, vecs, st = plan.solve(dval, v0=dv0, rtol=RTOL)
        assert (st["status"], st["breakdown"], st["columns"], st["matvecs"], st["restarts"]) == (status, breakdown, 3, 3, 1), st
        same_solve(st, vals, vecs, want, ("invariant", k))
        # Jacobi's own error on the 3 x 3 T (tests/test_eigsh_host.py measures it), |T|_F <= sqrt(14)
        assert np.abs(st["theta"][:2] - [3.0, 2.0]).max() <= 64 * EN.EPS * 14 ** 0.5 and (st["residuals"] == 0.0).all()
        plan.destroy()


def test_values_that_are_not_finite_are_data(env):
    S, torch, cuda = env
    csr = device_csr(torch, cuda, EN.dense("grid"))
    n, drp, dci, dval = csr
    plan = S.EigshPlan(n, drp, dci, 4, ncv=20)
    bad = dval.clone()
    bad[17] = float("nan")
    _, _, st = plan.solve(bad, rtol=RTOL)
    assert (st["status"], st["breakdown"], st["restarts"]) == ("breakdown", "beta", 0), st
    zero = torch.zeros(n, dtype=torch.float64, device=cuda)
    _, _, st = plan.solve(dval, v0=zero, rtol=RTOL)
    assert (st["status"], st["breakdown"], st["matvecs"]) == ("breakdown", "v0", 0), st
    vals, vecs, st = plan.solve(dval, rtol=RTOL)                           # and the plan is whole behind both
    assert st["status"] == "converged"
    plan.destroy()


def test_plan_refusals_need_no_launch(env):
    S, torch, cuda = env
    csr = device_csr(torch, cuda, EN.dense("grid"))
    n, drp, dci, dval = csr
    other = device_csr(torch, cuda, EN.dense("laplace"))
    foreign = S.SpmvPlan(other[0], other[0], other[1], other[2])
    for kw in (dict(k=20, ncv=20), dict(k=4, ncv=65), dict(k=4, ncv=n), dict(k=4, ncv=20, keep=3), dict(k=4, ncv=20, keep=20),
               dict(k=4, which="BE"), dict(k=0), dict(k=4, spmv_plan=foreign), dict(k=4, spmv_plan="plan")):
        with pytest.raises(S.SblasError):
            S.EigshPlan(n, drp, dci, **kw)
    plan = S.EigshPlan(n, drp, dci, 4)
    for call in (lambda: plan.iterate(1), lambda: plan.status(), lambda: plan.start(dval[:-1]), lambda: plan.start(dval, rtol=-1.0),
                 lambda: plan.start(dval, v0=dval), lambda: plan.solve(dval, check_every=0)):
        with pytest.raises(S.SblasError):
            call()
    plan.destroy()
    foreign.destroy()
