"""The Krylov solvers on the GPU (KrylovPlan, krylov_dot, pcg, bicgstab) against tests/krylov_numerics.py.

Every bit is pinned, so most checks are ==: the device dot against its host restatement, each fused update against numpy's
expression of the same shape, and a whole solve against a loop composed (in tests/solver_compose.py) from SpmvPlan, Ilu0Plan.apply,
krylov_dot and numpy updates with the scalar steps in Python floats.  Only "it solves" holds a tolerance, and that one
comes from the host loop's own residual."""
import math

import numpy as np
import pytest

import color_numerics as CN
import ilu0_numerics as IN
import krylov_numerics as KN
import solver_compose as SC

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


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "mixed", "special"])
def test_dot_has_the_reference_bits(env, kind):
    S, torch, cuda = env
    for n in KN.sizes():
        x, y = KN.vectors(kind, n)
        dx, dy = up(torch, cuda, x, y)
        got = S.krylov_dot(dx, dy).cpu().numpy()
        want = S.krylov_dot_ref(x, y)
        assert got.shape == (1,) and same(got[0], want), (kind, n, got[0], want)
        if kind == "random":
            assert got[0] == want


def test_dot_at_odd_offsets_and_on_a_side_stream(env):
    S, torch, cuda = env
    s = torch.cuda.Stream()
    for n in (257, KN.CELL + 1, 3 * KN.CELL + 5):
        x, y = KN.vectors("mixed", n, seed=1)
        want = S.krylov_dot_ref(x, y)
        for off_x, off_y in ((1, 0), (3, 5), (0, 7)):
            bx = torch.zeros(n + 8, dtype=torch.float64, device=cuda)
            by = torch.zeros(n + 8, dtype=torch.float64, device=cuda)
            bx[off_x:off_x + n] = torch.from_numpy(x).to(cuda)
            by[off_y:off_y + n] = torch.from_numpy(y).to(cuda)
            out = torch.empty(1, dtype=torch.float64, device=cuda)
            ws = torch.empty(-(-n // KN.CELL), dtype=torch.float64, device=cuda)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                assert S.krylov_dot(bx[off_x:off_x + n], by[off_y:off_y + n], out=out, workspace=ws) is out
            s.synchronize()
            assert same(out.cpu().numpy()[0], want), (n, off_x, off_y)


def test_multi_dot_has_the_single_dots_bits(env):
    S, torch, cuda = env
    for n in (1, 255, KN.CELL, 3 * KN.CELL + 5, KN.WIDTH * KN.CELL + 3):
        t, s = KN.vectors("mixed", n, seed=2)
        r, _ = KN.vectors("random", n, seed=3)
        dt, ds, dr = up(torch, cuda, t, s, r)
        single = lambda a, b: S.krylov_dot(a, b).cpu().numpy()[0]
        two = S.krylov_dots([(dt, ds), (dt, dt)]).cpu().numpy()
        assert same(two, [single(dt, ds), single(dt, dt)]), n
        three = S.krylov_dots([(dr, dt), (dr, dr), (ds, ds)]).cpu().numpy()
        assert same(three, [single(dr, dt), single(dr, dr), single(ds, ds)]), n
        assert same(three[1], S.krylov_dot_ref(r, r))
    with pytest.raises(S.SblasError):
        S.krylov_dots([(dt, ds)] * 4)
    with pytest.raises(S.SblasError):
        S.krylov_dot(dt, ds[:-1])
    with pytest.raises(S.SblasError):
        S.krylov_dot(dt, ds, workspace=torch.empty(1, dtype=torch.float64, device=cuda))   # too short: refused, not overrun


def stage1(S, torch, cuda, a, b):
    """the cells' sums of (a, b) as the dot's own first stage leaves them in its workspace"""
    n = a.numel()
    ws = torch.zeros(-(-n // KN.CELL), dtype=torch.float64, device=cuda)
    S.krylov_dot(a, b, workspace=ws)
    return ws.cpu().numpy()


@pytest.mark.parametrize("n", [1, 257, KN.CELL + 1, 3 * KN.CELL + 5])
def test_fused_updates_round_twice_and_carry_the_dots_first_stage(env, n):
    S, torch, cuda = env
    rng = np.random.default_rng(n)
    cells = -(-n // KN.CELL)
    alpha, beta, omega = 0.7310585786300049, -1.3678794411714423, 0.6224593312018546
    scal = np.zeros(16)
    scal[4:7] = alpha, beta, omega
    dscal, = up(torch, cuda, scal)
    vec = lambda: rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
    part = lambda: torch.full((2 * cells,), -7.0, dtype=torch.float64, device=cuda)
    for jac in (False, True):
        # PCG: x = x + alpha p, r = r - alpha q [, z = dinv r]
        x, r, p, q, dinv = vec(), vec(), vec(), vec(), vec()
        d = up(torch, cuda, x, r, p, q, dinv, np.full(n, -7.0))
        pt = part()
        S.krylov_update("pcg_xr", dscal, d[:6] if jac else d[:4], partial=pt, jacobi=jac)
        r1 = r - alpha * q
        assert same(d[0].cpu().numpy(), x + alpha * p) and same(d[1].cpu().numpy(), r1), (n, jac)
        assert same(pt.cpu().numpy()[:cells], stage1(S, torch, cuda, d[1], d[1])), (n, jac)
        if jac:
            assert same(d[5].cpu().numpy(), dinv * r1)
            assert same(pt.cpu().numpy()[cells:], stage1(S, torch, cuda, d[1], d[5]))
        # BiCGStab: p = r + beta (p - omega v) [, p^ = dinv p];  s = r - alpha v [, s^ = dinv s]
        p, r, v = vec(), vec(), vec()
        d = up(torch, cuda, p, r, v, dinv, np.full(n, -7.0))
        S.krylov_update("bicg_p", dscal, d if jac else d[:3], jacobi=jac)
        p1 = r + beta * (p - omega * v)
        assert same(d[0].cpu().numpy(), p1), (n, jac)
        assert same(d[4].cpu().numpy(), dinv * p1 if jac else np.full(n, -7.0))
        d = up(torch, cuda, np.full(n, -7.0), r, v, dinv, np.full(n, -7.0))
        S.krylov_update("bicg_s", dscal, d if jac else d[:3], jacobi=jac)
        s1 = r - alpha * v
        assert same(d[0].cpu().numpy(), s1), (n, jac)
        assert same(d[4].cpu().numpy(), dinv * s1 if jac else np.full(n, -7.0))
    # PCG: p = z + beta p
    p, z = vec(), vec()
    d = up(torch, cuda, p, z)
    S.krylov_update("pcg_p", dscal, d)
    assert same(d[0].cpu().numpy(), z + beta * p)
    # BiCGStab: x = (x + alpha p^) + omega s^, r = s - omega t, with (r, r) and (r^, r)
    x, ph, sh, s, t, rh = vec(), vec(), vec(), vec(), vec(), vec()
    d = up(torch, cuda, x, np.full(n, -7.0), ph, sh, s, t, rh)
    pt = part()
    S.krylov_update("bicg_xr", dscal, d, partial=pt)
    assert same(d[0].cpu().numpy(), (x + alpha * ph) + omega * sh) and same(d[1].cpu().numpy(), s - omega * t)
    assert same(pt.cpu().numpy()[:cells], stage1(S, torch, cuda, d[1], d[1]))
    assert same(pt.cpu().numpy()[cells:], stage1(S, torch, cuda, d[6], d[1]))
    # a status that is not "running": the update returns at entry
    dscal.view(torch.int64)[0] = 1
    d = up(torch, cuda, x, np.full(n, -7.0), ph, sh, s, t, rh)
    pt = part()
    S.krylov_update("bicg_xr", dscal, d, partial=pt)
    assert same(d[0].cpu().numpy(), x) and bool((d[1] == -7.0).all()) and bool((pt == -7.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# the solver equals its own composition
# ---------------------------------------------------------------------------------------------------------------------
Parts, composed_pcg, composed_bicgstab = SC.Parts, SC.composed_pcg, SC.composed_bicgstab


CASES = [("pcg", "laplacian32", "ilu0", True), ("pcg", "laplacian32", "jacobi", True), ("pcg", "laplacian32", None, False),
         ("pcg", "spd24", "ilu0", True), ("bicgstab", "convection24", "ilu0", True), ("bicgstab", "convection24", None, True)]
MATRICES = {"laplacian32": lambda: KN.laplacian(32), "spd24": lambda: KN.spd_perturbed(24),
            "convection24": lambda: KN.convection_diffusion(24)}


@pytest.mark.parametrize("method,matrix,precond,planned", CASES)
def test_the_solver_equals_its_own_composition(env, method, matrix, precond, planned):
    S, torch, cuda = env
    n, rp, ci, val = MATRICES[matrix]()
    rng = np.random.default_rng(30)
    b, x0 = rng.standard_normal(n), 0.1 * rng.standard_normal(n)
    P = Parts(env, n, rp, ci, val, precond, planned=planned)
    want_x, want_it, want_rnorm, want_status = (composed_pcg if method == "pcg" else composed_bicgstab)(P.matvec, P.apply, P.dot, b, x0, RTOL, 1000)
    plan = P.plan(method)
    info = plan.info()
    db, dx = up(torch, cuda, b, x0)
    x, st = plan.solve(P.dval, db, x=dx, rtol=RTOL, max_iter=1000, check_every=16, **P.kw())
    assert x is dx
    print("%s on %s with %s: %d iterations, |r| = %.3e (composition: %d, %.3e); %d launches an iteration, %d bytes held"
          % (method, matrix, precond, st["iterations"], st["rnorm"], want_it, want_rnorm, info["launches"], info["bytes"]))
    assert want_status == "converged" and 0 < want_it < 400
    assert (st["status"], st["iterations"]) == (want_status, want_it), st
    assert same(st["rnorm"], want_rnorm) and same(st["bnorm"], math.sqrt(S.krylov_dot_ref(b, b)))
    assert same(x.cpu().numpy(), want_x)
    extra = 1 if precond == "ilu0" else 0
    lim = S.krylov_limits()
    assert info["vectors"] == (lim["pcg_vectors"] if method == "pcg" else lim["bicgstab_vectors"]) + extra
    assert info["vector_bytes"] >= 8 * n and info["bytes"] >= info["vectors"] * info["vector_bytes"] + info["partial_bytes"] + info["scalar_bytes"]
    solves = [q.info()["launches"] for q in P.ilu.solvers()] if precond == "ilu0" else [0, 0]
    assert info["launches"] == S.krylov_launches(method, precond, *solves)
    plan.destroy(), P.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# the freeze
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lap(env):
    """the 32 x 32 Laplacian with ILU(0) on the device, b from rng(30), and the host loop's count and iterate"""
    n, rp, ci, val = KN.laplacian(32)
    b = np.random.default_rng(30).standard_normal(n)
    P = Parts(env, n, rp, ci, val, "ilu0")
    host_it, host_x = KN.host_pcg(n, rp, ci, val, b, IN.ilu0_ref(n, rp, ci, val), RTOL)
    yield dict(n=n, rp=rp, ci=ci, val=val, b=b, P=P, host_it=host_it, host_x=host_x)
    P.destroy()


@pytest.mark.parametrize("method", ["pcg", "bicgstab"])
def test_the_result_does_not_depend_on_check_every(env, lap, method):
    S, torch, cuda = env
    P = lap["P"]
    plan = P.plan(method)
    db, = up(torch, cuda, lap["b"])
    runs = []
    for every in (1, 7, 50):
        dx, st = plan.solve(P.dval, db, rtol=RTOL, check_every=every, **P.kw())
        runs.append((dx.cpu().numpy(), st))
    for x, st in runs[1:]:
        assert same(x, runs[0][0]) and st == runs[0][1], (st, runs[0][1])
    assert runs[0][1]["status"] == "converged" and runs[0][1]["rnorm"] <= RTOL * runs[0][1]["bnorm"]
    # after convergence further iterations change nothing
    plan.iterate(5)
    assert plan.status() == runs[0][1] and same(dx.cpu().numpy(), runs[0][0])
    # fewer iterations than needed: exactly max_iter, and "limit"
    few = runs[0][1]["iterations"] - 3
    x, st = plan.solve(P.dval, db, rtol=RTOL, max_iter=few, check_every=50, **P.kw())
    assert (st["status"], st["iterations"]) == ("limit", few) and st["rnorm"] > RTOL * st["bnorm"], st
    x2, st2 = plan.solve(P.dval, db, rtol=RTOL, max_iter=few, check_every=1, **P.kw())
    assert st2 == st and same(x2.cpu().numpy(), x.cpu().numpy())
    plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# it solves
# ---------------------------------------------------------------------------------------------------------------------
def true_residual(n, rp, ci, val, b, x):
    return float(np.linalg.norm(b - KN.matvec(n, rp, ci, val, x)))


def test_pcg_meets_the_host_loops_counts_and_residual(env, lap):
    """Measured on an MI355X: see DESIGN.md 3.22 for the counts and the two residuals this prints."""
    S, torch, cuda = env
    n, rp, ci, val, b, P = (lap[k] for k in ("n", "rp", "ci", "val", "b", "P"))
    db, = up(torch, cuda, b)
    x, st = S.pcg((n, P.drp, P.dci, P.dval), db, precond="ilu0", rtol=RTOL)
    _, plain = S.pcg((n, P.drp, P.dci, P.dval), db, rtol=RTOL)
    got = true_residual(n, rp, ci, val, b, x.cpu().numpy())
    host = true_residual(n, rp, ci, val, b, lap["host_x"])
    bound = 2.0 * max(host, RTOL * np.linalg.norm(b))
    print("PCG with ILU(0): device %d iterations, host loop %d, plain CG on the device %d; true residual %.6e, the host loop's "
          "%.6e, bound %.6e" % (st["iterations"], lap["host_it"], plain["iterations"], got, host, bound))
    assert st["status"] == plain["status"] == "converged"
    assert st["iterations"] <= lap["host_it"] + 2
    assert 2 * st["iterations"] < plain["iterations"]
    assert got <= bound


def test_pcg_in_the_multicolour_order(env, lap):
    S, torch, cuda = env
    n, rp, ci, val, b, P = (lap[k] for k in ("n", "rp", "ci", "val", "b", "P"))
    db, = up(torch, cuda, b)
    color = S.ColorPlan(n, P.drp, P.dci)
    perm = color.permute(P.drp, P.dci)
    color.destroy()
    drpb, dcib, _ = perm.csr()
    dvalb, bb = perm.values(P.dval), perm.to_permuted(db)
    ilu = S.Ilu0Plan(n, drpb, dcib)
    lu = ilu.factor(dvalb)
    plan = S.KrylovPlan(n, drpb, dcib, precond=ilu)
    xb, st = plan.solve(dvalb, bb, lu=lu, rtol=RTOL)
    x = perm.from_permuted(xb).cpu().numpy()
    order = perm.perm.cpu().numpy()
    rpb, cib, src = CN.permute(n, rp, ci, order)
    host_it, host_xb = KN.host_pcg(n, rpb, cib, val[src], b[order], IN.ilu0_ref(n, rpb, cib, val[src]), RTOL)
    got = true_residual(n, rp, ci, val, b, x)
    host = true_residual(n, rpb, cib, val[src], b[order], host_xb)
    bound = 2.0 * max(host, RTOL * np.linalg.norm(b))
    print("PCG with ILU(0) in the multicolour order: device %d iterations, host loop %d; true residual of x mapped back %.6e, "
          "the host loop's %.6e, bound %.6e" % (st["iterations"], host_it, got, host, bound))
    assert st["status"] == "converged" and abs(st["iterations"] - host_it) <= 2
    assert got <= bound
    plan.destroy(), ilu.destroy(), perm.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------------------------------------------------
def diagonal_system(env, d):
    S, torch, cuda = env
    n = len(d)
    return (n,) + tuple(up(torch, cuda, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.asarray(d, np.float64)))


@pytest.mark.parametrize("method", ["pcg", "bicgstab"])
def test_edges(env, lap, method):
    S, torch, cuda = env
    solve = S.pcg if method == "pcg" else S.bicgstab
    # n == 0
    x, st = solve(diagonal_system(env, []), torch.empty(0, dtype=torch.float64, device=cuda))
    assert x.numel() == 0 and (st["status"], st["iterations"]) == ("converged", 0)
    # n == 1
    x, st = solve(diagonal_system(env, [2.0]), up(torch, cuda, np.array([3.0]))[0])
    assert st["status"] == "converged" and st["iterations"] == 1 and x.cpu().numpy()[0] == 1.5, st
    # b == 0: x = 0 whatever the guess, at iteration 0, and nothing was divided
    n, P = lap["n"], lap["P"]
    A = (n, P.drp, P.dci, P.dval)
    x, st = solve(A, torch.zeros(n, dtype=torch.float64, device=cuda), x=torch.full((n,), -7.0, dtype=torch.float64, device=cuda))
    assert (st["status"], st["iterations"], st["rnorm"], st["bnorm"]) == ("converged", 0, 0.0, 0.0), st
    assert bool((x == 0.0).all()) and st["alpha"] == 0.0 and st["beta"] == 0.0
    # the guess is the solution: small integers, so b = A x is exact and r = 0
    xs = np.random.default_rng(5).integers(-8, 9, n).astype(np.float64)
    db, dx = up(torch, cuda, KN.matvec(n, lap["rp"], lap["ci"], lap["val"], xs), xs)
    x, st = solve(A, db, x=dx, precond="ilu0")
    assert (st["status"], st["iterations"], st["rnorm"]) == ("converged", 0, 0.0) and same(x.cpu().numpy(), xs), st
    # max_iter == 0 with work to do
    x, st = solve(A, db, max_iter=0)
    assert (st["status"], st["iterations"]) == ("limit", 0) and bool((x == 0.0).all())


def test_a_singular_system_breaks_down_and_names_the_denominator(env):
    S, torch, cuda = env
    # diag(1, 0, 1, 0) x = 1: after one iteration x = 2, r = (-1, 1, -1, 1), beta = 1, p = (0, 2, 0, 2), and A p = 0
    A = diagonal_system(env, [1.0, 0.0, 1.0, 0.0])
    x, st = S.pcg(A, torch.ones(4, dtype=torch.float64, device=cuda), max_iter=50, check_every=50)
    assert (st["status"], st["breakdown"], st["iterations"]) == ("breakdown", "(p, q)", 1), st
    assert same(x.cpu().numpy(), np.full(4, 2.0)) and st["rnorm"] == 2.0 and st["alpha"] == 2.0 and st["beta"] == 1.0
    # A = 0: BiCGStab's first (r^, v) is 0
    x, st = S.bicgstab(diagonal_system(env, [0.0, 0.0, 0.0]), torch.ones(3, dtype=torch.float64, device=cuda), max_iter=50)
    assert (st["status"], st["breakdown"], st["iterations"]) == ("breakdown", "(r^, v)", 0), st
    assert bool((x == 0.0).all())


@pytest.mark.parametrize("method", ["pcg", "bicgstab"])
def test_a_nan_in_val_never_converges(env, lap, method):
    S, torch, cuda = env
    n, P = lap["n"], lap["P"]
    dval = P.dval.clone()
    dval[7] = float("nan")
    db, = up(torch, cuda, lap["b"])
    x, st = (S.pcg if method == "pcg" else S.bicgstab)((n, P.drp, P.dci, dval), db, max_iter=20, check_every=20)
    assert st["status"] in ("breakdown", "limit"), st


def test_refusals_launch_nothing(env, lap):
    S, torch, cuda = env
    E = S.SblasError
    n, P = lap["n"], lap["P"]
    db, = up(torch, cuda, lap["b"])
    x = torch.full((n,), -7.0, dtype=torch.float64, device=cuda)
    plan = P.plan("pcg")
    lower, upper = P.ilu.solvers()
    other_rp = P.drp.clone()
    foreign = S.Ilu0Plan(n, other_rp, P.dci)
    bad = [lambda: plan.solve(P.dval, db.cpu(), x=x, lu=P.lu), lambda: plan.solve(P.dval, db, x=x.cpu(), lu=P.lu),
           lambda: plan.solve(P.dval.cpu(), db, x=x, lu=P.lu), lambda: plan.solve(P.dval, db.float(), x=x, lu=P.lu),
           lambda: plan.solve(P.dval, db[:-1], x=x, lu=P.lu), lambda: plan.solve(P.dval[:-1], db, x=x, lu=P.lu),
           lambda: plan.solve(P.dval, db, x=x, lu=P.lu[:-1]), lambda: plan.solve(P.dval, db, x=x), lambda: plan.solve(P.dval, x, x=x, lu=P.lu),
           lambda: plan.solve(P.dval, db, x=x, lu=P.lu, rtol=-1.0), lambda: plan.solve(P.dval, db, x=x, lu=P.lu, rtol=float("nan")),
           lambda: plan.solve(P.dval, db, x=x, lu=P.lu, max_iter=-1), lambda: plan.solve(P.dval, db, x=x, lu=P.lu, check_every=0),
           lambda: S.KrylovPlan(n, other_rp, P.dci, precond=P.ilu),              # the solves were planned on another rowptr
           lambda: S.KrylovPlan(n, P.drp, P.dci, precond=foreign),
           lambda: S.KrylovPlan(n, other_rp, P.dci, spmv_plan=P.spmv),
           lambda: S.KrylovPlan(n, P.drp, P.dci, precond=(upper, lower)),        # a lower plan given as upper
           lambda: S.KrylovPlan(n, P.drp, P.dci, precond=(lower, lower)),
           lambda: S.KrylovPlan(n, P.drp, P.dci, precond="ssor"), lambda: S.KrylovPlan(n, P.drp, P.dci, method="gmres"),
           lambda: S.KrylovPlan(n + 1, P.drp, P.dci), lambda: S.KrylovPlan(n, P.drp.long(), P.dci),
           lambda: S.KrylovPlan(n, P.drp, P.dci, precond="jacobi").solve(P.dval, db, x=x),
           lambda: S.pcg((n, P.drp, P.dci, P.dval), db, precond="ssor", x=x)]
    for k, call in enumerate(bad):
        with pytest.raises(E):
            call()
            pytest.fail("call %d was accepted" % k)
    fresh = P.plan("pcg")
    with pytest.raises(E):
        fresh.iterate(1)                                                     # before start
    with pytest.raises(E):
        fresh.status()
    L = S.lib()
    assert L.sblas_hip_krylov_start(None, None, P.dval.data_ptr(), P.lu.data_ptr(), db.data_ptr(), x.data_ptr(), 1e-8, 0.0, 10) == 1
    assert L.sblas_hip_krylov_start(fresh.handle, None, P.dval.data_ptr(), None, db.data_ptr(), x.data_ptr(), 1e-8, 0.0, 10) == 1
    assert L.sblas_hip_krylov_start(fresh.handle, None, P.dval.data_ptr(), P.lu.data_ptr(), None, x.data_ptr(), 1e-8, 0.0, 10) == 1
    torch.cuda.synchronize()
    assert bool((x == -7.0).all())                                           # nothing ran
    assert S.KrylovPlan(n, P.drp, P.dci, precond=(lower, upper)).info()["precond"] == "ilu0"
    plan.destroy(), fresh.destroy(), foreign.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# graph
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["pcg", "bicgstab"])
def test_iterate_replays_in_a_graph(env, lap, method):
    S, torch, cuda = env
    n, P = lap["n"], lap["P"]
    db, = up(torch, cuda, lap["b"])
    plan = P.plan(method)
    ex, est = plan.solve(P.dval, db, rtol=RTOL, check_every=4, **P.kw())   # eager: the count and bits to meet; loads the code objects
    ex = ex.clone()
    x = torch.zeros(n, dtype=torch.float64, device=cuda)
    plan.start(P.dval, db, x, rtol=RTOL, **P.kw())                           # start runs eagerly
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):                                 # a linear chain of launches
            plan.iterate(4)
    st = plan.status()
    assert (st["status"], st["iterations"]) == ("running", 0)              # capturing ran nothing
    for replay in range(1, 101):
        g.replay()
        st = plan.status()
        if st["status"] != "running":
            break
    assert st == est and replay == -(-est["iterations"] // 4), (st, est, replay)
    assert same(x.cpu().numpy(), ex.cpu().numpy())
    plan.destroy()
