"""Restarted GMRES on the GPU (GmresPlan, gmres, gmres_dots, gmres_project, gmres_combine) against tests/gmres_numerics.py.

Every bit is pinned, so most checks are ==: the multi-dot against the single pinned dot column by column, the projection
and the combination against numpy's expression of the same shape, and a whole solve against a loop composed (in
tests/solver_compose.py) from SpmvPlan / spmv, Ilu0Plan.apply, krylov_dot, numpy updates and the scalar step in Python floats.  Only "it solves"
holds a tolerance, and that one comes from a host GMRES's own residual."""
import numpy as np
import pytest

import gmres_numerics as GN
import ilu0_numerics as IN
import krylov_numerics as KN
import solver_compose as SC

pytestmark = pytest.mark.gpu

RTOL = 1e-10
CELL = KN.CELL


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
def columns(kind, n, k):
    """(V as a (k, n) array, w): the test vectors of the Krylov dots, a fresh seed a column"""
    w = KN.vectors(kind, n, seed=0)[1]
    return np.stack([KN.vectors(kind, n, seed=1 + i)[0] for i in range(k)]), w


def strided(torch, cuda, V, ldv, offset):
    """V's columns in a buffer with column stride ldv > n, starting at an odd element: a (k, n) view"""
    k, n = V.shape
    buf = torch.full((offset + k * ldv,), -7.0, dtype=torch.float64, device=cuda)
    view = buf[offset:offset + k * ldv].view(k, ldv)[:, :n]
    view.copy_(torch.from_numpy(V).to(cuda))
    return view


@pytest.mark.parametrize("kind", ["mixed", "special"])
def test_multi_dot_has_the_single_dots_bits(env, kind):
    S, torch, cuda = env
    side = torch.cuda.Stream()
    for n in (1, 255, CELL, CELL + 1, 3 * CELL + 5):
        V, w = columns(kind, n, 65)
        dV, dw = up(torch, cuda, V, w)
        single = np.array([S.krylov_dot(dV[i], dw).cpu().numpy()[0] for i in range(65)])
        assert same(single[0], S.krylov_dot_ref(V[0], w))
        for k in (1, 2, 7, 33, 65):
            got = S.gmres_dots(dV[:k], dw).cpu().numpy()
            assert got.shape == (k,) and same(got, single[:k]), (kind, n, k)
        # a column stride larger than n and an odd element offset, on a side stream, into a caller's out and workspace
        for k, ldv, off in ((7, n + 3, 1), (65, n + 9, 3), (1, n + 1, 5)):
            view = strided(torch, cuda, V[:k], ldv, off)
            out = torch.empty(k, dtype=torch.float64, device=cuda)
            ws = torch.full((k * -(-n // CELL) + 2,), -7.0, dtype=torch.float64, device=cuda)
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                assert S.gmres_dots(view, dw, out=out, workspace=ws) is out
            side.synchronize()
            assert same(out.cpu().numpy(), single[:k]), (kind, n, k, ldv, off)
            assert bool((ws[-2:] == -7.0).all())                             # the workspace's own size, not more


def test_multi_dot_with_more_cells_than_the_second_stage_has_lanes(env):
    S, torch, cuda = env
    n = KN.WIDTH * CELL + 3
    V, w = columns("mixed", n, 3)
    dV, dw = up(torch, cuda, V, w)
    got = S.gmres_dots(dV, dw).cpu().numpy()
    want = [S.krylov_dot(dV[i], dw).cpu().numpy()[0] for i in range(3)]
    assert same(got, want) and same(got[1], S.krylov_dot_ref(V[1], w))


def test_multi_dot_refusals(env):
    S, torch, cuda = env
    n = CELL + 1
    V = torch.ones((66, n), dtype=torch.float64, device=cuda)
    w = torch.ones(n, dtype=torch.float64, device=cuda)
    out = torch.full((66,), -7.0, dtype=torch.float64, device=cuda)
    ws = torch.full((66 * 2,), -7.0, dtype=torch.float64, device=cuda)
    E = S.SblasError
    for call in (lambda: S.gmres_dots(V[:0], w), lambda: S.gmres_dots(V, w), lambda: S.gmres_dots(V[:3], w[:-1]),
                 lambda: S.gmres_dots(V[:3], w, workspace=ws[:5]),           # too short: refused, not overrun
                 lambda: S.gmres_dots(V[:3], w, out=out[:2]), lambda: S.gmres_dots(V[:3].float(), w),
                 lambda: S.gmres_dots(V[:3, ::2], w[:-(n // 2)]),           # a column must be contiguous
                 lambda: S.gmres_project(V[:3], w[:2], w), lambda: S.gmres_combine(V[:3], w[:4]),
                 lambda: S.gmres_project(V[:3], w[:3], w.clone(), partial=ws[:1])):
        with pytest.raises(E):
            call()
    L = S.lib()
    args = lambda k, wbytes: (-1, None, n, k, V.data_ptr(), n, w.data_ptr(), out.data_ptr(), ws.data_ptr(), wbytes)
    assert L.sblas_hip_gmres_dots_f64(*args(0, ws.numel() * 8)) == 1
    assert L.sblas_hip_gmres_dots_f64(*args(66, ws.numel() * 8)) == 1
    assert L.sblas_hip_gmres_dots_f64(*args(3, 3 * 2 * 8 - 8)) != 0
    assert L.sblas_hip_gmres_dots_f64(-1, None, n, 3, V.data_ptr(), n - 1, w.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel() * 8) == 1
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((ws == -7.0).all())           # nothing ran


def stage1(S, torch, cuda, a, b):
    """the cells' sums of (a, b) as the dot's own first stage leaves them in its workspace"""
    ws = torch.zeros(-(-a.numel() // CELL), dtype=torch.float64, device=cuda)
    S.krylov_dot(a, b, workspace=ws)
    return ws.cpu().numpy()


@pytest.mark.parametrize("n", [1, 257, CELL + 1, 3 * CELL + 5])
def test_projection_and_combination_round_twice(env, n):
    S, torch, cuda = env
    rng = np.random.default_rng(n)
    cells = -(-n // CELL)
    for k in (1, 4, 65):
        V = rng.standard_normal((k, n)) * 10.0 ** rng.integers(-3, 4, (k, n))
        w = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
        h = rng.standard_normal(k) * 10.0 ** rng.integers(-2, 3, k)
        dh, = up(torch, cuda, h)
        want = w.copy()
        for i in range(k):
            want = want - h[i] * V[i]
        comb = h[0] * V[0]
        for i in range(1, k):
            comb = comb + h[i] * V[i]
        for ldv, off in ((n, 0), (n + 3, 1)):
            dV = strided(torch, cuda, V, ldv, off)
            dw, = up(torch, cuda, w)
            part = torch.full((cells + 1,), -7.0, dtype=torch.float64, device=cuda)
            assert S.gmres_project(dV, dh, dw, partial=part) is dw
            assert same(dw.cpu().numpy(), want), (n, k, ldv)
            assert same(part.cpu().numpy()[:cells], stage1(S, torch, cuda, dw, dw)) and float(part[cells]) == -7.0, (n, k, ldv)
            dw, = up(torch, cuda, w)
            S.gmres_project(dV, dh, dw)                                      # without the partial: the same w
            assert same(dw.cpu().numpy(), want)
            u = torch.full((n,), -7.0, dtype=torch.float64, device=cuda)
            assert S.gmres_combine(dV, dh, out=u) is u
            assert same(u.cpu().numpy(), comb), (n, k, ldv)


# ---------------------------------------------------------------------------------------------------------------------
# the solver equals its own composition
# ---------------------------------------------------------------------------------------------------------------------
Parts, composed_gmres = SC.Parts, SC.composed_gmres


def agrees(st, x, want):
    assert (st["status"], st["iterations"], st["restarts"], st["columns"], st["breakdown"]) == \
        (want["status"], want["iterations"], want["restarts"], want["columns"], want["breakdown"]), (st, {k: v for k, v in want.items() if k != "x"})
    assert same(st["rnorm"], want["rnorm"]) and same(st["bnorm"], want["bnorm"]), (st, want["rnorm"], want["bnorm"])
    assert same(x.cpu().numpy(), want["x"])


def problem(matrix):
    n, rp, ci, val = matrix
    rng = np.random.default_rng(30)
    return n, rp, ci, val, rng.standard_normal(n), 0.1 * rng.standard_normal(n)


CASES = [("convection24", 5, None, True), ("convection24", 30, None, True), ("convection24", 64, None, True),
         ("convection24", 30, "jacobi", True), ("convection24", 30, "ilu0", True), ("convection24", 30, "ilu0", False),
         ("convection8", 1, None, True), ("laplacian32", 30, "ilu0", True)]
MATRICES = {"convection24": lambda: KN.convection_diffusion(24), "convection8": lambda: KN.convection_diffusion(8),
            "laplacian32": lambda: KN.laplacian(32)}


@pytest.mark.parametrize("matrix,restart,precond,planned", CASES)
def test_the_solver_equals_its_own_composition(env, matrix, restart, precond, planned):
    S, torch, cuda = env
    n, rp, ci, val, b, x0 = problem(MATRICES[matrix]())
    P = Parts(env, n, rp, ci, val, precond, planned=planned)
    want = composed_gmres(P.matvec, P.apply, P.dot, P.dots, b, x0, restart, RTOL, 1000)
    plan = P.plan(restart)
    info = plan.info()
    db, dx = up(torch, cuda, b, x0)
    x, st = plan.solve(P.dval, db, x=dx, rtol=RTOL, max_iter=1000, check_every=16, **P.kw())
    assert x is dx
    print("GMRES(%d) on %s with %s: %d steps, %d restarts, |r| = %.3e (composition: %d, %d, %.3e); %d launches a step, %d bytes held"
          % (restart, matrix, precond, st["iterations"], st["restarts"], st["rnorm"], want["iterations"], want["restarts"], want["rnorm"],
             info["step_launches"], info["bytes"]))
    assert want["status"] == "converged" and 0 < want["iterations"] < 400    # about the inputs: a host float64 GMRES meets it
    agrees(st, x, want)
    lim = S.gmres_limits()
    assert info["restart"] == restart and info["precond"] == precond
    assert info["vectors"] == lim["vectors_per_restart"] * restart + lim["vectors_fixed"] + (1 if precond == "ilu0" else 0)
    assert info["vector_bytes"] >= 8 * n and info["partial_bytes"] >= 8 * (restart + 1) * -(-n // CELL)
    assert info["bytes"] >= info["vectors"] * info["vector_bytes"] + info["partial_bytes"] + info["scalar_bytes"] + info["matrix_bytes"]
    solves = [q.info()["launches"] for q in P.ilu.solvers()] if precond == "ilu0" else [0, 0]
    L = S.gmres_launches(restart, precond, *solves)
    assert (info["step_launches"], info["close_launches"], info["restart_launches"], info["cycle_launches"]) == \
        (L["step"], L["close"], L["restart"], L["cycle"])
    plan.destroy(), P.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# the freeze, the graph, and "it solves": GMRES(5) on the 24 x 24 convection-diffusion grid
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def conv(env):
    n, rp, ci, val, b, x0 = problem(KN.convection_diffusion(24))
    P = Parts(env, n, rp, ci, val, None)
    yield dict(n=n, rp=rp, ci=ci, val=val, b=b, x0=x0, P=P)
    P.destroy()


def test_the_result_does_not_depend_on_check_every(env, conv):
    S, torch, cuda = env
    P = conv["P"]
    plan = P.plan(5)
    db, = up(torch, cuda, conv["b"])
    runs = []
    for every in (1, 7, 50):
        dx, = up(torch, cuda, conv["x0"])
        x, st = plan.solve(P.dval, db, x=dx, rtol=RTOL, check_every=every)
        runs.append((x.cpu().numpy(), st))
    for x, st in runs[1:]:
        assert same(x, runs[0][0]) and st == runs[0][1], (st, runs[0][1])
    st = runs[0][1]
    assert st["status"] == "converged" and st["rnorm"] <= RTOL * st["bnorm"] and st["restarts"] > 2
    # after the end further iterations change nothing: not x, not the status
    plan.iterate(9)
    assert plan.status() == st and same(dx.cpu().numpy(), runs[0][0])
    plan.destroy()


def test_max_iter_stops_at_exactly_max_iter(env, conv):
    S, torch, cuda = env
    P = conv["P"]
    plan = P.plan(5)
    db, = up(torch, cuda, conv["b"])
    want = composed_gmres(P.matvec, P.apply, P.dot, P.dots, conv["b"], conv["x0"], 5, RTOL, 7)   # a full cycle, a restart, two columns, the limit
    assert (want["status"], want["iterations"], want["restarts"], want["columns"]) == ("limit", 7, 1, 2)
    for every in (50, 1, 3):
        dx, = up(torch, cuda, conv["x0"])
        x, st = plan.solve(P.dval, db, x=dx, rtol=RTOL, max_iter=7, check_every=every)
        agrees(st, x, want)
        assert st["rnorm"] > RTOL * st["bnorm"]
    # max_iter == 0 with work to do: LIMIT at 0 and x untouched
    dx, = up(torch, cuda, conv["x0"])
    x, st = plan.solve(P.dval, db, x=dx, rtol=RTOL, max_iter=0)
    assert (st["status"], st["iterations"], st["restarts"], st["columns"]) == ("limit", 0, 0, 0) and same(x.cpu().numpy(), conv["x0"])
    agrees(st, x, composed_gmres(P.matvec, P.apply, P.dot, P.dots, conv["b"], conv["x0"], 5, RTOL, 0))
    plan.destroy()


def test_iterate_replays_in_a_graph(env, conv):
    """iterate(restart + 2) is a linear chain of launches; replayed, every pass but the first begins two columns into a
    cycle, so the chain's close and restart are met by a cycle that filled two steps earlier"""
    S, torch, cuda = env
    P = conv["P"]
    plan = P.plan(5)
    db, ex = up(torch, cuda, conv["b"], conv["x0"])
    _, est = plan.solve(P.dval, db, x=ex, rtol=RTOL, check_every=4)       # eager: the bits to meet; loads the code objects
    x, = up(torch, cuda, conv["x0"])
    plan.start(P.dval, db, x, rtol=RTOL)                                    # start runs eagerly
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            plan.iterate(5 + 2)
    st = plan.status()
    assert (st["status"], st["iterations"], st["columns"]) == ("running", 0, 0)   # capturing ran nothing
    for replay in range(1, 201):
        g.replay()
        st = plan.status()
        if st["status"] != "running":
            break
    print("GMRES(5) in a graph of 7 steps: %d replays for %d steps" % (replay, st["iterations"]))
    assert st == est, (st, est)
    assert same(x.cpu().numpy(), ex.cpu().numpy())
    assert replay <= -(-est["iterations"] // 5) + 1                          # every replay but the first finishes five columns
    plan.destroy()


def true_residual(n, rp, ci, val, b, x):
    return float(np.linalg.norm(b - KN.matvec(n, rp, ci, val, x)))


@pytest.mark.parametrize("restart,precond", [(30, None), (5, None), (30, "ilu0")])
def test_it_solves(env, conv, restart, precond):
    S, torch, cuda = env
    n, rp, ci, val, b, x0, P = (conv[k] for k in ("n", "rp", "ci", "val", "b", "x0", "P"))
    db, dx = up(torch, cuda, b, x0)
    x, st = S.gmres((n, P.drp, P.dci, P.dval), db, precond=precond, restart=restart, x=dx, rtol=RTOL)
    M = None
    if precond == "ilu0":
        lu = IN.ilu0_ref(n, rp, ci, val)
        rp64 = rp.astype(np.int64)

        def M(r):
            y, z = np.zeros(n), np.zeros(n)
            for i in range(n):
                c, v = ci[rp64[i]:rp64[i + 1]], lu[rp64[i]:rp64[i + 1]]
                y[i] = r[i] - np.dot(v[c < i], y[c[c < i]])
            for i in range(n - 1, -1, -1):
                c, v = ci[rp64[i]:rp64[i + 1]], lu[rp64[i]:rp64[i + 1]]
                z[i] = (y[i] - np.dot(v[c > i], z[c[c > i]])) / v[c == i][0]
            return z
    host_steps, host_restarts, host_x = GN.host_gmres(n, rp, ci, val, b, x0, restart, RTOL, precond=M)
    got, host = true_residual(n, rp, ci, val, b, x.cpu().numpy()), true_residual(n, rp, ci, val, b, host_x)
    bound = 2.0 * max(host, RTOL * np.linalg.norm(b))
    print("GMRES(%d) with %s: device %d steps and %d restarts, host GMRES %d and %d; true residual %.6e, the host's %.6e, bound %.6e"
          % (restart, precond, st["iterations"], st["restarts"], host_steps, host_restarts, got, host, bound))
    assert st["status"] == "converged"
    assert got <= bound


# ---------------------------------------------------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------------------------------------------------
def diagonal_system(env, d):
    S, torch, cuda = env
    n = len(d)
    return (n,) + tuple(up(torch, cuda, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.asarray(d, np.float64)))


def test_edges(env, conv):
    S, torch, cuda = env
    # n == 0
    x, st = S.gmres(diagonal_system(env, []), torch.empty(0, dtype=torch.float64, device=cuda))
    assert x.numel() == 0 and (st["status"], st["iterations"]) == ("converged", 0)
    # n == 1: the first step's w leaves nothing behind (eta == 0), the lucky breakdown, and that is convergence
    x, st = S.gmres(diagonal_system(env, [2.0]), up(torch, cuda, np.array([3.0]))[0])
    assert (st["status"], st["iterations"], st["rnorm"], st["eta"]) == ("converged", 1, 0.0, 0.0) and x.cpu().numpy()[0] == 1.5, st
    # b == 0: x = 0 whatever the guess, at iteration 0, and nothing was divided
    n, P = conv["n"], conv["P"]
    A = (n, P.drp, P.dci, P.dval)
    x, st = S.gmres(A, torch.zeros(n, dtype=torch.float64, device=cuda), x=torch.full((n,), -7.0, dtype=torch.float64, device=cuda))
    assert (st["status"], st["iterations"], st["rnorm"], st["bnorm"], st["restarts"]) == ("converged", 0, 0.0, 0.0, 0), st
    assert bool((x == 0.0).all())
    # the guess is the solution: small integers, so b = A x is exact and r = 0; x is untouched
    xs = np.random.default_rng(5).integers(-8, 9, n).astype(np.float64)
    db, dx = up(torch, cuda, KN.matvec(n, conv["rp"], conv["ci"], conv["val"], xs), xs)
    for precond in (None, "jacobi", "ilu0"):
        x, st = S.gmres(A, db, x=dx, precond=precond)
        assert (st["status"], st["iterations"], st["rnorm"]) == ("converged", 0, 0.0) and same(x.cpu().numpy(), xs), (precond, st)


def test_a_nan_in_val_never_converges(env, conv):
    S, torch, cuda = env
    n, P = conv["n"], conv["P"]
    dval = P.dval.clone()
    dval[7] = float("nan")
    db, = up(torch, cuda, conv["b"])
    for precond in (None, "jacobi"):
        x, st = S.gmres((n, P.drp, P.dci, dval), db, precond=precond, restart=5, max_iter=20, check_every=20)
        assert st["status"] in ("breakdown", "limit") and st["iterations"] <= 20, st
    # a NaN that arrives later: a clean start, then val changes under the solve's feet between two batches
    plan = P.plan(5)
    val = P.dval.clone()
    x = torch.zeros(n, dtype=torch.float64, device=cuda)
    plan.start(val, db, x, rtol=RTOL, max_iter=40)
    plan.iterate(3)
    assert plan.status()["status"] == "running"
    val[7] = float("nan")
    plan.iterate(40)
    st = plan.status()
    assert st["status"] in ("breakdown", "limit") and st["iterations"] <= 40, st
    plan.destroy()


def test_a_singular_system_never_converges(env):
    S, torch, cuda = env
    # diag(1, 0, 1, 0) x = 1, every operation exact: v_0 = 1/2, the first column is fine (h = eta = 1/2), the second
    # finds w = 0 and rotates h = (1/2, 1/2) to (., 0): d = 0, a breakdown that keeps the first column
    x, st = S.gmres(diagonal_system(env, [1.0, 0.0, 1.0, 0.0]), torch.ones(4, dtype=torch.float64, device=cuda), max_iter=50, check_every=50)
    assert st["status"] in ("breakdown", "limit") and 0 <= st["iterations"] <= 50, st
    assert (st["status"], st["breakdown"], st["iterations"], st["columns"]) == ("breakdown", "givens", 1, 1), st
    assert bool(torch.isfinite(x).all())
    # a zero row in a grid matrix, b not in the range: whatever it ends as, it is not CONVERGED
    n, rp, ci, val = KN.convection_diffusion(8)
    val = val.copy()
    val[rp[11]:rp[12]] = 0.0
    b = np.random.default_rng(30).standard_normal(n)
    drp, dci, dval, db = up(torch, cuda, rp, ci, val, b)
    for restart in (4, 30):
        x, st = S.gmres((n, drp, dci, dval), db, restart=restart, rtol=RTOL, max_iter=120, check_every=32)
        assert st["status"] in ("breakdown", "limit") and 0 <= st["iterations"] <= 120, st


def test_refusals_launch_nothing(env, conv):
    S, torch, cuda = env
    E = S.SblasError
    n, rp, ci, val = (conv[k] for k in ("n", "rp", "ci", "val"))
    P = Parts(env, n, rp, ci, val, "ilu0")
    db, = up(torch, cuda, conv["b"])
    x = torch.full((n,), -7.0, dtype=torch.float64, device=cuda)
    plan = P.plan(5)
    lower, upper = P.ilu.solvers()
    other_rp = P.drp.clone()
    foreign = S.Ilu0Plan(n, other_rp, P.dci)
    bad = [lambda: plan.solve(P.dval, db.cpu(), x=x, lu=P.lu), lambda: plan.solve(P.dval, db, x=x.cpu(), lu=P.lu),
           lambda: plan.solve(P.dval.cpu(), db, x=x, lu=P.lu), lambda: plan.solve(P.dval, db.float(), x=x, lu=P.lu),
           lambda: plan.solve(P.dval, db[:-1], x=x, lu=P.lu), lambda: plan.solve(P.dval[:-1], db, x=x, lu=P.lu),
           lambda: plan.solve(P.dval, db, x=x, lu=P.lu[:-1]), lambda: plan.solve(P.dval, db, x=x),       # a missing lu
           lambda: plan.solve(P.dval, x, x=x, lu=P.lu), lambda: plan.solve(P.dval, x[:], x=x, lu=P.lu),  # x is b
           lambda: plan.solve(P.dval, db, x=x, lu=P.lu, rtol=-1.0), lambda: plan.solve(P.dval, db, x=x, lu=P.lu, rtol=float("nan")),
           lambda: plan.solve(P.dval, db, x=x, lu=P.lu, atol=-1.0), lambda: plan.solve(P.dval, db, x=x, lu=P.lu, atol=float("nan")),
           lambda: plan.solve(P.dval, db, x=x, lu=P.lu, max_iter=-1), lambda: plan.solve(P.dval, db, x=x, lu=P.lu, check_every=0),
           lambda: S.GmresPlan(n, other_rp, P.dci, precond=P.ilu),              # the solves were planned on another rowptr
           lambda: S.GmresPlan(n, P.drp, P.dci, precond=foreign),
           lambda: S.GmresPlan(n, other_rp, P.dci, spmv_plan=P.spmv),           # a foreign SpMV plan
           lambda: S.GmresPlan(n, P.drp, P.dci, precond=(upper, lower)),        # swapped
           lambda: S.GmresPlan(n, P.drp, P.dci, precond=(lower, lower)),
           lambda: S.GmresPlan(n, P.drp, P.dci, precond="ssor"), lambda: S.GmresPlan(n, P.drp, P.dci, restart=0),
           lambda: S.GmresPlan(n, P.drp, P.dci, restart=65),
           lambda: S.GmresPlan(n + 1, P.drp, P.dci), lambda: S.GmresPlan(n, P.drp.long(), P.dci),
           lambda: S.GmresPlan(n, P.drp, P.dci, precond="jacobi").solve(P.dval, db, x=x),                # a missing dinv
           lambda: S.gmres((n, P.drp, P.dci, P.dval), db, precond="ssor", x=x)]
    for k, call in enumerate(bad):
        with pytest.raises(E):
            call()
            pytest.fail("call %d was accepted" % k)
    fresh = P.plan(5)
    with pytest.raises(E):
        fresh.iterate(1)                                                     # before start
    with pytest.raises(E):
        fresh.status()
    L = S.lib()
    assert L.sblas_hip_gmres_start(None, None, P.dval.data_ptr(), P.lu.data_ptr(), db.data_ptr(), x.data_ptr(), 1e-8, 0.0, 10) == 1
    assert L.sblas_hip_gmres_start(fresh.handle, None, P.dval.data_ptr(), None, db.data_ptr(), x.data_ptr(), 1e-8, 0.0, 10) == 1
    assert L.sblas_hip_gmres_start(fresh.handle, None, P.dval.data_ptr(), P.lu.data_ptr(), None, x.data_ptr(), 1e-8, 0.0, 10) == 1
    assert L.sblas_hip_gmres_start(fresh.handle, None, P.dval.data_ptr(), P.lu.data_ptr(), db.data_ptr(), x.data_ptr(), float("nan"), 0.0, 10) == 1
    import ctypes as C
    h = C.c_void_p()
    create = lambda restart, pre, lo, hi: L.sblas_hip_gmres_plan_create(-1, None, n, P.dval.numel(), P.drp.data_ptr(), P.dci.data_ptr(), restart,
                                                                        None, pre, lo, hi, C.byref(h))
    assert create(0, 0, None, None) == 1 and create(65, 0, None, None) == 1 and create(5, 3, None, None) == 1
    assert create(5, 2, lower.handle, None) == 1 and create(5, 0, lower.handle, upper.handle) == 1 and not h.value
    torch.cuda.synchronize()
    assert bool((x == -7.0).all())                                           # nothing ran
    both = S.GmresPlan(n, P.drp, P.dci, restart=5, precond=(lower, upper))
    assert both.info()["precond"] == "ilu0"
    plan.destroy(), fresh.destroy(), both.destroy(), foreign.destroy(), P.destroy()
