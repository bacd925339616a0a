"""Smoothed aggregation on the device (amg.hip): the hierarchy with P and R, the coarsening guard, the transfer
and prolongator-values kernels alone, apply eager and replayed from a graph, plain plans through the new create, the plan
inside PCG, BiCGStab and GMRES against loops composed from parts, check() and the refusals.  Every comparison of values is
==, against the numpy restatements of amg_sa_numerics."""
import ctypes
import math

import numpy as np
import pytest

import amg_numerics as AN
import amg_sa_numerics as SA
import krylov_numerics as KN
import solver_compose as SC

pytestmark = pytest.mark.gpu

RTOL = 1e-10
CONFIGS = (dict(), dict(smoother="l1", nu=2, coarse_sweeps=3, coarse_scale=1.5))


@pytest.fixture(scope="module")
def env(sblas, cuda):
    import torch
    return sblas, torch, cuda


def up(torch, cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def same(a, b):
    return KN.same_bits(a, b)


def host(t):
    return t.cpu().numpy() if t is not None else np.zeros(0)


class Built:
    """one case on the device: the smoothed plan after setup(val) with the defaults, and the restated hierarchy"""

    def __init__(self, env, name):
        S, torch, cuda = env
        self.c, self.host = SA.built(name, S.amg_aggregate)
        c = self.c
        self.n = c["n"]
        self.drp, self.dci, self.dval = up(torch, cuda, c["rp"], c["ci"], c["val"])
        self.plan = S.AmgPlan(self.n, self.drp, self.dci, val=self.dval if c["theta"] > 0.0 else None, theta=c["theta"], prolongator="smoothed")
        self.plan.setup(self.dval)


@pytest.fixture(scope="module")
def built(env):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Built(env, name)
        return made[name]
    yield get
    for b in made.values():
        b.plan.destroy()


def with_smoother(H, kw):
    return [dict(L, wd=AN.weights(L["n"], L["rowptr"], L["colidx"], L["val"], kw.get("smoother", "jacobi"))) for L in H]


def cycle(H, r, kw):
    if not H:
        return np.zeros(0)
    return SA.cycle_py(with_smoother(H, kw), r, kw.get("nu", 1), kw.get("coarse_sweeps", 8), kw.get("coarse_scale", 1.0))


def assert_levels(plan, want, what):
    info = plan.info()
    assert plan.levels() == [(L["n"], len(L["colidx"])) for L in want], what
    assert info["levels"] == len(want) and info["launches"] == AN.launches(len(want)) and info["ready"]
    assert info["entries"] == sum(len(L["colidx"]) for L in want)
    for l, W in enumerate(want):
        L = plan.level(l)
        assert np.array_equal(host(L["rowptr"]), W["rowptr"]) and np.array_equal(host(L["colidx"]), W["colidx"]), (what, l)
        assert same(host(L["val"]), W["val"]) and same(host(L["wd"]), W["wd"]), (what, l)
        if l + 1 < len(want):
            for key in ("agg", "aggptr", "members"):
                assert np.array_equal(host(L[key]), W[key]), (what, l, key)
            T = plan.transfer(l)
            assert (T["n"], T["n_coarse"], T["nnz"]) == (W["n"], len(W["aggptr"]) - 1, len(W["p_colidx"])), (what, l)
            for key in ("p_rowptr", "p_colidx", "r_rowptr", "r_colidx"):
                assert np.array_equal(host(T[key]), W[key]), (what, l, key)
            assert same(host(T["p_val"]), W["p_val"]) and same(host(T["r_val"]), W["r_val"]), (what, l)
        else:
            assert L["agg"] is None and L["n_coarse"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# the hierarchy and the guard
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SA.CASES)
def test_the_hierarchy_equals_the_restatement(env, built, name):
    S, torch, cuda = env
    B = built(name)
    info = B.plan.info()
    print("%s: levels %s, operator complexity %.3f, %d launches a cycle, %d bytes" % (name, B.plan.levels(), info["operator_complexity"],
                                                                                         info["launches"], info["bytes"]))
    assert (info["prolongator"], info["prolong_omega"], info["min_reduction"]) == ("smoothed", 2.0 / 3.0, 0.2)
    assert_levels(B.plan, B.host, name)
    assert B.plan.check() is None
    if B.n:                                                                    # other values: the aggregates and every pattern stay
        values = B.c["val"] * (1.0 + 0.25 * np.sin(np.arange(len(B.c["val"]))))
        dval, = up(torch, cuda, values)
        B.plan.setup(dval)
        assert_levels(B.plan, SA.hierarchy(dict(B.c, val=values), SA.fixed(B.host)), name)
        B.plan.setup(B.dval)
        torch.cuda.synchronize()


def test_the_guard_stops_a_hierarchy_that_barely_coarsens(env):
    S, torch, cuda = env
    c = SA.case("star5000")
    drp, dci, dval = up(torch, cuda, c["rp"], c["ci"], c["val"])
    for kind in ("plain", "smoothed"):
        plan = S.AmgPlan(c["n"], drp, dci, prolongator=kind, min_reduction=0.2)
        assert plan.levels() == [(5000, len(c["ci"]))] and plan.info()["min_reduction"] == 0.2
        plan.setup(dval)
        r = np.random.default_rng(5).standard_normal(c["n"])
        H = SA.hierarchy(c, S.amg_aggregate, kind, min_reduction=0.2)
        assert len(H) == 1 and same(host(plan.apply(up(torch, cuda, r)[0])), AN.cycle_py(H, r))
        plan.destroy()
    plan = S.AmgPlan(c["n"], drp, dci)                                       # plain, unguarded: as before
    assert plan.info()["levels"] == 20 and plan.info()["min_reduction"] == 0.0 and plan.info()["prolongator"] == "plain"
    assert [n for n, _ in plan.levels()] == list(range(5000, 4980, -1))
    plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# the kernels alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SA.CASES)
def test_single_kernels_have_the_restatements_bits(env, built, name):
    S, torch, cuda = env
    B = built(name)
    rng = np.random.default_rng(11)
    for l, H in list(enumerate(B.host))[:3]:
        n, nnz = H["n"], len(H["colidx"])
        values = H["val"] * (1.0 + 0.125 * np.cos(np.arange(nnz)))
        want_t = SA.tentative_values(n, H["rowptr"], H["colidx"], values)
        for offset in (0, 1):                                                # alignment must not reach the bits
            vbuf, tbuf = torch.zeros(nnz + 1, dtype=torch.float64, device=cuda), torch.full((nnz + 1,), -7.0, dtype=torch.float64, device=cuda)
            vbuf[offset:offset + nnz].copy_(up(torch, cuda, values)[0])
            S.amg_pvalues(B.plan, l, vbuf[offset:offset + nnz], tbuf[offset:offset + nnz])
            assert same(host(tbuf[offset:offset + nnz]), want_t), (name, l, offset)
            assert float(tbuf[nnz if offset == 0 else 0]) == -7.0
            if l + 1 == len(B.host):
                continue
            nc = len(H["aggptr"]) - 1
            res, e, x = rng.standard_normal(n), rng.standard_normal(nc), rng.standard_normal(n)
            fine = [torch.full((n + 1,), -7.0, dtype=torch.float64, device=cuda) for _ in range(2)]
            coarse = [torch.full((nc + 1,), -7.0, dtype=torch.float64, device=cuda) for _ in range(2)]
            dres, dx = (t[offset:offset + n] for t in fine)
            dbc, de = (t[offset:offset + nc] for t in coarse)
            dres.copy_(up(torch, cuda, res)[0]), dx.copy_(up(torch, cuda, x)[0]), de.copy_(up(torch, cuda, e)[0])
            S.amg_restrict(B.plan, l, dres, dbc)
            assert same(host(dbc), SA.transfer(H["r_rowptr"], H["r_colidx"], H["r_val"], res)), (name, l, offset)
            S.amg_prolong(B.plan, l, de, dx, scale=1.5)
            assert same(host(dx), x + np.float64(1.5) * SA.transfer(H["p_rowptr"], H["p_colidx"], H["p_val"], e)), (name, l, offset)
            assert same(host(dres), res) and same(host(de), e)                  # read only
            for t in fine + coarse:                                           # nothing beside the operands is written
                assert float(t[-1 if offset == 0 else 0]) == -7.0


# ---------------------------------------------------------------------------------------------------------------------
# apply
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SA.CASES)
def test_apply_equals_the_cycle_restatement(env, built, name):
    S, torch, cuda = env
    B = built(name)
    r = np.random.default_rng(5).standard_normal(B.n)
    dr, = up(torch, cuda, r)
    for kw in CONFIGS:
        B.plan.setup(B.dval, **kw)
        z = B.plan.apply(dr)
        z2 = torch.full((B.n,), -7.0, dtype=torch.float64, device=cuda)
        assert B.plan.apply(dr, out=z2) is z2
        want = cycle(B.host, r, kw)
        assert same(host(z), want) and same(host(z2), want), (name, kw)
        assert B.plan.info()["launches"] == AN.launches(len(B.host), kw.get("nu", 1), kw.get("coarse_sweeps", 8))
        assert same(host(dr), r)                                               # r is read only
        if B.n:                                                                # the C reference on the plan's own arrays agrees
            H = []
            for l in range(len(B.host)):
                L = {k: host(v) for k, v in B.plan.level(l).items() if hasattr(v, "cpu")}
                L["n"] = B.host[l]["n"]
                if l + 1 < len(B.host):
                    L.update({k: host(v) for k, v in B.plan.transfer(l).items() if hasattr(v, "cpu")})
                H.append(L)
            assert same(S.amg_cycle_sa_ref(H, r, nu=kw.get("nu", 1), coarse_sweeps=kw.get("coarse_sweeps", 8),
                                           coarse_scale=kw.get("coarse_scale", 1.0)), want)
    B.plan.setup(B.dval)


@pytest.mark.parametrize("name", ["grid32", "random600"])
def test_apply_replays_in_a_graph_after_a_new_setup(env, built, name):
    S, torch, cuda = env
    B = built(name)
    r = np.random.default_rng(6).standard_normal(B.n)
    dr, = up(torch, cuda, r)
    for kw in CONFIGS:
        dval = B.dval.clone()
        B.plan.setup(dval, **kw)
        z = torch.zeros(B.n, dtype=torch.float64, device=cuda)
        B.plan.apply(dr, out=z)                                              # eager first: loads the code objects
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                B.plan.apply(dr, out=z, stream=s)
        values = B.c["val"] * (1.0 + 0.1 * np.cos(np.arange(len(B.c["val"]))))
        dval.copy_(up(torch, cuda, values)[0])
        B.plan.setup(dval, **kw)                                             # the same pointer, new values: every level follows
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = host(z).copy()
        want = cycle(SA.hierarchy(dict(B.c, val=values), SA.fixed(B.host)), r, kw)
        assert same(got, want) and same(host(B.plan.apply(dr)), want), (name, kw)
    B.plan.setup(B.dval)
    assert same(host(B.plan.apply(dr)), cycle(B.host, r, {}))


# ---------------------------------------------------------------------------------------------------------------------
# plain plans through the new create
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grid24", "aniso32", "clique130", "random600"])
def test_a_plain_plan_through_create_ex_is_the_old_creates(env, name):
    S, torch, cuda = env
    c = SA.case(name)
    n = c["n"]
    drp, dci, dval = up(torch, cuda, c["rp"], c["ci"], c["val"])
    by_value = c["theta"] > 0.0
    old = S.AmgPlan(n, drp, dci, val=dval if by_value else None, theta=c["theta"])
    new = S.AmgPlan(n, drp, dci, val=dval if by_value else None, theta=c["theta"])
    S.lib().sblas_hip_amg_plan_destroy(new.handle)
    h, bad = ctypes.c_void_p(), ctypes.c_int64(-1)
    rc = S.lib().sblas_hip_amg_plan_create_ex(-1, None, n, len(c["ci"]), drp.data_ptr(), dci.data_ptr(), dval.data_ptr() if by_value else None,
                                              c["theta"], 64, 20, 0, 0, 0.0, 0.0, ctypes.byref(h), ctypes.byref(bad))
    assert rc == 0 and h.value
    new.handle = h
    r, = up(torch, cuda, np.random.default_rng(5).standard_normal(n))
    for kw in CONFIGS:
        old.setup(dval, **kw), new.setup(dval, **kw)
        a, b = old.info(), new.info()
        assert a == b and b["prolongator"] == "plain" and b["prolong_omega"] == 0.0
        for l in range(a["levels"]):
            A, Bl = old.level(l), new.level(l)
            for key in A:
                if hasattr(A[key], "cpu"):
                    assert same(host(A[key]), host(Bl[key])) if A[key].dtype == torch.float64 else np.array_equal(host(A[key]), host(Bl[key])), (l, key)
                else:
                    assert A[key] == Bl[key], (l, key)
        assert same(host(old.apply(r)), host(new.apply(r)))
    with pytest.raises(S.SblasError):
        new.transfer(0)                                                        # a plain plan has no transfer operators
    old.destroy(), new.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# in the solvers
# ---------------------------------------------------------------------------------------------------------------------
def Parts(env, n, rp, ci, val):
    return SC.Parts(env, n, rp, ci, val, "amg_smoothed", planned=False)


@pytest.fixture(scope="module")
def lap(env):
    n, rp, ci, val = KN.laplacian(32)
    P = Parts(env, n, rp, ci, val)
    yield dict(n=n, rp=rp, ci=ci, val=val, b=np.random.default_rng(30).standard_normal(n), P=P)
    P.amg.destroy()


@pytest.fixture(scope="module")
def conv(env):
    n, rp, ci, val = KN.convection_diffusion(24)
    P = Parts(env, n, rp, ci, val)
    yield dict(n=n, rp=rp, ci=ci, val=val, b=np.random.default_rng(30).standard_normal(n), P=P)
    P.amg.destroy()


@pytest.mark.parametrize("method", ["pcg", "bicgstab"])
def test_krylov_with_a_smoothed_plan_equals_its_composition(env, lap, conv, method):
    S, torch, cuda = env
    M = lap if method == "pcg" else conv
    n, b, P = M["n"], M["b"], M["P"]
    x0 = 0.1 * np.random.default_rng(31).standard_normal(n)
    loop = SC.composed_pcg if method == "pcg" else SC.composed_bicgstab
    want_x, want_it, want_rnorm, want_status = loop(P.matvec, P.apply, P.dot, b, x0, RTOL, 1000)
    plan = S.KrylovPlan(n, P.drp, P.dci, method=method, precond=P.amg)
    info = plan.info()
    db, = up(torch, cuda, b)
    runs = []
    for every in (1, 7, 50):
        dx, = up(torch, cuda, x0)
        x, st = plan.solve(P.dval, db, x=dx, rtol=RTOL, max_iter=1000, check_every=every)
        runs.append((x.cpu().numpy(), st))
    x, st = runs[0]
    print("%s with smoothed AMG: %d iterations, |r| = %.3e (composition: %d, %.3e); %d launches an iteration"
          % (method, st["iterations"], st["rnorm"], want_it, want_rnorm, info["launches"]))
    assert want_status == "converged" and 0 < want_it < 200
    assert (st["status"], st["iterations"]) == (want_status, want_it), st
    assert same(st["rnorm"], want_rnorm) and same(st["bnorm"], math.sqrt(S.krylov_dot_ref(b, b))) and same(x, want_x)
    for x2, st2 in runs[1:]:
        assert st2 == st and same(x2, x)
    assert info["precond"] == "amg" and info["launches"] == S.krylov_launches(method, "amg", P.amg.info()["launches"])
    plan.destroy()


def test_gmres_with_a_smoothed_plan_equals_its_composition(env, conv):
    S, torch, cuda = env
    n, b, P = conv["n"], conv["b"], conv["P"]
    x0 = 0.1 * np.random.default_rng(31).standard_normal(n)
    for restart in (30, 5):                                                 # 5: closes and restarts with a cycle in them
        want = SC.composed_gmres(P.matvec, P.apply, P.dot, P.dots, b, x0, restart, RTOL, 1000)
        plan = S.GmresPlan(n, P.drp, P.dci, restart=restart, precond=P.amg)
        info = plan.info()
        db, = up(torch, cuda, b)
        runs = []
        for every in (1, 7, 50):
            dx, = up(torch, cuda, x0)
            x, st = plan.solve(P.dval, db, x=dx, rtol=RTOL, max_iter=1000, check_every=every)
            runs.append((x.cpu().numpy(), st))
        x, st = runs[0]
        print("GMRES(%d) with smoothed AMG: %d steps, %d restarts, |r| = %.3e" % (restart, st["iterations"], st["restarts"], st["rnorm"]))
        assert want["status"] == "converged" and 0 < want["iterations"] < 200
        assert (st["status"], st["iterations"], st["restarts"], st["columns"], st["breakdown"]) == \
            (want["status"], want["iterations"], want["restarts"], want["columns"], want["breakdown"]), st
        assert same(st["rnorm"], want["rnorm"]) and same(st["bnorm"], want["bnorm"]) and same(x, want["x"])
        for x2, st2 in runs[1:]:
            assert st2 == st and same(x2, x)
        assert info["precond"] == "amg" and info["step_launches"] == S.gmres_launches(restart, "amg", P.amg.info()["launches"])["step"]
        plan.destroy()


def test_pcg_with_a_smoothed_plan_halves_the_plain_plans_count(env, lap):
    """Measured on an MI355X: DESIGN.md 3.25 records the counts this prints."""
    S, torch, cuda = env
    n, rp, ci, val, b, P = (lap[k] for k in ("n", "rp", "ci", "val", "b", "P"))
    db, = up(torch, cuda, b)
    x, st = S.pcg((n, P.drp, P.dci, P.dval), db, precond="amg_smoothed", rtol=RTOL)
    _, plain = S.pcg((n, P.drp, P.dci, P.dval), db, precond="amg", rtol=RTOL)
    H = SA.built("grid32", S.amg_aggregate)[1]
    host_it, host_x = AN.host_pcg(n, rp, ci, val, b, lambda r: S.amg_cycle_sa_ref(H, r), RTOL)
    residual = lambda v: float(np.linalg.norm(b - KN.matvec(n, rp, ci, val, v)))
    print("PCG with smoothed AMG: device %d iterations, host loop %d, the plain plan %d; true residual %.6e, the host loop's %.6e"
          % (st["iterations"], host_it, plain["iterations"], residual(x.cpu().numpy()), residual(host_x)))
    assert st["status"] == plain["status"] == "converged"
    assert st["iterations"] == host_it
    assert 2 * st["iterations"] <= plain["iterations"]


# ---------------------------------------------------------------------------------------------------------------------
# check() and the refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_check_names_the_level_and_row(env, built):
    S, torch, cuda = env
    B = built("grid24")
    assert B.plan.check() is None
    diag0 = np.flatnonzero(np.repeat(np.arange(B.n), np.diff(B.c["rp"])) == B.c["ci"])
    for what in (0.0, -4.0, float("nan")):
        val = B.c["val"].copy()
        val[diag0[200]] = what
        val[diag0[411]] = what
        B.plan.setup(up(torch, cuda, val)[0])
        assert B.plan.check() == (0, 200), what
    B.plan.setup(B.dval)
    assert B.plan.check() is None
    assert_levels(B.plan, B.host, "grid24 after a flagged setup")


def test_refusals_launch_nothing(env, lap):
    S, torch, cuda = env
    E = S.SblasError
    n, P = lap["n"], lap["P"]
    db, = up(torch, cuda, lap["b"])
    z = torch.full((n,), -7.0, dtype=torch.float64, device=cuda)
    fresh = S.AmgPlan(n, P.drp, P.dci, prolongator="smoothed")                # no setup yet
    last = P.amg.info()["levels"] - 1
    nc = P.amg.transfer(0)["n_coarse"]
    bad = [lambda: S.AmgPlan(n, P.drp, P.dci, prolongator="energy"), lambda: S.AmgPlan(n, P.drp, P.dci, prolongator="smoothed", prolong_omega=0.0),
           lambda: S.AmgPlan(n, P.drp, P.dci, prolongator="smoothed", prolong_omega=-1.0),
           lambda: S.AmgPlan(n, P.drp, P.dci, prolongator="smoothed", prolong_omega=float("nan")),
           lambda: S.AmgPlan(n, P.drp, P.dci, prolongator="smoothed", prolong_omega=float("inf")),
           lambda: S.AmgPlan(n, P.drp, P.dci, prolongator="smoothed", min_reduction=1.0), lambda: S.AmgPlan(n, P.drp, P.dci, min_reduction=-0.1),
           lambda: S.AmgPlan(n, P.drp, P.dci, min_reduction=float("nan")),
           lambda: P.amg.transfer(last), lambda: P.amg.transfer(-1),
           lambda: fresh.apply(db, out=z), lambda: S.amg_restrict(fresh, 0, db, z[:nc]),   # before setup: R has no values
           lambda: S.amg_prolong(fresh, 0, z[:nc], z), lambda: S.amg_restrict(P.amg, last, db, z),
           lambda: S.amg_pvalues(P.amg, 0, P.dval, P.dval), lambda: S.amg_pvalues(P.amg, 99, P.dval, P.dval.clone()),
           lambda: S.pcg((n, P.drp, P.dci, P.dval), db, precond="amg_energy", x=z)]
    for k, call in enumerate(bad):
        with pytest.raises(E):
            call()
            pytest.fail("call %d was accepted" % k)
    L = S.lib()
    h, row = ctypes.c_void_p(), ctypes.c_int64(-1)
    create = lambda kind, w, m: L.sblas_hip_amg_plan_create_ex(-1, None, n, len(P.dci), P.drp.data_ptr(), P.dci.data_ptr(), None, 0.0, 0, 0, 0,
                                                               kind, w, m, ctypes.byref(h), ctypes.byref(row))
    for args in ((2, 2.0 / 3.0, 0.2), (-1, 2.0 / 3.0, 0.2), (1, 0.0, 0.2), (1, float("nan"), 0.2), (1, float("inf"), 0.2), (1, 2.0 / 3.0, 1.0),
                 (1, 2.0 / 3.0, float("nan")), (0, 0.0, -0.5)):
        assert create(*args) != 0 and not h.value, args
    sizes, ptrs = (ctypes.c_int64 * 3)(), (ctypes.c_void_p * 6)()
    plain = S.AmgPlan(n, P.drp, P.dci)
    assert L.sblas_hip_amg_plan_transfer(plain.handle, 0, sizes, ptrs) != 0
    assert L.sblas_hip_amg_pvalues_f64(plain.handle, None, 0, P.dval.data_ptr(), z.data_ptr()) != 0
    torch.cuda.synchronize()
    assert bool((z == -7.0).all())                                           # nothing ran
    fresh.destroy(), plain.destroy()
