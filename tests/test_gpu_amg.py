"""The aggregation AMG plan on the device (amg.hip): the single kernels, the hierarchy, apply and check against the host
reference, the plan inside PCG, BiCGStab and GMRES against loops composed from parts, the iteration counts and the
refusals.  Every comparison of values is ==."""
import ctypes
import math

import numpy as np
import pytest

import amg_numerics as AN
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


class Built:
    """one case on the device: the plan after setup(val) with the defaults, and the host hierarchy of the same rule"""

    def __init__(self, env, name):
        S, torch, cuda = env
        self.c = c = AN.case(name)
        self.n = c["n"]
        self.drp, self.dci, self.dval = up(torch, cuda, c["rp"], c["ci"], c["val"])
        self.plan = S.AmgPlan(self.n, self.drp, self.dci, val=self.dval if c["theta"] > 0.0 else None, theta=c["theta"])
        self.plan.setup(self.dval)
        self.host = AN.hierarchy(c, S.amg_aggregate)


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


def fixed_aggregates(host, n, rp, ci, val, theta, seed, level):
    """the aggregates the hierarchy was made with (a level that was discarded reduces nothing: singletons)"""
    if "agg" in host[level]:
        return host[level]["agg"], host[level]["aggptr"], host[level]["members"]
    return np.arange(n, dtype=np.int32), np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)


def download(plan):
    """the plan's hierarchy as the host reference takes it"""
    out = []
    for l in range(plan.info()["levels"]):
        L = plan.level(l)
        out.append({k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in L.items() if v is not None})
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the hierarchy
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", AN.CASES)
def test_the_hierarchy_equals_the_hosts(env, built, name):
    S, torch, cuda = env
    B = built(name)
    plan, host = B.plan, B.host
    info = plan.info()
    assert plan.levels() == [(L["n"], len(L["colidx"])) for L in host]
    assert info["levels"] == len(host) and info["launches"] == S.amg_launches(len(host)) == AN.launches(len(host)) and info["ready"]
    print("%s: levels %s, operator complexity %.3f, %d launches a cycle, %d bytes" % (name, plan.levels(), info["operator_complexity"],
                                                                                         info["launches"], info["bytes"]))
    for values in (B.c["val"], B.c["val"] * (1.0 + 0.25 * np.sin(np.arange(len(B.c["val"]))))):
        dval, = up(torch, cuda, values)
        plan.setup(dval)
        want = AN.hierarchy(dict(B.c, val=values), lambda *a: fixed_aggregates(host, *a))
        above = None
        for l, (H, W) in enumerate(zip(host, want)):
            L = plan.level(l)
            assert np.array_equal(L["rowptr"].cpu().numpy(), H["rowptr"]) and np.array_equal(L["colidx"].cpu().numpy(), H["colidx"])
            assert same(L["val"].cpu().numpy(), W["val"]) and same(L["wd"].cpu().numpy(), W["wd"])
            if l > 0:                                                          # CooPlan.assemble of the level above
                assert same(L["val"].cpu().numpy(), above.cpu().numpy())
            if l + 1 < len(host):
                for key in ("agg", "aggptr", "members"):
                    assert np.array_equal(L[key].cpu().numpy(), H[key]), (name, l, key)
                row = np.repeat(np.arange(H["n"]), np.diff(H["rowptr"]))
                coo = S.CooPlan(len(H["aggptr"]) - 1, len(H["aggptr"]) - 1, *up(torch, cuda, H["agg"][row], H["agg"][H["colidx"]]), dup="sum")
                above = coo.assemble(L["val"])
                torch.cuda.synchronize()
                coo.destroy()
            else:
                assert L["agg"] is None and L["n_coarse"] == 0
        assert plan.check() is None
    plan.setup(B.dval)


# ---------------------------------------------------------------------------------------------------------------------
# the single kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", AN.CASES)
def test_single_kernels_have_the_restatements_bits(env, built, name):
    S, torch, cuda = env
    B = built(name)
    rng = np.random.default_rng(11)
    for l, H in list(enumerate(B.host))[:3]:
        n = H["n"]
        b, x = rng.standard_normal(n), rng.standard_normal(n)
        s = AN.row_sums(H, x)
        want = {"sweep": x + H["wd"] * (b - s), "residual": b - s, "first": H["wd"] * b}
        for offset in (0, 1):                                                # alignment must not reach the bits
            buf = [torch.zeros(n + 1, dtype=torch.float64, device=cuda) for _ in range(3)]
            db, dx, dy = (t[offset:offset + n] for t in buf)
            db.copy_(up(torch, cuda, b)[0]), dx.copy_(up(torch, cuda, x)[0])
            for mode in ("sweep", "residual", "first"):
                dy.fill_(-7.0)
                S.amg_sweep(B.plan, l, db, dx, dy, mode=mode)
                assert same(dy.cpu().numpy(), want[mode]), (name, l, mode, offset)
            # x and y swapped back and forth: three sweeps
            S.amg_sweep(B.plan, l, db, dx, dy), S.amg_sweep(B.plan, l, db, dy, dx), S.amg_sweep(B.plan, l, db, dx, dy)
            x1 = want["sweep"]
            x2 = x1 + H["wd"] * (b - AN.row_sums(H, x1))
            x3 = x2 + H["wd"] * (b - AN.row_sums(H, x2))
            assert same(dx.cpu().numpy(), x2) and same(dy.cpu().numpy(), x3)
            if l + 1 < len(B.host):
                nc = len(H["aggptr"]) - 1
                bc = np.zeros(nc)
                for a in range(nc):
                    t = 0.0
                    for k in range(H["aggptr"][a], H["aggptr"][a + 1]):
                        t = t + float(b[H["members"][k]])
                    bc[a] = t
                cbuf = torch.full((nc + 1,), -7.0, dtype=torch.float64, device=cuda)
                db.copy_(up(torch, cuda, b)[0])
                S.amg_restrict(B.plan, l, db, cbuf[offset:offset + nc])
                assert same(cbuf[offset:offset + nc].cpu().numpy(), bc)
                dx.copy_(up(torch, cuda, x)[0])
                S.amg_prolong(B.plan, l, cbuf[offset:offset + nc], dx, scale=1.5)
                assert same(dx.cpu().numpy(), x + np.float64(1.5) * bc[H["agg"]])


# ---------------------------------------------------------------------------------------------------------------------
# apply
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", AN.CASES)
def test_apply_equals_the_cycle_reference(env, built, name):
    S, torch, cuda = env
    B = built(name)
    r = np.random.default_rng(5).standard_normal(B.n)
    dr, = up(torch, cuda, r)
    for kw in (dict(), dict(smoother="l1", nu=2, coarse_sweeps=3, coarse_scale=1.5)):
        B.plan.setup(B.dval, **kw)
        z = B.plan.apply(dr)
        z2 = torch.full((B.n,), -7.0, dtype=torch.float64, device=cuda)
        assert B.plan.apply(dr, out=z2) is z2
        H = download(B.plan)
        want = S.amg_cycle_ref(H, r, nu=kw.get("nu", 1), coarse_sweeps=kw.get("coarse_sweeps", 8), coarse_scale=kw.get("coarse_scale", 1.0))
        assert same(z.cpu().numpy(), want) and same(z2.cpu().numpy(), want), (name, kw)
        assert B.plan.info()["launches"] == AN.launches(len(H), kw.get("nu", 1), kw.get("coarse_sweeps", 8))
        assert same(dr.cpu().numpy(), r)                                       # r is read only
    B.plan.setup(B.dval)


def test_apply_replays_in_a_graph_after_a_new_setup(env, built):
    S, torch, cuda = env
    B = built("grid32")
    r = np.random.default_rng(6).standard_normal(B.n)
    dr, = up(torch, cuda, r)
    dval = B.dval.clone()
    B.plan.setup(dval)
    z = torch.zeros(B.n, dtype=torch.float64, device=cuda)
    B.plan.apply(dr, out=z)                                                  # eager first: loads the code objects
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            B.plan.apply(dr, out=z, stream=s)
    dval.mul_(1.0 + 0.1 * torch.cos(torch.arange(len(dval), device=cuda, dtype=torch.float64)))
    B.plan.setup(dval)                                                       # the same pointer, new values: every level follows
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    got = z.cpu().numpy().copy()
    eager = B.plan.apply(dr).cpu().numpy()
    assert same(got, eager) and same(eager, S.amg_cycle_ref(download(B.plan), r))
    B.plan.setup(B.dval)
    assert same(B.plan.apply(dr).cpu().numpy(), S.amg_cycle_ref(B.host, r))


def test_check_names_the_level_and_row(env, built):
    S, torch, cuda = env
    B = built("grid24")
    H = B.host
    assert B.plan.check() is None
    diag0 = np.flatnonzero(np.repeat(np.arange(B.n), np.diff(B.c["rp"])) == B.c["ci"])
    for what in (0.0, float("nan")):
        val = B.c["val"].copy()
        val[diag0[200]] = what
        val[diag0[411]] = what
        B.plan.setup(up(torch, cuda, val)[0])
        assert B.plan.check() == (0, 200), what
    # a coarse diagonal that sums to exactly zero while every fine one stays positive: the two entries that join two
    # members of aggregate 3 take half of what its coarse diagonal sums to each (small integers: every sum is exact)
    val = B.c["val"].copy()
    rp, ci = B.c["rp"], B.c["ci"]
    members = H[0]["members"][H[0]["aggptr"][3]:H[0]["aggptr"][4]]
    u, v = next((u, v) for u in members for v in members if u < v and v in ci[rp[u]:rp[u + 1]])
    d1 = np.flatnonzero(np.repeat(np.arange(H[1]["n"]), np.diff(H[1]["rowptr"])) == H[1]["colidx"])
    clean = AN.assemble(val, H[0]["perm"], H[0]["runptr"])[d1[3]]
    assert clean > 0.0 and clean % 2.0 == 0.0
    for a, b in ((u, v), (v, u)):
        val[rp[a] + int(np.flatnonzero(ci[rp[a]:rp[a + 1]] == b)[0])] -= clean / 2.0
    assert AN.assemble(val, H[0]["perm"], H[0]["runptr"])[d1[3]] == 0.0
    B.plan.setup(up(torch, cuda, val)[0])
    assert B.plan.check() == (1, 3)
    B.plan.setup(B.dval)
    assert B.plan.check() is None


# ---------------------------------------------------------------------------------------------------------------------
# in the solvers
# ---------------------------------------------------------------------------------------------------------------------
def Parts(env, n, rp, ci, val):
    return SC.Parts(env, n, rp, ci, val, "amg", planned=False)


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
def test_krylov_with_amg_equals_its_composition(env, lap, conv, method):
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
    print("%s with AMG: %d iterations, |r| = %.3e (composition: %d, %.3e); %d launches an iteration"
          % (method, st["iterations"], st["rnorm"], want_it, want_rnorm, info["launches"]))
    assert want_status == "converged" and 0 < want_it < 200
    assert (st["status"], st["iterations"]) == (want_status, want_it), st
    assert same(st["rnorm"], want_rnorm) and same(st["bnorm"], math.sqrt(S.krylov_dot_ref(b, b))) and same(x, want_x)
    for x2, st2 in runs[1:]:
        assert st2 == st and same(x2, x)
    lim = S.krylov_limits()
    assert info["precond"] == "amg" and info["vectors"] == (lim["pcg_vectors"] if method == "pcg" else lim["bicgstab_vectors"]) + 1
    assert info["launches"] == S.krylov_launches(method, "amg", P.amg.info()["launches"])
    plan.destroy()


def test_gmres_with_amg_equals_its_composition(env, conv):
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
        print("GMRES(%d) with AMG: %d steps, %d restarts, |r| = %.3e" % (restart, st["iterations"], st["restarts"], st["rnorm"]))
        assert want["status"] == "converged" and 0 < want["iterations"] < 200
        assert (st["status"], st["iterations"], st["restarts"], st["columns"], st["breakdown"]) == \
            (want["status"], want["iterations"], want["restarts"], want["columns"], want["breakdown"]), st
        assert same(st["rnorm"], want["rnorm"]) and same(st["bnorm"], want["bnorm"]) and same(x, want["x"])
        for x2, st2 in runs[1:]:
            assert st2 == st and same(x2, x)
        assert info["precond"] == "amg" and info["step_launches"] == S.gmres_launches(restart, "amg", P.amg.info()["launches"])["step"]
        plan.destroy()


def test_pcg_with_amg_halves_the_iterations(env, lap):
    """Measured on an MI355X: DESIGN.md 3.24 records the counts and residuals this prints."""
    S, torch, cuda = env
    n, rp, ci, val, b, P = (lap[k] for k in ("n", "rp", "ci", "val", "b", "P"))
    db, = up(torch, cuda, b)
    x, st = S.pcg((n, P.drp, P.dci, P.dval), db, precond="amg", rtol=RTOL)
    _, plain = S.pcg((n, P.drp, P.dci, P.dval), db, rtol=RTOL)
    H = AN.hierarchy(AN.case("grid32"), S.amg_aggregate)
    host_it, host_x = AN.host_pcg(n, rp, ci, val, b, lambda r: S.amg_cycle_ref(H, r), RTOL)
    residual = lambda v: float(np.linalg.norm(b - KN.matvec(n, rp, ci, val, v)))
    got, host = residual(x.cpu().numpy()), residual(host_x)
    bound = 2.0 * max(host, RTOL * np.linalg.norm(b))                        # the bound test_gpu_krylov.py uses for ILU(0)
    print("PCG with AMG: device %d iterations, host loop %d, plain CG on the device %d; true residual %.6e, the host loop's %.6e, "
          "bound %.6e" % (st["iterations"], host_it, plain["iterations"], got, host, bound))
    assert st["status"] == plain["status"] == "converged"
    assert st["iterations"] == host_it
    assert 2 * st["iterations"] <= plain["iterations"]
    assert got <= bound


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(env, lap):
    S, torch, cuda = env
    E = S.SblasError
    n, P = lap["n"], lap["P"]
    db, = up(torch, cuda, lap["b"])
    z = torch.full((n,), -7.0, dtype=torch.float64, device=cuda)
    other_rp = P.drp.clone()
    fresh = S.AmgPlan(n, P.drp, P.dci)                                       # no setup yet
    unsorted = P.dci.clone()
    unsorted[int(P.drp[5])], unsorted[int(P.drp[5]) + 1] = P.dci[int(P.drp[5]) + 1].item(), P.dci[int(P.drp[5])].item()
    bad = [lambda: fresh.apply(db, out=z),                                     # before setup
           lambda: S.amg_sweep(fresh, 0, db, db.clone(), z),
           lambda: P.amg.apply(z, out=z),                                      # z is r
           lambda: P.amg.apply(db.cpu(), out=z), lambda: P.amg.apply(db, out=z[:-1]), lambda: P.amg.apply(db.float(), out=z),
           lambda: fresh.setup(P.dval, smoother="ssor"), lambda: fresh.setup(P.dval, omega=-1.0), lambda: fresh.setup(P.dval, nu=0),
           lambda: fresh.setup(P.dval, coarse_sweeps=0), lambda: fresh.setup(P.dval[:-1]), lambda: fresh.setup(P.dval, omega=float("nan")),
           lambda: S.AmgPlan(n, P.drp, P.dci, theta=0.25), lambda: S.AmgPlan(n, P.drp, P.dci, val=P.dval, theta=1.5),
           lambda: S.AmgPlan(n, P.drp, P.dci, val=P.dval, theta=float("nan")), lambda: S.AmgPlan(n + 1, P.drp, P.dci),
           lambda: S.AmgPlan(n, P.drp, P.dci, max_levels=0), lambda: S.AmgPlan(n, P.drp, P.dci, coarse_max=0),
           lambda: S.KrylovPlan(n, other_rp, P.dci, precond=P.amg),            # a plan of another structure
           lambda: S.GmresPlan(n, other_rp, P.dci, precond=P.amg),
           lambda: S.amg_sweep(P.amg, 0, db, z, z), lambda: S.amg_sweep(P.amg, 99, db, db.clone(), z),
           lambda: S.amg_sweep(P.amg, 0, db, db.clone(), z, mode="ssor"),
           lambda: S.amg_restrict(P.amg, P.amg.info()["levels"] - 1, db, z),
           lambda: S.pcg((n, P.drp, P.dci, P.dval), db, precond="ssor", x=z)]
    for k, call in enumerate(bad):
        with pytest.raises(E):
            call()
            pytest.fail("call %d was accepted" % k)
    with pytest.raises(E) as err:
        S.AmgPlan(n, P.drp, unsorted)
    assert err.value.bad_row == 5
    L = S.lib()
    dev = torch.cuda.current_device()
    assert L.sblas_hip_amg_plan_speaks_for(P.amg.handle, -1, n, len(P.dci), P.drp.data_ptr(), P.dci.data_ptr()) == 0
    assert L.sblas_hip_amg_plan_speaks_for(P.amg.handle, dev + 1, n, len(P.dci), P.drp.data_ptr(), P.dci.data_ptr()) != 0   # another device
    assert L.sblas_hip_amg_plan_speaks_for(P.amg.handle, -1, n, len(P.dci), other_rp.data_ptr(), P.dci.data_ptr()) != 0
    h = ctypes.c_void_p()
    assert L.sblas_hip_krylov_plan_create(-1, None, 0, n, len(P.dci), P.drp.data_ptr(), P.dci.data_ptr(), None, 3, None, None,
                                          ctypes.byref(h)) != 0       # AMG without a handle stays refused
    assert L.sblas_hip_krylov_plan_create(-1, None, 0, n, len(P.dci), P.drp.data_ptr(), P.dci.data_ptr(), None, 3, P.amg.handle, P.amg.handle,
                                          ctypes.byref(h)) != 0       # upper_plan must be NULL
    assert L.sblas_hip_amg_plan_apply(P.amg.handle, None, db.data_ptr(), None) != 0
    torch.cuda.synchronize()
    assert bool((z == -7.0).all())                                           # nothing ran
    fresh.destroy()
