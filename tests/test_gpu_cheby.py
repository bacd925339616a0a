"""The Chebyshev plan on the device (cheby.hip): the estimate's scalars, lambda_max and the table against
the host reference, apply and smooth against the reference polynomial (eager, twice, offset operands, replayed from a graph
after a new setup), a caller's lambda_max, check(), the plan inside PCG, BiCGStab and GMRES against loops composed from
parts, the iteration count and the refusals.  Every comparison of values is ==."""
import ctypes
import math

import numpy as np
import pytest

import amg_numerics as AN
import cheby_numerics as CN
import krylov_numerics as KN
import solver_compose as SC

pytestmark = pytest.mark.gpu

RTOL = 1e-10
SHAPES = ["n1", "diagonal300", "tridiagonal3000", "grid24", "clique130", "star5000", "random4000", "aniso32"]


@pytest.fixture(scope="module")
def env(sblas, cuda):
    import torch
    return sblas, torch, cuda


def up(torch, cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def same(a, b):
    return KN.same_bits(a, b)


def host_estimate(S, c, seed=0, degree=4, steps=10, boost=1.1, ratio=30.0):
    """the whole setup by the host reference -> dict(alpha, beta, m, ritz, g, lambda_max, lambda_min, table)"""
    n, rp, ci, val = c["n"], c["rp"], c["ci"], c["val"]
    L = S.cheby_lanczos_ref(n, rp, ci, val, eig_steps=steps, seed=seed)
    ritz = S.cheby_ritz_ref(L["alpha"], L["beta"])["ritz"] if L["m"] else 0.0
    g = S.cheby_rowbound_ref(n, rp, ci, val)
    lam = S.cheby_lambda_ref(L["m"], ritz, g, boost)
    T = S.cheby_coef_ref(lam, degree=degree, eig_ratio=ratio)
    return dict(L, ritz=ritz, g=g, lambda_max=lam, lambda_min=T["lambda_min"], table=T["table"])


class Built:
    """one case on the device: the plan of degree 4 after setup(val), and the host's estimate of the same rule"""

    def __init__(self, env, name):
        S, torch, cuda = env
        self.c = c = CN.case(name)
        self.n = c["n"]
        self.drp, self.dci, self.dval = up(torch, cuda, c["rp"], c["ci"], c["val"])
        self.plan = S.ChebyshevPlan(self.n, self.drp, self.dci)
        self.plan.setup(self.dval)
        self.host = host_estimate(S, c)


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


def assert_setup_equals(plan, W, what):
    got, sc = plan.check(), plan.scalars()
    assert got["bad_row"] is None and got["m"] == W["m"], (what, got, W["m"])
    assert same(sc["alpha"], W["alpha"]) and same(sc["beta"], W["beta"]), what
    assert same(got["ritz"], W["ritz"]) and same(got["g"], W["g"]), (what, got)
    assert same(got["lambda_max"], W["lambda_max"]) and same(got["lambda_min"], W["lambda_min"]) and same(sc["table"], W["table"]), (what, got)


# ---------------------------------------------------------------------------------------------------------------------
# setup: the estimate
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_the_estimate_equals_the_hosts_at_two_seeds(env, built, name):
    S, torch, cuda = env
    B = built(name)
    assert_setup_equals(B.plan, B.host, name)
    info = B.plan.info()
    assert info["ready"] and info["launches"] == info["degree"] == 4 and info["setup_launches"] == 6 * 10 + 1
    print("%s: m %d, Ritz %.6g, g %.6g, lambda_max %.6g; %d units, %d bytes" % (name, B.host["m"], B.host["ritz"], B.host["g"],
                                                                                  B.host["lambda_max"], info["units"], info["bytes"]))
    other = S.ChebyshevPlan(B.n, B.drp, B.dci, degree=3, eig_steps=6, eig_boost=1.05, eig_ratio=20.0, seed=5)
    values = B.c["val"] * (1.0 + 0.25 * np.sin(np.arange(len(B.c["val"]))))   # other values too (no longer symmetric: the bits still agree)
    other.setup(up(torch, cuda, values)[0])
    assert_setup_equals(other, host_estimate(S, dict(B.c, val=values), seed=5, degree=3, steps=6, boost=1.05, ratio=20.0), name + " seed 5")
    other.setup(B.dval)                                                      # repeatable: a second setup, the first one's values again
    other.setup(up(torch, cuda, values)[0])
    assert_setup_equals(other, host_estimate(S, dict(B.c, val=values), seed=5, degree=3, steps=6, boost=1.05, ratio=20.0), name + " again")
    other.destroy()


def test_the_indefinite_case_freezes_where_the_host_stops(env):
    S, torch, cuda = env
    c = CN.case("indefinite2")
    drp, dci, dval = up(torch, cuda, c["rp"], c["ci"], c["val"])
    for seed in (0, 5, 9):
        plan = S.ChebyshevPlan(2, drp, dci, seed=seed)
        plan.setup(dval)
        W = host_estimate(S, c, seed=seed)
        assert W["m"] < 10
        assert_setup_equals(plan, W, seed)
        plan.destroy()


def test_a_given_lambda_max_gives_the_host_tables_bits(env, built):
    S, torch, cuda = env
    B = built("grid24")
    for lam in (2.0, 1.9544612, 7.25):
        B.plan.setup(B.dval, lambda_max=lam)
        got, sc = B.plan.check(), B.plan.scalars()
        W = S.cheby_coef_ref(lam, degree=4)
        assert same(sc["table"], W["table"]) and same(got["lambda_max"], lam) and same(got["lambda_min"], W["lambda_min"])
        assert got["m"] == 0 and got["ritz"] == 0.0 and same(got["g"], B.host["g"]) and got["bad_row"] is None
    B.plan.setup(B.dval)
    assert_setup_equals(B.plan, B.host, "the estimate again")


def test_check_names_a_planted_diagonal(env, built):
    S, torch, cuda = env
    B = built("grid24")
    diag = np.flatnonzero(np.repeat(np.arange(B.n), np.diff(B.c["rp"])) == B.c["ci"])
    for what in (0.0, -4.0, float("nan"), float("inf")):
        val = B.c["val"].copy()
        val[diag[200]] = what
        val[diag[411]] = what
        B.plan.setup(up(torch, cuda, val)[0])
        assert B.plan.check()["bad_row"] == 200, what
    B.plan.setup(B.dval)
    assert B.plan.check()["bad_row"] is None


# ---------------------------------------------------------------------------------------------------------------------
# apply and smooth
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_apply_and_smooth_equal_the_reference(env, built, name):
    S, torch, cuda = env
    B = built(name)
    n, rp, ci, val = B.n, B.c["rp"], B.c["ci"], B.c["val"]
    rng = np.random.default_rng(5)
    r, x = rng.standard_normal(n), rng.standard_normal(n)
    for degree in (4, 1, 2, 3):                                              # both parities of the ping-pong; 4 is the module's plan
        plan = B.plan if degree == 4 else S.ChebyshevPlan(n, B.drp, B.dci, degree=degree)
        if degree != 4:
            plan.setup(B.dval)
        table = plan.scalars()["table"]
        assert same(table, S.cheby_coef_ref(B.host["lambda_max"], degree=degree)["table"])
        want = S.cheby_apply_ref(n, rp, ci, val, table, r)
        want_s = S.cheby_apply_ref(n, rp, ci, val, table, r, x)
        for offset in (0, 1):                                                # alignment must not reach the bits
            buf = [torch.full((n + 1,), -7.0, dtype=torch.float64, device=cuda) for _ in range(3)]
            dr, dx, dz = (t[offset:offset + n] for t in buf)
            dr.copy_(up(torch, cuda, r)[0]), dx.copy_(up(torch, cuda, x)[0])
            assert plan.apply(dr, out=dz) is dz
            assert same(dz.cpu().numpy(), want), (name, degree, offset)
            plan.apply(dr, out=dz)                                           # twice: nothing is carried from one call to the next
            assert same(dz.cpu().numpy(), want), (name, degree, offset, "twice")
            dz.fill_(-7.0)
            assert plan.smooth(dr, dx, out=dz) is dz
            assert same(dz.cpu().numpy(), want_s), (name, degree, offset, "smooth")
            plan.smooth(dr, dx, out=dz)
            assert same(dz.cpu().numpy(), want_s), (name, degree, offset, "smooth twice")
            assert same(dr.cpu().numpy(), r) and same(dx.cpu().numpy(), x)   # the operands are read only
            assert all(float(t[n if offset == 0 else 0]) == -7.0 for t in buf)   # the element beside them is untouched
        if degree != 4:
            plan.destroy()
    assert same(B.plan.apply(up(torch, cuda, r)[0]).cpu().numpy(), S.cheby_apply_ref(n, rp, ci, val, B.host["table"], r))


def test_apply_and_smooth_replay_in_a_graph_after_a_new_setup(env, built):
    S, torch, cuda = env
    B = built("grid24")
    n, rp, ci = B.n, B.c["rp"], B.c["ci"]
    rng = np.random.default_rng(6)
    r, x = rng.standard_normal(n), rng.standard_normal(n)
    dr, dx = up(torch, cuda, r, x)
    dval = B.dval.clone()
    plan = S.ChebyshevPlan(n, B.drp, B.dci, degree=3)
    plan.setup(dval)
    z, y = torch.zeros(n, dtype=torch.float64, device=cuda), torch.zeros(n, dtype=torch.float64, device=cuda)
    plan.apply(dr, out=z), plan.smooth(dr, dx, out=y)                        # eager first: loads the code objects
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            plan.setup(dval, stream=s)                                       # setup is capturable too: the estimate is in the graph
            plan.apply(dr, out=z, stream=s)
            plan.smooth(dr, dx, out=y, stream=s)
    dval.mul_(1.0 + 0.1 * torch.cos(torch.arange(len(dval), device=cuda, dtype=torch.float64)))
    torch.cuda.synchronize()
    z.fill_(-7.0), y.fill_(-7.0)
    g.replay()
    torch.cuda.synchronize()
    values = dval.cpu().numpy()
    W = host_estimate(S, dict(B.c, val=values), degree=3)
    assert_setup_equals(plan, W, "replayed")
    assert same(z.cpu().numpy(), S.cheby_apply_ref(n, rp, ci, values, W["table"], r))
    assert same(y.cpu().numpy(), S.cheby_apply_ref(n, rp, ci, values, W["table"], r, x))
    plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# in the solvers
# ---------------------------------------------------------------------------------------------------------------------
class Parts(SC.Parts):
    """solver_compose's parts with M^-1 v by ChebyshevPlan.apply"""

    def __init__(self, env, n, rp, ci, val, degree=4):
        self.cheb, self.degree = None, degree
        super().__init__(env, n, rp, ci, val, None, planned=False)

    def revalue(self, val):
        super().revalue(val)
        if self.cheb is None:
            self.cheb = self.env[0].ChebyshevPlan(self.n, self.drp, self.dci, degree=self.degree)
        self.cheb.setup(self.dval)

    def handle(self):
        return self.cheb

    def apply(self, v):
        S, torch, cuda = self.env
        return self.cheb.apply(up(torch, cuda, v)[0]).cpu().numpy()

    def destroy(self):
        if self.cheb is not None:
            self.cheb.destroy()
        self.cheb = None
        super().destroy()


@pytest.fixture(scope="module")
def lap(env):
    n, rp, ci, val = KN.laplacian(24)
    P = Parts(env, n, rp, ci, val)
    yield dict(n=n, rp=rp, ci=ci, val=val, b=np.random.default_rng(30).standard_normal(n), P=P)
    P.destroy()


@pytest.fixture(scope="module")
def conv(env):
    n, rp, ci, val = KN.convection_diffusion(24)
    P = Parts(env, n, rp, ci, val)
    yield dict(n=n, rp=rp, ci=ci, val=val, b=np.random.default_rng(30).standard_normal(n), P=P)
    P.destroy()


@pytest.mark.parametrize("method", ["pcg", "bicgstab"])
def test_krylov_with_the_plan_equals_its_composition(env, lap, conv, method):
    S, torch, cuda = env
    M = lap if method == "pcg" else conv
    n, b, P = M["n"], M["b"], M["P"]
    x0 = 0.1 * np.random.default_rng(31).standard_normal(n)
    loop = SC.composed_pcg if method == "pcg" else SC.composed_bicgstab
    want_x, want_it, want_rnorm, want_status = loop(P.matvec, P.apply, P.dot, b, x0, RTOL, 1000)
    plan = S.KrylovPlan(n, P.drp, P.dci, method=method, precond=P.cheb)
    info = plan.info()
    db, = up(torch, cuda, b)
    runs = []
    for every in (1, 7, 50):
        dx, = up(torch, cuda, x0)
        x, st = plan.solve(P.dval, db, x=dx, rtol=RTOL, max_iter=1000, check_every=every)
        runs.append((x.cpu().numpy(), st))
    x, st = runs[0]
    print("%s with the polynomial: %d iterations, |r| = %.3e (composition: %d, %.3e); %d launches an iteration"
          % (method, st["iterations"], st["rnorm"], want_it, want_rnorm, info["launches"]))
    assert want_status == "converged" and 0 < want_it < 200
    assert (st["status"], st["iterations"]) == (want_status, want_it), st
    assert same(st["rnorm"], want_rnorm) and same(st["bnorm"], math.sqrt(S.krylov_dot_ref(b, b))) and same(x, want_x)
    for x2, st2 in runs[1:]:
        assert st2 == st and same(x2, x)
    lim = S.krylov_limits()
    assert info["precond"] == "chebyshev" and info["vectors"] == (lim["pcg_vectors"] if method == "pcg" else lim["bicgstab_vectors"]) + 1
    assert info["launches"] == S.krylov_launches(method, "chebyshev", 4) == (8 + 4 if method == "pcg" else 10 + 2 * 4)
    plan.destroy()


def test_gmres_with_the_plan_equals_its_composition(env, conv):
    S, torch, cuda = env
    n, b, P = conv["n"], conv["b"], conv["P"]
    x0 = 0.1 * np.random.default_rng(31).standard_normal(n)
    for restart in (30, 5):                                                 # 5: closes and restarts with a polynomial in them
        want = SC.composed_gmres(P.matvec, P.apply, P.dot, P.dots, b, x0, restart, RTOL, 1000)
        plan = S.GmresPlan(n, P.drp, P.dci, restart=restart, precond=P.cheb)
        info = plan.info()
        db, = up(torch, cuda, b)
        runs = []
        for every in (1, 7, 50):
            dx, = up(torch, cuda, x0)
            x, st = plan.solve(P.dval, db, x=dx, rtol=RTOL, max_iter=1000, check_every=every)
            runs.append((x.cpu().numpy(), st))
        x, st = runs[0]
        print("GMRES(%d) with the polynomial: %d steps, %d restarts, |r| = %.3e" % (restart, st["iterations"], st["restarts"], st["rnorm"]))
        assert want["status"] == "converged" and 0 < want["iterations"] < 200
        assert (st["status"], st["iterations"], st["restarts"], st["columns"], st["breakdown"]) == \
            (want["status"], want["iterations"], want["restarts"], want["columns"], want["breakdown"]), st
        assert same(st["rnorm"], want["rnorm"]) and same(st["bnorm"], want["bnorm"]) and same(x, want["x"])
        for x2, st2 in runs[1:]:
            assert st2 == st and same(x2, x)
        assert info["precond"] == "chebyshev" and info["step_launches"] == S.gmres_launches(restart, "chebyshev", 4)["step"] == 9 + 4
        plan.destroy()


def test_pcg_on_the_device_takes_the_host_loops_count(env):
    """the one-shot with the defaults on the 32^2 Laplacian: DESIGN.md 3.27 records the counts this prints"""
    S, torch, cuda = env
    n, rp, ci, val = KN.laplacian(32)
    rp, ci = rp.astype(np.int32), ci.astype(np.int32)
    b = np.random.default_rng(30).standard_normal(n)
    drp, dci, dval, db = up(torch, cuda, rp, ci, val, b)
    x, st = S.pcg((n, drp, dci, dval), db, precond="chebyshev", rtol=RTOL)
    _, plain = S.pcg((n, drp, dci, dval), db, rtol=RTOL)
    table = host_estimate(S, dict(n=n, rp=rp, ci=ci, val=val))["table"]
    host_it, host_x = AN.host_pcg(n, rp, ci, val, b, lambda r: S.cheby_apply_ref(n, rp, ci, val, table, r), RTOL)
    residual = lambda v: float(np.linalg.norm(b - KN.matvec(n, rp, ci, val, v)))
    got, host = residual(x.cpu().numpy()), residual(host_x)
    bound = 2.0 * max(host, RTOL * np.linalg.norm(b))                        # the bound test_gpu_krylov.py uses for ILU(0)
    print("PCG with the polynomial: device %d iterations, host loop %d, plain CG on the device %d; true residual %.6e, the host "
          "loop's %.6e, bound %.6e" % (st["iterations"], host_it, plain["iterations"], got, host, bound))
    assert st["status"] == plain["status"] == "converged"
    assert st["iterations"] == host_it
    assert 2 * st["iterations"] <= plain["iterations"]
    assert got <= bound
    for one_shot, kw in ((S.bicgstab, {}), (S.gmres, dict(restart=20))):
        _, st2 = one_shot((n, drp, dci, dval), db, precond="chebyshev", rtol=RTOL, **kw)
        assert st2["status"] == "converged"


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
    fresh = S.ChebyshevPlan(n, P.drp, P.dci)                                 # no setup yet
    unsorted = P.dci.clone()
    unsorted[int(P.drp[5])], unsorted[int(P.drp[5]) + 1] = P.dci[int(P.drp[5]) + 1].item(), P.dci[int(P.drp[5])].item()
    nan = float("nan")
    bad = [lambda: fresh.apply(db, out=z), lambda: fresh.smooth(db, db.clone(), out=z), lambda: fresh.check(),   # before setup
           lambda: P.cheb.apply(z, out=z),                                     # z is r
           lambda: P.cheb.smooth(db, z, out=z), lambda: P.cheb.smooth(z, db, out=z),
           lambda: P.cheb.apply(db.cpu(), out=z), lambda: P.cheb.apply(db, out=z[:-1]), lambda: P.cheb.apply(db.float(), out=z),
           lambda: fresh.setup(P.dval[:-1]), lambda: fresh.setup(P.dval, lambda_max=0.0), lambda: fresh.setup(P.dval, lambda_max=-2.0),
           lambda: fresh.setup(P.dval, lambda_max=float("inf")), lambda: fresh.setup(P.dval, lambda_max=nan),
           lambda: S.ChebyshevPlan(n, P.drp, P.dci, degree=0), lambda: S.ChebyshevPlan(n, P.drp, P.dci, degree=65),
           lambda: S.ChebyshevPlan(n, P.drp, P.dci, eig_steps=0), lambda: S.ChebyshevPlan(n, P.drp, P.dci, eig_steps=65),
           lambda: S.ChebyshevPlan(n, P.drp, P.dci, eig_boost=0.5), lambda: S.ChebyshevPlan(n, P.drp, P.dci, eig_boost=nan),
           lambda: S.ChebyshevPlan(n, P.drp, P.dci, eig_ratio=1.0), lambda: S.ChebyshevPlan(n, P.drp, P.dci, eig_ratio=nan),
           lambda: S.ChebyshevPlan(n + 1, P.drp, P.dci),
           lambda: S.KrylovPlan(n, other_rp, P.dci, precond=P.cheb),           # a plan of another structure
           lambda: S.GmresPlan(n, other_rp, P.dci, precond=P.cheb),
           lambda: S.KrylovPlan(n, P.drp, P.dci, precond="chebyshev"), lambda: S.KrylovPlan(n, P.drp, P.dci, precond="ssor"),
           lambda: S.KrylovPlan(n, P.drp, P.dci, precond=3), lambda: S.KrylovPlan(n, P.drp, P.dci, precond=4),
           lambda: S.KrylovPlan(n, P.drp, P.dci, precond=(None, None)), lambda: S.GmresPlan(n, P.drp, P.dci, precond=4),
           lambda: S.pcg((n, P.drp, P.dci, P.dval), db, precond="ssor", x=z)]
    for k, call in enumerate(bad):
        with pytest.raises(E):
            call()
            pytest.fail("call %d was accepted" % k)
    with pytest.raises(E) as err:
        S.ChebyshevPlan(n, P.drp, unsorted)
    assert err.value.bad_row == 5
    L = S.lib()
    dev = torch.cuda.current_device()
    nnz = len(P.dci)
    assert L.sblas_hip_cheby_plan_speaks_for(P.cheb.handle, -1, n, nnz, P.drp.data_ptr(), P.dci.data_ptr()) == 0
    assert L.sblas_hip_cheby_plan_speaks_for(P.cheb.handle, dev + 1, n, nnz, P.drp.data_ptr(), P.dci.data_ptr()) != 0   # another device
    assert L.sblas_hip_cheby_plan_speaks_for(P.cheb.handle, -1, n, nnz, other_rp.data_ptr(), P.dci.data_ptr()) != 0
    h = ctypes.c_void_p()
    for create, head in ((L.sblas_hip_krylov_plan_create, (-1, None, 0)), (L.sblas_hip_gmres_plan_create, (-1, None))):
        tail = (30,) if create is L.sblas_hip_gmres_plan_create else ()
        args = head + (n, nnz, P.drp.data_ptr(), P.dci.data_ptr()) + tail + (None, 4)
        assert create(*args, None, None, ctypes.byref(h)) != 0               # code 4 without a handle is refused
        assert create(*args, P.cheb.handle, P.cheb.handle, ctypes.byref(h)) != 0   # upper_plan must be NULL
        assert create(*args, fresh.handle, None, ctypes.byref(h)) == 0 and h.value   # a plan before its setup may be taken: start needs it ready
        (L.sblas_hip_gmres_plan_destroy if tail else L.sblas_hip_krylov_plan_destroy)(h)
        h = ctypes.c_void_p()
    assert L.sblas_hip_cheby_plan_apply(P.cheb.handle, None, db.data_ptr(), None) != 0
    torch.cuda.synchronize()
    assert bool((z == -7.0).all())                                           # nothing ran
    fresh.destroy()
