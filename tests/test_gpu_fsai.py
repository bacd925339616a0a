"""The FSAI plan on the device (fsai.hip): G's pattern and values and check() against the host reference
(eager, after a second setup, replayed from a graph after the values changed, on the planted failures), apply against the
two planned SpMVs it is made of (also with offset operands), the plan inside PCG, BiCGStab and GMRES against loops composed
from parts, the iteration count and the refusals.  Every comparison of values is ==."""
import ctypes
import math

import numpy as np
import pytest

import amg_numerics as AN
import fsai_numerics as FN
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


def make_plan(env, c):
    """the case's plan, its pattern (if it has one) and max_row with it -> (plan, drp, dci)"""
    S, torch, cuda = env
    drp, dci = up(torch, cuda, c["rp"], c["ci"])
    pat = tuple(up(torch, cuda, *c["pattern"])) if c["pattern"] is not None else None
    return S.FsaiPlan(c["n"], drp, dci, pattern=pat, max_row=c["max_row"]), drp, dci


def host_g(S, c, val):
    grp, gci = S.fsai_pattern(c["n"], c["rp"], c["ci"], pattern=c["pattern"], max_row=c["max_row"])
    return (grp, gci) + S.fsai_ref(c["n"], c["rp"], c["ci"], val, grp, gci)


def assert_g_equals(plan, W, what):
    grp, gci, gval, bad = W
    drp, dci, dval = plan.csr()
    assert np.array_equal(drp.cpu().numpy(), grp) and np.array_equal(dci.cpu().numpy(), gci), what
    assert same(dval.cpu().numpy(), gval), what
    assert plan.check() == bad, what


class Built:
    """one case on the device: the plan after setup(val), and the host's G by the same rule"""

    def __init__(self, env, name):
        S, torch, cuda = env
        self.c = c = FN.case(name)
        self.n = c["n"]
        self.plan, self.drp, self.dci = make_plan(env, c)
        self.dval, = up(torch, cuda, c["val"])
        self.plan.setup(self.dval)
        self.host = host_g(S, c, c["val"])


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


# ---------------------------------------------------------------------------------------------------------------------
# setup
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FN.CASES)
def test_g_equals_the_reference_eagerly_and_after_a_second_setup(env, built, name):
    S, torch, cuda = env
    B = built(name)
    assert_g_equals(B.plan, B.host, name)
    info = B.plan.info()
    rows = np.diff(B.host[0])
    lim = S.fsai_limits()
    assert info["ready"] and info["launches"] == 2 and (info["n"], info["nnz"], info["nnz_g"]) == (B.n, len(B.c["ci"]), len(B.host[1]))
    assert info["longest"] == (rows.max() if B.n else 0)
    assert (info["rows_g4"], info["rows_g16"], info["rows_g64"]) == (int((rows <= lim["g4_max"]).sum()),
                                                                   int(((rows > lim["g4_max"]) & (rows <= lim["g16_max"])).sum()),
                                                                   int((rows > lim["g16_max"]).sum()))
    print("%s: %d rows of 4 lanes, %d of 16, %d of 64; %d units, %d bytes" % (name, info["rows_g4"], info["rows_g16"], info["rows_g64"],
                                                                             info["units"], info["bytes"]))
    values = B.c["val"] * (1.0 + 0.125 * np.sin(np.arange(len(B.c["val"]))))  # other values (no longer symmetric: only the lower part is read)
    B.plan.setup(up(torch, cuda, values)[0])
    assert_g_equals(B.plan, host_g(S, B.c, values), name + " with new values")
    B.plan.setup(B.dval)                                                     # repeatable: the first values again
    assert_g_equals(B.plan, B.host, name + " again")


@pytest.mark.parametrize("name", sorted(FN.failures()))
def test_a_failed_row_is_written_and_named_as_the_reference_does(env, name):
    S, torch, cuda = env
    n, rp, ci, val, row = FN.failures()[name]
    c = dict(n=n, rp=rp, ci=ci, pattern=None, max_row=None)
    plan, drp, dci = make_plan(env, c)
    plan.setup(up(torch, cuda, val)[0])
    W = host_g(S, c, val)
    assert W[3] == row
    assert_g_equals(plan, W, name)
    sound = np.where(np.isfinite(val) & (val != 0.0), np.abs(val), 1.0) * np.where(ci == np.repeat(np.arange(n), np.diff(rp)), 4.0, -0.25)
    plan.setup(up(torch, cuda, sound)[0])                                    # the flag is cleared by the next setup
    assert_g_equals(plan, host_g(S, c, sound), name + " mended")
    assert plan.check() is None
    plan.destroy()


def test_setup_and_apply_replay_in_a_graph_after_the_values_changed(env):
    S, torch, cuda = env
    c = FN.case("mixed70")
    n = c["n"]
    plan, drp, dci = make_plan(env, c)
    dval, = up(torch, cuda, c["val"])
    r = np.random.default_rng(6).standard_normal(n)
    dr, = up(torch, cuda, r)
    z = torch.zeros(n, dtype=torch.float64, device=cuda)
    plan.setup(dval), plan.apply(dr, out=z)                                  # eager first: loads the code objects
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            plan.setup(dval, stream=s)
            plan.apply(dr, out=z, stream=s)
    dval.mul_(1.0 + 0.1 * torch.cos(torch.arange(len(dval), device=cuda, dtype=torch.float64)))
    torch.cuda.synchronize()
    z.fill_(-7.0)
    g.replay()
    torch.cuda.synchronize()
    values = dval.cpu().numpy()
    assert_g_equals(plan, host_g(S, c, values), "replayed")
    assert same(z.cpu().numpy(), composed_apply(env, plan, dr).cpu().numpy())
    # a failure planted between replays is found by the replayed setup
    diag = SC.stored_diagonal(c["rp"], c["ci"])
    dval[int(diag[33])] = -1.0
    g.replay()
    torch.cuda.synchronize()
    values = dval.cpu().numpy()
    W = host_g(S, c, values)
    assert W[3] == 33
    assert_g_equals(plan, W, "replayed with a planted diagonal")
    plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# apply
# ---------------------------------------------------------------------------------------------------------------------
def composed_apply(env, plan, dr):
    """z = G^T (G r) by the two existing calls: SpmvPlan on csr(), then TransposePlan(csr()).spmv"""
    S, torch, cuda = env
    grp, gci, gval = plan.csr()
    n = plan.n
    t, z = torch.empty(n, dtype=torch.float64, device=cuda), torch.empty(n, dtype=torch.float64, device=cuda)
    spmv = S.SpmvPlan(n, n, grp, gci)
    spmv(gval, dr, 1.0, 0.0, t)
    tp = S.TransposePlan(n, n, grp, gci, gval)
    tp.spmv(t, 1.0, 0.0, z)
    torch.cuda.synchronize()
    tp.destroy(), spmv.destroy()
    return z


@pytest.mark.parametrize("name", [name for name in FN.CASES if name != "n0"])
def test_apply_equals_the_two_planned_products(env, built, name):
    S, torch, cuda = env
    B = built(name)
    n = B.n
    r = np.random.default_rng(5).standard_normal(n)
    want = composed_apply(env, B.plan, up(torch, cuda, r)[0]).cpu().numpy()
    G = FN.dense_g(n, *B.host[:3])
    assert np.allclose(want, G.T @ (G @ r), rtol=1e-12, atol=1e-13)         # and those are G^T (G r)
    for offset in (0, 1):                                                    # alignment must not reach the bits
        buf = [torch.full((n + 1,), -7.0, dtype=torch.float64, device=cuda) for _ in range(2)]
        dr, dz = (t[offset:offset + n] for t in buf)
        dr.copy_(up(torch, cuda, r)[0])
        assert B.plan.apply(dr, out=dz) is dz
        assert same(dz.cpu().numpy(), want), (name, offset)
        B.plan.apply(dr, out=dz)                                             # twice: nothing is carried from one call to the next
        assert same(dz.cpu().numpy(), want), (name, offset, "twice")
        assert same(dr.cpu().numpy(), r)                                     # the operand is read only
        assert all(float(t[n if offset == 0 else 0]) == -7.0 for t in buf)   # the element beside them is untouched
    assert same(B.plan.apply(up(torch, cuda, r)[0]).cpu().numpy(), want)


def test_the_empty_plan(env, built):
    S, torch, cuda = env
    B = built("n0")
    empty = torch.empty(0, dtype=torch.float64, device=cuda)
    assert B.plan.apply(empty).numel() == 0 and B.plan.check() is None and B.plan.info()["units"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# in the solvers
# ---------------------------------------------------------------------------------------------------------------------
class Parts(SC.Parts):
    """solver_compose's parts with M^-1 v by FsaiPlan.apply"""

    def __init__(self, env, n, rp, ci, val):
        self.fsai = None
        super().__init__(env, n, rp, ci, val, None, planned=False)

    def revalue(self, val):
        super().revalue(val)
        if self.fsai is None:
            self.fsai = self.env[0].FsaiPlan(self.n, self.drp, self.dci)
        self.fsai.setup(self.dval)

    def handle(self):
        return self.fsai

    def apply(self, v):
        S, torch, cuda = self.env
        return self.fsai.apply(up(torch, cuda, v)[0]).cpu().numpy()

    def destroy(self):
        if self.fsai is not None:
            self.fsai.destroy()
        self.fsai = None
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
    plan = S.KrylovPlan(n, P.drp, P.dci, method=method, precond=P.fsai)
    info = plan.info()
    db, = up(torch, cuda, b)
    runs = []
    for every in (1, 7, 50):
        dx, = up(torch, cuda, x0)
        x, st = plan.solve(P.dval, db, x=dx, rtol=RTOL, max_iter=1000, check_every=every)
        runs.append((x.cpu().numpy(), st))
    x, st = runs[0]
    print("%s with FSAI: %d iterations, |r| = %.3e (composition: %d, %.3e); %d launches an iteration"
          % (method, st["iterations"], st["rnorm"], want_it, want_rnorm, info["launches"]))
    assert want_status == "converged" and 0 < want_it < 200
    assert (st["status"], st["iterations"]) == (want_status, want_it), st
    assert same(st["rnorm"], want_rnorm) and same(st["bnorm"], math.sqrt(S.krylov_dot_ref(b, b))) and same(x, want_x)
    for x2, st2 in runs[1:]:
        assert st2 == st and same(x2, x)
    lim = S.krylov_limits()
    assert info["precond"] == "fsai" and info["vectors"] == (lim["pcg_vectors"] if method == "pcg" else lim["bicgstab_vectors"]) + 1
    assert info["launches"] == S.krylov_launches(method, "fsai", 2) == (8 + 2 if method == "pcg" else 10 + 2 * 2)
    plan.destroy()


def test_gmres_with_the_plan_equals_its_composition(env, conv):
    S, torch, cuda = env
    n, b, P = conv["n"], conv["b"], conv["P"]
    x0 = 0.1 * np.random.default_rng(31).standard_normal(n)
    for restart in (30, 5):                                                 # 5: closes and restarts with an apply in them
        want = SC.composed_gmres(P.matvec, P.apply, P.dot, P.dots, b, x0, restart, RTOL, 1000)
        plan = S.GmresPlan(n, P.drp, P.dci, restart=restart, precond=P.fsai)
        info = plan.info()
        db, = up(torch, cuda, b)
        runs = []
        for every in (1, 7, 50):
            dx, = up(torch, cuda, x0)
            x, st = plan.solve(P.dval, db, x=dx, rtol=RTOL, max_iter=1000, check_every=every)
            runs.append((x.cpu().numpy(), st))
        x, st = runs[0]
        print("GMRES(%d) with FSAI: %d steps, %d restarts, |r| = %.3e" % (restart, st["iterations"], st["restarts"], st["rnorm"]))
        assert want["status"] == "converged" and 0 < want["iterations"] < 200
        assert (st["status"], st["iterations"], st["restarts"], st["columns"], st["breakdown"]) == \
            (want["status"], want["iterations"], want["restarts"], want["columns"], want["breakdown"]), st
        assert same(st["rnorm"], want["rnorm"]) and same(st["bnorm"], want["bnorm"]) and same(x, want["x"])
        for x2, st2 in runs[1:]:
            assert st2 == st and same(x2, x)
        assert info["precond"] == "fsai" and info["step_launches"] == S.gmres_launches(restart, "fsai", 2)["step"] == 9 + 2
        plan.destroy()


def test_pcg_on_the_device_takes_the_host_loops_count(env):
    """the one-shot on the 32^2 Laplacian: DESIGN.md 3.39 records the counts this prints"""
    S, torch, cuda = env
    n, rp, ci, val = KN.laplacian(32)
    rp, ci = rp.astype(np.int32), ci.astype(np.int32)
    b = np.random.default_rng(30).standard_normal(n)
    drp, dci, dval, db = up(torch, cuda, rp, ci, val, b)
    x, st = S.pcg((n, drp, dci, dval), db, precond="fsai", rtol=RTOL)
    _, plain = S.pcg((n, drp, dci, dval), db, rtol=RTOL)
    grp, gci = S.fsai_pattern(n, rp, ci)
    G = FN.dense_g(n, grp, gci, S.fsai_ref(n, rp, ci, val, grp, gci)[0])
    host_it, host_x = AN.host_pcg(n, rp, ci, val, b, lambda r: G.T @ (G @ r), RTOL)
    residual = lambda v: float(np.linalg.norm(b - KN.matvec(n, rp, ci, val, v)))
    got, host = residual(x.cpu().numpy()), residual(host_x)
    bound = 2.0 * max(host, RTOL * np.linalg.norm(b))                        # the bound test_gpu_krylov.py uses for ILU(0)
    print("PCG with FSAI: device %d iterations, host loop %d, plain CG on the device %d; true residual %.6e, the host loop's %.6e, "
          "bound %.6e" % (st["iterations"], host_it, plain["iterations"], got, host, bound))
    assert st["status"] == plain["status"] == "converged"
    assert st["iterations"] == host_it
    assert st["iterations"] < plain["iterations"]
    assert got <= bound
    for one_shot, kw in ((S.bicgstab, {}), (S.gmres, dict(restart=20))):
        _, st2 = one_shot((n, drp, dci, dval), db, precond="fsai", rtol=RTOL, **kw)
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
    wide = torch.full((n + 1,), -7.0, dtype=torch.float64, device=cuda)
    other_rp = P.drp.clone()
    fresh = S.FsaiPlan(n, P.drp, P.dci)                                      # no setup yet
    bad = [lambda: fresh.apply(db, out=z), lambda: fresh.check(),             # before setup
           lambda: P.fsai.apply(z, out=z),                                    # z is r
           lambda: P.fsai.apply(wide[:n], out=wide[1:]),                      # z overlaps r
           lambda: P.fsai.apply(db.cpu(), out=z), lambda: P.fsai.apply(db, out=z.cpu()),   # a wrong device
           lambda: P.fsai.apply(db.float(), out=z), lambda: P.fsai.apply(db, out=z.float()),   # a wrong dtype
           lambda: P.fsai.apply(db, out=z[:-1]), lambda: fresh.setup(P.dval[:-1]), lambda: fresh.setup(P.dval.float()),
           lambda: S.FsaiPlan(n, P.drp, P.dci, max_row=0), lambda: S.FsaiPlan(n, P.drp, P.dci, max_row=65),
           lambda: S.FsaiPlan(n, P.drp, P.dci, pattern=(P.drp,)), lambda: S.FsaiPlan(n + 1, P.drp, P.dci),
           lambda: S.KrylovPlan(n, other_rp, P.dci, precond=P.fsai),           # a plan of another structure
           lambda: S.GmresPlan(n, other_rp, P.dci, precond=P.fsai),
           lambda: S.KrylovPlan(n, P.drp, P.dci, precond="fsai"), lambda: S.KrylovPlan(n, P.drp, P.dci, precond=6),
           lambda: S.GmresPlan(n, P.drp, P.dci, precond=6),
           lambda: S.KrylovMultiPlan(n, P.drp, P.dci, 4, precond=P.fsai),     # no block apply yet
           lambda: S.pcg((n, P.drp, P.dci, P.dval), db, precond="spai", x=z)]
    for k, call in enumerate(bad):
        with pytest.raises(E):
            call()
            pytest.fail("call %d was accepted" % k)
    # a row over 64 without max_row, and a pattern row without its diagonal: refused at create and named
    c = FN.case("clique70_max64")
    crp, cci = up(torch, cuda, c["rp"], c["ci"])
    with pytest.raises(E) as err:
        S.FsaiPlan(c["n"], crp, cci)
    assert err.value.bad_row == 64
    g = FN.case("grid12_squared")
    grp_, gci_ = up(torch, cuda, g["rp"], g["ci"])
    prp, pci = g["pattern"]
    keep = np.ones(len(pci), bool)
    keep[prp[31 + 1] - 1] = False                                            # row 31 loses its diagonal, the last entry of its lower row
    lost_rp = prp.copy()
    lost_rp[32:] -= 1
    with pytest.raises(E) as err:
        S.FsaiPlan(g["n"], grp_, gci_, pattern=tuple(up(torch, cuda, lost_rp, pci[keep])))
    assert err.value.bad_row == 31
    unsorted = P.dci.clone()
    unsorted[int(P.drp[5])], unsorted[int(P.drp[5]) + 1] = P.dci[int(P.drp[5]) + 1].item(), P.dci[int(P.drp[5])].item()
    with pytest.raises(E) as err:
        S.FsaiPlan(n, P.drp, unsorted)
    assert err.value.bad_row == 5
    L = S.lib()
    dev = torch.cuda.current_device()
    nnz = len(P.dci)
    assert L.sblas_hip_fsai_plan_speaks_for(P.fsai.handle, -1, n, nnz, P.drp.data_ptr(), P.dci.data_ptr()) == 0
    assert L.sblas_hip_fsai_plan_speaks_for(P.fsai.handle, dev + 1, n, nnz, P.drp.data_ptr(), P.dci.data_ptr()) != 0   # another device
    assert L.sblas_hip_fsai_plan_speaks_for(P.fsai.handle, -1, n, nnz, other_rp.data_ptr(), P.dci.data_ptr()) != 0
    h = ctypes.c_void_p()
    for create, head in ((L.sblas_hip_krylov_plan_create, (-1, None, 0)), (L.sblas_hip_gmres_plan_create, (-1, None))):
        tail = (30,) if create is L.sblas_hip_gmres_plan_create else ()
        for kind in (6, 5):
            args = head + (n, nnz, P.drp.data_ptr(), P.dci.data_ptr()) + tail + (None, kind)
            assert create(*args, None, None, ctypes.byref(h)) != 0           # code 6 without a handle is refused; 5 is no kind
            assert create(*args, P.fsai.handle, P.fsai.handle, ctypes.byref(h)) != 0   # upper_plan must be NULL
        args = head + (n, nnz, P.drp.data_ptr(), P.dci.data_ptr()) + tail + (None,)
        assert create(*args, 5, P.fsai.handle, None, ctypes.byref(h)) != 0   # 5 stays no kind, whatever comes with it
        assert create(*args, 6, fresh.handle, None, ctypes.byref(h)) == 0 and h.value   # a plan before its setup may be taken: start needs it ready
        (L.sblas_hip_gmres_plan_destroy if tail else L.sblas_hip_krylov_plan_destroy)(h)
        h = ctypes.c_void_p()
    assert L.sblas_hip_fsai_plan_apply(P.fsai.handle, None, db.data_ptr(), None) != 0
    torch.cuda.synchronize()
    assert bool((z == -7.0).all()) and bool((wide == -7.0).all())            # nothing ran
    fresh.destroy()
