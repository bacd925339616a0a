"""The AMG cycle on a block of columns on the GPU (AmgPlan.apply_multi, amg_sweep_multi, amg_restrict_multi,
amg_prolong_multi) and its seat under KrylovMultiPlan, pcg_multi and bicgstab_multi.

The contract is one sentence: column j of a block result has exactly the bits of the single-column entry on column j.  So
every comparison of values is == against the EXISTING single-column entries (amg_sweep, amg_restrict, amg_prolong,
AmgPlan.apply), which their own suites hold against the host restatements; a whole solve is == against the lockstep loop
of tests/multi_compose.py composed from an SpmmPlan of the test's own, krylov_dot per column and AmgPlan.apply on one
column.  Only "it solves" holds a tolerance: the factor 4 of test_gpu_krylov_multi.py on the true residual of the same
column's KrylovPlan + AmgPlan solve."""
import ctypes as C

import numpy as np
import pytest

import amg_numerics as AN
import krylov_numerics as KN
import multi_compose as MC
import solver_compose as SC

pytestmark = pytest.mark.gpu

RTOL = 1e-10
SENTINEL = -7.0
CASES = ["n1", "tridiagonal3000", "grid24", "clique130", "star5000", "random4000", "aniso32"]


@pytest.fixture(scope="module")
def env(sblas, cuda):
    import torch
    return sblas, torch, cuda


def up(torch, cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def same(a, b):
    return KN.same_bits(a, b)


class Guarded:
    """host (n, s) as a device block at leading dimension ld whose first element sits `offset` elements into an
    allocation, with one guard row before and after and the padding columns all holding the sentinel"""

    def __init__(self, torch, cuda, host, ld=None, offset=0):
        n, s = host.shape
        self.n, self.s, self.ld, self.offset = n, s, (s if ld is None else ld), offset
        self.buf = torch.full((offset + (n + 2) * self.ld + 1,), SENTINEL, dtype=torch.float64, device=cuda)
        self.view = self.buf[offset + self.ld:offset + (n + 1) * self.ld].view(n, self.ld)[:, :s]
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(host)).to(cuda))

    def host(self):
        return self.view.cpu().numpy()

    def intact(self):
        """everything outside the block still holds the sentinel"""
        h = self.buf.cpu().numpy().copy()
        inner = h[self.offset + self.ld:self.offset + (self.n + 1) * self.ld].reshape(self.n, self.ld)
        inner[:, :self.s] = SENTINEL
        return bool((h == SENTINEL).all())


def layouts(s):
    """(ld, offset): ld = s and s + 3, the base 16-byte aligned and one element off.  The 16-byte path runs where the
    base and ld * 8 are multiples of 16 and a tile is full (s = 8 at ld 8; the first tile of s = 11 at ld 14; s = 64)."""
    return [(ld, offset) for ld in (s, s + 3) for offset in (0, 1)]


class Built:
    """one case on the device with one prolongator and aggregation; set up with the defaults"""

    def __init__(self, env, name, prolongator="plain", aggregation="host"):
        S, torch, cuda = env
        self.c = c = AN.case(name)
        self.n = c["n"]
        self.drp, self.dci, self.dval = up(torch, cuda, c["rp"], c["ci"], c["val"])
        self.plan = S.AmgPlan(self.n, self.drp, self.dci, val=self.dval if c["theta"] > 0.0 else None, theta=c["theta"],
                              prolongator=prolongator, aggregation=aggregation)
        self.plan.setup(self.dval)


@pytest.fixture(scope="module")
def built(env):
    made = {}

    def get(name, prolongator="plain", aggregation="host"):
        key = (name, prolongator, aggregation)
        if key not in made:
            made[key] = Built(env, *key)
        return made[key]
    yield get
    for b in made.values():
        b.plan.destroy()


def level_sizes(plan):
    return [(plan.level(l)["n"], plan.level(l)["n_coarse"]) for l in range(plan.info()["levels"])]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the single kernels: every column is the single-column entry on that column
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prolongator", ["plain", "smoothed"])
@pytest.mark.parametrize("name", CASES)
def test_block_kernels_have_the_single_kernels_bits(env, built, name, prolongator):
    S, torch, cuda = env
    B = built(name, prolongator)
    plan = B.plan
    widths = (1, 3, 8, 11) + ((64,) if name == "grid24" else ())
    smax = max(widths)
    rng = np.random.default_rng(23)
    sizes = level_sizes(plan)
    if name == "n1":
        assert sizes == [(1, 0)]
    z = lambda k: torch.zeros(k, dtype=torch.float64, device=cuda)
    for l, (n, nc) in list(enumerate(sizes))[:2]:
        hb, hx = rng.standard_normal((n, smax)), rng.standard_normal((n, smax))
        # the references, once: the single-column entries on contiguous copies of the columns
        want = {mode: np.zeros((n, smax)) for mode in ("sweep", "residual", "first")}
        for j in range(smax):
            db, dx = up(torch, cuda, hb[:, j], hx[:, j])
            for mode in want:
                want[mode][:, j] = S.amg_sweep(plan, l, db, dx, z(n), mode=mode).cpu().numpy()
        if nc:
            he = rng.standard_normal((nc, smax))
            want_bc, want_x = np.zeros((nc, smax)), np.zeros((n, smax))
            for j in range(smax):
                dres, de, dx = up(torch, cuda, hb[:, j], he[:, j], hx[:, j])
                want_bc[:, j] = S.amg_restrict(plan, l, dres, z(nc)).cpu().numpy()
                want_x[:, j] = S.amg_prolong(plan, l, de, dx, scale=0.75).cpu().numpy()
        else:                                                                # the coarsest level has no transfers
            one = torch.zeros((n, 1), dtype=torch.float64, device=cuda)
            with pytest.raises(S.SblasError):
                S.amg_restrict_multi(plan, l, one, one.clone())
            assert S.lib().sblas_hip_amg_restrict_multi_f64(plan.handle, None, l, 1, one.data_ptr(), 1, one.clone().data_ptr(), 1) == 1
        for s in widths:
            for ld, offset in layouts(s):
                gb, gx = Guarded(torch, cuda, hb[:, :s], ld, offset), Guarded(torch, cuda, hx[:, :s], ld, offset)
                for mode in ("sweep", "residual", "first"):
                    gy = Guarded(torch, cuda, np.full((n, s), SENTINEL), ld, offset)
                    out = S.amg_sweep_multi(plan, l, gb.view, None if mode == "first" else gx.view, gy.view, mode=mode)
                    assert out is gy.view
                    assert same(gy.host(), want[mode][:, :s]), (name, l, mode, s, ld, offset)
                    assert gy.intact() and gb.intact() and gx.intact(), (name, l, mode, s, ld, offset)
                assert same(gb.host(), hb[:, :s]) and same(gx.host(), hx[:, :s])
                if nc:
                    gbc = Guarded(torch, cuda, np.full((nc, s), SENTINEL), ld, offset)
                    S.amg_restrict_multi(plan, l, gb.view, gbc.view)
                    assert same(gbc.host(), want_bc[:, :s]) and gbc.intact(), (name, l, "restrict", s, ld, offset)
                    ge = Guarded(torch, cuda, he[:, :s], ld, offset)
                    S.amg_prolong_multi(plan, l, ge.view, gx.view, scale=0.75)
                    assert same(gx.host(), want_x[:, :s]) and gx.intact() and ge.intact(), (name, l, "prolong", s, ld, offset)
            # operands of different layouts in one launch: b aligned, x one element off, y at a wider ld
            gb, gx = Guarded(torch, cuda, hb[:, :s], s + (s % 2), 0), Guarded(torch, cuda, hx[:, :s], s, 1)
            gy = Guarded(torch, cuda, np.full((n, s), SENTINEL), s + 5, 0)
            S.amg_sweep_multi(plan, l, gb.view, gx.view, gy.view)
            assert same(gy.host(), want["sweep"][:, :s]) and gy.intact(), (name, l, s)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the block cycle: column j is apply() on column j
# ---------------------------------------------------------------------------------------------------------------------
def cycle_columns(n, seed=31):
    """a random column, e_k, a zero column, 1e6 random and 1e-150 random"""
    rng = np.random.default_rng(seed)
    e = np.zeros(n)
    e[n // 3] = 1.0
    return np.ascontiguousarray(np.stack([rng.standard_normal(n), e, np.zeros(n), 1e6 * rng.standard_normal(n),
                                          1e-150 * rng.standard_normal(n)], axis=1))


def columns_of_apply(torch, cuda, plan, R):
    return np.stack([plan.apply(up(torch, cuda, R[:, j])[0]).cpu().numpy() for j in range(R.shape[1])], axis=1)


@pytest.mark.parametrize("aggregation", ["host", "device"])
@pytest.mark.parametrize("prolongator", ["plain", "smoothed"])
@pytest.mark.parametrize("name", CASES)
def test_apply_multi_is_apply_on_every_column(env, built, name, prolongator, aggregation):
    S, torch, cuda = env
    B = built(name, prolongator, aggregation)
    plan, n = B.plan, B.n
    R = cycle_columns(n)
    s = R.shape[1]
    dval = B.dval.clone()
    for smoother in ("jacobi", "l1"):
        for nu in (1, 2):
            plan.setup(dval, smoother=smoother, nu=nu)
            want = columns_of_apply(torch, cuda, plan, R)
            assert not want[:, 2].any()                                      # M^-1 0 = 0
            dR, = up(torch, cuda, R)
            for _ in range(2):                                               # eagerly, twice: nothing of the first is left behind
                Z = plan.apply_multi(dR)
                assert tuple(Z.shape) == (n, s) and same(Z.cpu().numpy(), want), (name, prolongator, aggregation, smoother, nu)
            assert plan.multi_info()["width"] >= s and plan.multi_info()["launches"] == plan.info()["launches"] == S.amg_launches(
                plan.info()["levels"], nu=nu)                                # a walk call is one launch whatever s is
            # R and out column slices of wider tensors, one element off an aligned base
            gR, gZ = Guarded(torch, cuda, R, s + 3, 1), Guarded(torch, cuda, np.full((n, s), SENTINEL), s + 2, 1)
            assert plan.apply_multi(gR.view, out=gZ.view) is gZ.view
            assert same(gZ.host(), want) and gZ.intact() and gR.intact() and same(gR.host(), R)
    # a captured block cycle replayed after a NEW setup with new values behind the same pointer
    dR, = up(torch, cuda, R)
    Z = torch.zeros((n, s), dtype=torch.float64, device=cuda)
    plan.apply_multi(dR, out=Z)                                              # eager first: loads the code objects
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            plan.apply_multi(dR, out=Z, stream=side)
    dval.mul_(1.0 + 0.1 * torch.cos(torch.arange(len(dval), device=cuda, dtype=torch.float64)))
    plan.setup(dval, smoother="l1", nu=2)                                    # the options the graph was captured with
    Z.fill_(SENTINEL)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert same(Z.cpu().numpy(), columns_of_apply(torch, cuda, plan, R)), (name, prolongator, aggregation)
    plan.setup(B.dval)


# ---------------------------------------------------------------------------------------------------------------------
# 3. no column of the cycle can reach another column
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prolongator", ["plain", "smoothed"])
@pytest.mark.parametrize("name", CASES)
def test_columns_do_not_touch(env, built, name, prolongator):
    S, torch, cuda = env
    B = built(name, prolongator)
    plan, n = B.plan, B.n
    s = 11                                                                   # a full tile and a ragged one
    R = np.random.default_rng(41).standard_normal((n, s))
    Z = plan.apply_multi(up(torch, cuda, R)[0]).cpu().numpy()
    assert np.isfinite(Z).all()
    for j, poison in ((4, np.nan), (9, np.inf), (0, -np.inf)):
        bad = R.copy()
        bad[:, j] = poison
        for layout in ((s, 0), (s + 3, 1)):
            got = plan.apply_multi(Guarded(torch, cuda, bad, *layout).view).cpu().numpy()
            others = [c for c in range(s) if c != j]
            assert same(got[:, others], Z[:, others]), (name, prolongator, j, poison, layout)
            assert not np.isfinite(got[:, j]).any()                          # its own column, nobody else's
        one = bad.copy()                                                     # one poisoned ENTRY: still that column alone
        one[:, j] = R[:, j]
        one[n // 2, j] = poison
        got = plan.apply_multi(up(torch, cuda, one)[0]).cpu().numpy()
        assert same(got[:, others], Z[:, others]) and same(got[:, j], plan.apply(up(torch, cuda, one[:, j])[0]).cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------------
# 4. the solvers with the block cycle against their own composition
# ---------------------------------------------------------------------------------------------------------------------
class AmgParts:
    """the device's parts of a lockstep loop: A V by an SpmmPlan of the test's own for width s, called row-major; the
    pinned dot per column; M^-1 by AmgPlan.apply on ONE column"""

    def __init__(self, env, A, s, prolongator):
        S, torch, cuda = self.env = env
        self.n, self.rp, self.ci, self.val = A[0], A[1].astype(np.int32), A[2].astype(np.int32), A[3]
        self.s = s
        self.drp, self.dci, self.dval = up(torch, cuda, self.rp, self.ci, self.val)
        self.spmm = S.SpmmPlan(self.n, self.n, self.drp, self.dci, s)
        self.ws = torch.empty(max(S.spmm_workspace_bytes(self.n, self.n, len(self.ci), s) // 8, 1), dtype=torch.float64, device=cuda)
        self.amg = S.AmgPlan(self.n, self.drp, self.dci, prolongator=prolongator)
        self.amg.setup(self.dval)

    def matvec(self, V):
        S, torch, cuda = self.env
        dv, = up(torch, cuda, V)
        out = torch.empty(self.n * self.s, dtype=torch.float64, device=cuda)
        self.spmm.spmm_ordered(self.dval, dv.reshape(-1), self.s, S.ROW_MAJOR, self.s, 1.0, 0.0, out, self.s, S.ROW_MAJOR, self.ws)
        return out.cpu().numpy().reshape(self.n, self.s)

    def dot(self, a, b):
        S, torch, cuda = self.env
        return float(S.krylov_dot(*up(torch, cuda, a, b)).cpu().numpy()[0])

    def apply(self, v):
        S, torch, cuda = self.env
        return self.amg.apply(up(torch, cuda, v)[0]).cpu().numpy()

    def destroy(self):
        self.spmm.destroy(), self.amg.destroy()


MATRICES = {"pcg": lambda: KN.laplacian(32), "bicgstab": lambda: KN.convection_diffusion(24)}
SOLVES = [("pcg", "plain"), ("pcg", "smoothed"), ("bicgstab", "plain")]


@pytest.fixture(scope="module")
def composed(env):
    """the composed loop of every case, run once and shared by the tests that compare against it"""
    made = {}

    def get(method, prolongator):
        key = (method, prolongator)
        if key not in made:
            A = MATRICES[method]()
            B, X0, names = MC.columns(A[0], lambda v: KN.matvec(*A, v))
            P = AmgParts(env, A, B.shape[1], prolongator)
            loop = MC.composed_pcg_multi if method == "pcg" else MC.composed_bicgstab_multi
            want = loop(P.matvec, P.apply, P.dot, B, X0, RTOL, 1000)
            for w in want:
                w.x.setflags(write=False)
            made[key] = dict(A=A, B=B, X0=X0, names=names, P=P, want=want)
        return made[key]
    yield get
    for c in made.values():
        c["P"].destroy()


def assert_solved(st, X, c):
    x = X.cpu().numpy()
    for j, (name, w) in enumerate(zip(c["names"], c["want"])):
        got = dict(status=st["status"][j], iterations=int(st["iterations"][j]), breakdown=st["breakdown"][j])
        assert got == dict(status=w.status, iterations=w.iterations, breakdown=w.breakdown), (name, got, w.asdict())
        for key in ("rnorm", "bnorm", "alpha", "beta", "omega"):
            assert same(st[key][j], getattr(w, key)), (name, key, st[key][j], getattr(w, key))
        assert same(x[:, j], w.x), (name, "x")
    assert st["running"] == 0


@pytest.mark.parametrize("check_every", [1, 7, 50])
@pytest.mark.parametrize("method,prolongator", SOLVES)
def test_the_solver_with_a_block_cycle_equals_its_own_composition(env, composed, method, prolongator, check_every):
    S, torch, cuda = env
    c = composed(method, prolongator)
    P, n, s = c["P"], c["A"][0], c["B"].shape[1]
    assert s == 9
    by = dict(zip(c["names"], c["want"]))
    # the cases are worth having: the NaN column breaks down while the others converge, and the stops are spread out, so
    # the block cycle keeps running on frozen columns while others go on
    assert (by["nan"].status, by["nan"].iterations) == ("breakdown", 0)
    assert by["nan"].breakdown == (SC.DENOM_PQ if method == "pcg" else SC.DENOM_RV)
    assert all(w.status == "converged" for k, w in by.items() if k != "nan")
    assert (by["zero"].iterations, by["zero"].x.any()) == (0, False)
    assert MC.spread_ok([w.iterations for w in c["want"]]), [w.iterations for w in c["want"]]
    plan = S.KrylovMultiPlan(n, P.drp, P.dci, s, method=method, precond=P.amg)
    dB = Guarded(torch, cuda, c["B"]).view
    gX = Guarded(torch, cuda, c["X0"], s + 3, 1)                            # X: a slice of a wider tensor
    X, st = plan.solve(P.dval, dB, X=gX.view, rtol=RTOL, max_iter=1000, check_every=check_every)
    assert X is gX.view
    if check_every == 7:
        print("%s with a %s block cycle: iterations %s" % (method, prolongator, dict(zip(c["names"], st["iterations"].tolist()))))
    assert_solved(st, X, c)
    assert gX.intact()
    info = plan.info()
    cycle = P.amg.info()["launches"]
    assert (info["n"], info["nrhs"], info["method"], info["precond"]) == (n, s, method, "amg")
    assert info["launches"] == S.krylov_multi_launches(method, P.amg, 0) == (7 + cycle if method == "pcg" else 8 + 2 * cycle)
    assert P.amg.multi_info()["width"] >= s
    # a second solve on the same plan has the same bits, X contiguous this time (the 16-byte path where a tile is full)
    X2, st2 = plan.solve(P.dval, dB, X=Guarded(torch, cuda, c["X0"]).view, rtol=RTOL, max_iter=1000, check_every=check_every)
    assert_solved(st2, X2, c)
    plan.destroy()


@pytest.mark.parametrize("method,prolongator", [("pcg", "smoothed"), ("bicgstab", "plain")])
def test_iterate_with_a_block_cycle_replays_in_a_graph(env, composed, method, prolongator):
    S, torch, cuda = env
    c = composed(method, prolongator)
    P, n, s = c["P"], c["A"][0], c["B"].shape[1]
    plan = S.KrylovMultiPlan(n, P.drp, P.dci, s, method=method, precond=P.amg)
    dB, dX = Guarded(torch, cuda, c["B"]).view, Guarded(torch, cuda, c["X0"], s + 3, 1).view
    ex, est = plan.solve(P.dval, dB, X=dX.clone(), rtol=RTOL, check_every=9)  # eager: the bits to meet; loads the code objects
    assert_solved(est, ex, c)
    plan.start(P.dval, dB, dX, rtol=RTOL)                                    # start runs eagerly
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):                              # a linear chain of launches
            plan.iterate(9)
    st = plan.status()
    assert int(st["iterations"].max()) == 0                                  # capturing ran nothing
    most = max(w.iterations for w in c["want"])
    for round_ in range(2):                                                  # the second: the same graph after a NEW start
        if round_:
            dX.copy_(torch.from_numpy(c["X0"]).to(cuda))
            plan.start(P.dval, dB, dX, rtol=RTOL)
        for replay in range(1, 200):
            g.replay()
            st = plan.status()
            if st["running"] == 0:
                break
        assert replay == -(-most // 9), (replay, most)
        assert_solved(st, dX, c)
    plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# 5. it solves
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,prolongator", SOLVES)
def test_it_solves_as_well_as_the_single_solver(env, composed, method, prolongator):
    """Each converged column's true residual |b_j - A x_j| (float64, on the host) against the same column's KrylovPlan
    solve with the same AmgPlan: within the factor 4 of test_gpu_krylov_multi.py.  The two differ in the product alone
    (the SpMM's row sums against the SpMV's); the cycle's bits are the same on both sides.  DESIGN.md 3.30 records the
    observed range."""
    S, torch, cuda = env
    c = composed(method, prolongator)
    P, n, s = c["P"], c["A"][0], c["B"].shape[1]
    B, X0 = c["B"], c["X0"]
    X, st = S.KrylovMultiPlan(n, P.drp, P.dci, s, method=method, precond=P.amg).solve(P.dval, Guarded(torch, cuda, B).view,
                                                                                       X=Guarded(torch, cuda, X0).view, rtol=RTOL)
    x = X.cpu().numpy()
    single = S.KrylovPlan(n, P.drp, P.dci, method=method, precond=P.amg)
    true = lambda b, v: float(np.linalg.norm(b - KN.matvec(n, P.rp, P.ci, P.val, v)))
    ratios, counts = {}, {}
    for j, name in enumerate(c["names"]):
        db, dx = up(torch, cuda, B[:, j], X0[:, j])
        xs, sst = single.solve(P.dval, db, x=dx, rtol=RTOL)
        assert st["status"][j] == sst["status"], (name, st["status"][j], sst)
        if sst["status"] != "converged":
            assert name == "nan"
            continue
        mine, theirs = true(B[:, j], x[:, j]), true(B[:, j], xs.cpu().numpy())
        ratios[name] = mine / theirs if theirs > 0.0 else (1.0 if mine == 0.0 else np.inf)
        counts[name] = (int(st["iterations"][j]), sst["iterations"])
        assert mine <= 4.0 * theirs, (name, mine, theirs)
    print("%s with a %s block cycle: true residual over the single solver's: %s" % (method, prolongator, {k: "%.6g" % v for k, v in ratios.items()}))
    print("    iterations (batched, single): %s" % counts)
    assert len(ratios) == s - 1
    single.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# 6. edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lap(env):
    S, torch, cuda = env
    n, rp, ci, val = KN.laplacian(24)
    rp, ci = rp.astype(np.int32), ci.astype(np.int32)
    drp, dci, dval = up(torch, cuda, rp, ci, val)
    return dict(n=n, rp=rp, ci=ci, val=val, drp=drp, dci=dci, dval=dval)


def test_empty_and_one_row(env):
    S, torch, cuda = env
    # n = 0: nothing is launched, every column reads converged
    rp0, ci0 = torch.zeros(1, dtype=torch.int32, device=cuda), torch.zeros(0, dtype=torch.int32, device=cuda)
    v0 = torch.zeros(0, dtype=torch.float64, device=cuda)
    amg = S.AmgPlan(0, rp0, ci0)
    amg.setup(v0)
    e = torch.zeros((0, 3), dtype=torch.float64, device=cuda)
    assert tuple(amg.apply_multi(e).shape) == (0, 3) and amg.multi_info() == dict(width=3, bytes=0, launches=0)
    plan = S.KrylovMultiPlan(0, rp0, ci0, 3, precond=amg)
    X, st = plan.solve(v0, e, X=e.clone())
    assert st["status"] == ["converged"] * 3 and not st["iterations"].any() and st["running"] == 0
    assert plan.info()["precond"] == "amg" and plan.info()["launches"] == 7
    plan.destroy(), amg.destroy()
    # n = 1: one level, the coarsest sweeps only; the solve converges in one iteration
    c = AN.case("n1")
    drp, dci, dval = up(torch, cuda, c["rp"], c["ci"], c["val"])
    amg = S.AmgPlan(1, drp, dci)
    amg.setup(dval)
    assert amg.info()["levels"] == 1 and amg.info()["launches"] == 8
    R = np.array([[3.0, 0.0, -1e-150, np.inf]])
    Z = amg.apply_multi(up(torch, cuda, R)[0]).cpu().numpy()
    assert same(Z, np.stack([amg.apply(up(torch, cuda, R[:, j])[0]).cpu().numpy() for j in range(4)], axis=1))
    for solve in (S.pcg_multi, S.bicgstab_multi):
        B = np.array([[3.0, 0.0, -2.0]])
        X, st = solve((1, drp, dci, dval), up(torch, cuda, B)[0], precond="amg", rtol=1e-12)
        assert st["status"] == ["converged"] * 3 and list(st["iterations"]) == [1, 0, 1]
        assert np.allclose(X.cpu().numpy(), B / 2.0, rtol=1e-12, atol=0.0)
    amg.destroy()


def test_one_column_sixty_four_and_the_limit(env, lap):
    S, torch, cuda = env
    n, rng = lap["n"], np.random.default_rng(5)
    amg = S.AmgPlan(n, lap["drp"], lap["dci"], prolongator="smoothed")
    amg.setup(lap["dval"])
    # reserve only grows
    assert amg.multi_info()["width"] == 0 and amg.multi_info()["bytes"] == 0
    before = amg.info()["bytes"]
    assert amg.reserve(4) == 4
    held = amg.multi_info()["bytes"]
    assert held >= 4 * 4 * 8 * sum(k for k, _ in amg.levels()) and amg.reserve(2) == 4 and amg.multi_info()["bytes"] == held
    assert amg.info()["bytes"] == before                                     # the plan's own bytes are what they were
    # s = 1: the block cycle is the cycle, and the solve equals its composition bit for bit
    r = rng.standard_normal((n, 1))
    assert same(amg.apply_multi(up(torch, cuda, r)[0]).cpu().numpy()[:, 0], amg.apply(up(torch, cuda, r[:, 0])[0]).cpu().numpy())
    A = (n, lap["rp"], lap["ci"], lap["val"])
    P = AmgParts(env, A, 1, "smoothed")
    want = MC.composed_pcg_multi(P.matvec, P.apply, P.dot, r, np.zeros((n, 1)), 1e-8, 1000)
    plan = S.KrylovMultiPlan(n, P.drp, P.dci, 1, precond=P.amg)
    X, st = plan.solve(P.dval, up(torch, cuda, r)[0], rtol=1e-8)
    assert_solved(st, X, dict(names=["only"], want=want))
    assert want[0].status == "converged" and 3 < want[0].iterations < 40
    # max_iter = 0: the limit at iteration 0 unless converged there; X untouched
    X0 = rng.standard_normal((n, 1))
    dX, = up(torch, cuda, X0)
    plan.start(P.dval, up(torch, cuda, r)[0], dX, rtol=1e-8, max_iter=0)
    plan.iterate(3)
    st = plan.status()
    assert st["status"] == ["limit"] and not st["iterations"].any() and same(dX.cpu().numpy(), X0)
    plan.destroy(), P.destroy()
    # s = 64, the widest: every column is apply() on it, and the one-shots converge and solve
    R = rng.standard_normal((n, 64)) * 10.0 ** rng.integers(-2, 3, 64)
    Z = amg.apply_multi(up(torch, cuda, R)[0]).cpu().numpy()
    assert amg.multi_info()["width"] == 64
    for j in (0, 7, 8, 31, 63):
        assert same(Z[:, j], amg.apply(up(torch, cuda, R[:, j])[0]).cpu().numpy()), j
    for solve, precond in ((S.pcg_multi, "amg_smoothed"), (S.bicgstab_multi, "amg")):
        X, st = solve((n, lap["drp"], lap["dci"], lap["dval"]), up(torch, cuda, R)[0], precond=precond, rtol=1e-8, check_every=4)
        assert st["status"] == ["converged"] * 64 and st["running"] == 0 and int(st["iterations"].max()) < 40
        x = X.cpu().numpy()
        for j in range(64):
            # |r| of the recurrence meets rtol |b|; the true residual differs from it by the rounding of a few dozen
            # iterations, far inside a factor 2
            res = np.linalg.norm(R[:, j] - KN.matvec(n, lap["rp"], lap["ci"], lap["val"], x[:, j]))
            assert st["rnorm"][j] <= 1e-8 * st["bnorm"][j] and res <= 2e-8 * np.linalg.norm(R[:, j]), (j, res)
    amg.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# 7. refusals, each before any launch
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(env, lap):
    S, torch, cuda = env
    E, L = S.SblasError, S.lib()
    n, s = lap["n"], 5
    drp, dci, dval = lap["drp"], lap["dci"], lap["dval"]
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=cuda)
    R = torch.ones((n, s), dtype=torch.float64, device=cuda)
    Z = torch.full((n, s), SENTINEL, dtype=torch.float64, device=cuda)
    amg = S.AmgPlan(n, drp, dci)
    apply_multi = lambda **k: L.sblas_hip_amg_plan_apply_multi(k.get("plan", amg.handle), None, k.get("s", s), k.get("R", R.data_ptr()), k.get("ldr", s),
                                                               k.get("Z", Z.data_ptr()), k.get("ldz", s))
    # a plan that is not set up
    assert apply_multi() == 1
    with pytest.raises(E, match="setup"):
        amg.apply_multi(R, out=Z)
    amg.setup(dval)
    # above the reserved width: the library says so by name; Python reserves on demand, except under capture
    assert amg.multi_info()["width"] == 0 and apply_multi() == 3             # SBLAS_E_WORKSPACE
    amg.reserve(s)
    assert apply_multi(s=s + 1, ldr=s + 1, ldz=s + 1) == 3
    for k in (dict(s=0), dict(s=65, ldr=65, ldz=65), dict(ldr=s - 1), dict(ldz=s - 1), dict(R=None), dict(Z=None), dict(R=R.data_ptr() + 4),
              dict(Z=Z.data_ptr() + 4), dict(Z=R.data_ptr()), dict(Z=R.data_ptr() + 8), dict(plan=None)):
        assert apply_multi(**k) == 1, k
    wide = z(n, 2 * s)
    for match, kw in (("columns", dict(R=z(n, 65))), ("tensor", dict(R=z(n))), ("tensor", dict(R=R, out=z(n, s + 1))),
                      ("tensor", dict(R=z(n + 1, s))), ("row-major", dict(R=z(s, n).t())), ("float64", dict(R=R.float())),
                      ("GPU tensor", dict(R=R.cpu())), ("overlap", dict(R=R, out=R)),
                      ("overlap", dict(R=wide[:, :s], out=wide[:, s:])),     # interleaved slices of one tensor: ranges overlap
                      ("row-major", dict(R=R, out=torch.as_strided(z(n * s), (n, s), (s - 1, 1))))):
        with pytest.raises(E, match=match):
            amg.apply_multi(**kw)
    with pytest.raises(E, match="columns"):
        amg.reserve(0)
    with pytest.raises(E, match="columns"):
        amg.reserve(65)
    assert L.sblas_hip_amg_plan_reserve_multi(amg.handle, None, 0) == 1 and L.sblas_hip_amg_plan_reserve_multi(amg.handle, None, 65) == 1
    assert L.sblas_hip_amg_plan_reserve_multi(None, None, 4) == 1
    # the single-kernel entries
    for k, args in (("sweep", (amg.handle, None, 0, 0, s, R.data_ptr(), s - 1, R.data_ptr(), s, Z.data_ptr(), s)),
                    ("sweep", (amg.handle, None, 0, 3, s, R.data_ptr(), s, R.data_ptr(), s, Z.data_ptr(), s)),
                    ("sweep", (amg.handle, None, 0, 0, s, R.data_ptr(), s, Z.data_ptr(), s, Z.data_ptr(), s)),
                    ("sweep", (amg.handle, None, 9, 0, s, R.data_ptr(), s, R.data_ptr(), s, Z.data_ptr(), s)),
                    ("sweep", (amg.handle, None, 0, 0, 65, R.data_ptr(), 65, R.data_ptr(), 65, Z.data_ptr(), 65))):
        assert L.sblas_hip_amg_sweep_multi_f64(*args) == 1, args
    assert L.sblas_hip_amg_restrict_multi_f64(amg.handle, None, 0, s, R.data_ptr(), s, R.data_ptr(), s) == 1
    assert L.sblas_hip_amg_prolong_multi_f64(amg.handle, None, 0, 1.0, s, R.data_ptr(), s - 1, Z.data_ptr(), s) == 1
    # reserve under a stream capture: an allocation
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    wider, wider_out = z(n, s + 2), z(n, s + 2)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            with pytest.raises(E, match="before capturing"):
                amg.reserve(s + 1)
            with pytest.raises(E, match="before capturing"):
                amg.apply_multi(wider, out=wider_out)
            rc_capturing = L.sblas_hip_amg_plan_reserve_multi(amg.handle, side.cuda_stream, s + 3)
            amg.apply_multi(R, out=Z, stream=side)                           # at the reserved width: capturable
    assert rc_capturing == 1 and amg.multi_info()["width"] == s
    torch.cuda.synchronize()
    assert bool((Z == SENTINEL).all()) and bool((R == 1.0).all())            # nothing ran
    # a Chebyshev-smoothed plan: at apply_multi and at start
    plan = S.KrylovMultiPlan(n, drp, dci, s, precond=amg)
    amg.setup(dval, smoother="chebyshev")
    assert apply_multi() == 1
    with pytest.raises(E, match="Chebyshev"):
        amg.apply_multi(R, out=Z)
    X = torch.full((n, s), SENTINEL, dtype=torch.float64, device=cuda)
    with pytest.raises(E, match="Chebyshev"):
        plan.start(dval, R, X)
    assert L.sblas_hip_krylov_multi_start(plan.handle, None, dval.data_ptr(), None, R.data_ptr(), s, X.data_ptr(), s, 1e-8, 0.0, 10) == 1
    with pytest.raises(E):
        plan.iterate(1)                                                      # not started
    torch.cuda.synchronize()
    assert bool((X == SENTINEL).all()) and bool((Z == SENTINEL).all())
    amg.setup(dval)
    plan.start(dval, R, X, dinv=None)                                        # no dinv; with the sweeps back it starts
    plan.destroy()
    # a plan that is not set up, at start
    raw = S.AmgPlan(n, drp, dci)
    plan = S.KrylovMultiPlan(n, drp, dci, s, precond=raw)
    with pytest.raises(E, match="setup"):
        plan.start(dval, R, X)
    assert L.sblas_hip_krylov_multi_start(plan.handle, None, dval.data_ptr(), None, R.data_ptr(), s, Z.data_ptr(), s, 1e-8, 0.0, 10) == 1
    plan.destroy(), raw.destroy()
    # an AmgPlan of another structure, at create
    drp2, dci2 = drp.clone(), dci.clone()
    other = S.AmgPlan(n, drp2, dci2)
    with pytest.raises(E, match="another structure"):
        S.KrylovMultiPlan(n, drp, dci, s, precond=other)
    h = C.c_void_p()
    create_ex = L.sblas_hip_krylov_multi_plan_create_ex
    base = (-1, None, 0, n, dci.numel(), drp.data_ptr(), dci.data_ptr(), s)
    assert create_ex(*base, S.PRECOND_AMG, other.handle, C.byref(h)) == 1 and not h.value
    assert create_ex(*base, S.PRECOND_AMG, None, C.byref(h)) == 1 and not h.value           # AMG without its plan
    assert create_ex(*base, S.PRECOND_NONE, amg.handle, C.byref(h)) == 1 and not h.value     # a plan where none belongs
    assert create_ex(*base, S.PRECOND_JACOBI, amg.handle, C.byref(h)) == 1 and not h.value
    for kind in (S.PRECOND_ILU0, S.PRECOND_CHEBYSHEV, 7, -1):
        assert create_ex(*base, kind, amg.handle, C.byref(h)) == 1 and not h.value
        assert create_ex(*base, kind, None, C.byref(h)) == 1 and not h.value
    assert create_ex(-1, None, 0, n, dci.numel(), drp.data_ptr(), dci.data_ptr(), 65, S.PRECOND_AMG, amg.handle, C.byref(h)) == 1
    # with NONE / JACOBI and no plan it is the old create
    assert create_ex(*base, S.PRECOND_JACOBI, None, C.byref(h)) == 0 and h.value
    info = (C.c_int64 * 12)()
    L.sblas_hip_krylov_multi_plan_info(h, info)
    assert (info[3], info[11]) == (S.PRECOND_JACOBI, 5)
    L.sblas_hip_krylov_multi_plan_destroy(h)
    # the ten-argument create has no plan argument and keeps refusing the applied kinds
    for kind in (S.PRECOND_ILU0, S.PRECOND_AMG, S.PRECOND_CHEBYSHEV):
        assert L.sblas_hip_krylov_multi_plan_create(*base, kind, C.byref(h)) == 1
    other.destroy()
    # the names, and the plans of the kinds without a block form, stay refused as they were
    ilu, cheb = S.Ilu0Plan(n, drp, dci), S.ChebyshevPlan(n, drp, dci)
    for precond, what in ((ilu, "ilu0"), (cheb, "chebyshev"), ("ilu0", "ilu0"), ("amg", "amg"), ("chebyshev", "chebyshev")):
        with pytest.raises(E, match="the %s preconditioner has no multi-column apply" % what):
            S.KrylovMultiPlan(n, drp, dci, s, precond=precond)
        with pytest.raises(E, match="the %s preconditioner has no multi-column apply" % what):
            S.krylov_multi_launches("pcg", precond)
    ilu.destroy(), cheb.destroy(), amg.destroy()
