"""The tiled triangular solve on the GPU (SptrsvPlan.solve_multi, Ilu0Plan.apply_multi) and ILU(0)'s seat under
KrylovMultiPlan as the pair ilu.solvers().

The contract is one sentence: column j of a block result has exactly the bits of the single-column entry on column j.  So
every comparison of values is == on bits against the EXISTING single-column entries (SptrsvPlan.solve on a 1-D b,
Ilu0Plan.apply on one column), which their own suites hold against the host restatements; a whole solve is == against
the lockstep loop of tests/multi_compose.py composed from an SpmmPlan of the test's own, krylov_dot per column and
Ilu0Plan.apply on one column.  Only "it solves" holds a tolerance: the factor 4 of test_gpu_krylov_multi.py on the true
residual of the same column's KrylovPlan + ILU(0) solve."""
import ctypes as C

import numpy as np
import pytest

import ilu0_numerics as IN
import krylov_numerics as KN
import multi_compose as MC
import sptrsv_numerics as TN

pytestmark = pytest.mark.gpu

RTOL = 1e-10
SENTINEL = -7.0
ALPHA = -1.5


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


def mirror(n, rp, ci):
    """the pattern turned over both diagonals, (i, c) -> (n - 1 - i, n - 1 - c), stored order kept inside a row: a lower
    builder's upper twin with the same levels and the same row lengths"""
    rp = np.asarray(rp, np.int64)
    return TN.csr_of_rows([[n - 1 - int(c) for c in ci[rp[i]:rp[i + 1]]] for i in range(n - 1, -1, -1)])


# name -> (n, rowptr, colidx) of the LOWER pattern, and whether the pattern already stores both triangles
def build(name):
    rng = np.random.default_rng(17)
    if name == "diagonal1":
        return TN.diagonal(1), False
    if name == "bidiagonal300":                                             # a 300-level chain
        return TN.bidiagonal(300), False
    if name == "grid5_24":
        return TN.grid5(24), False
    if name == "arrow200":                                                  # a 64-lane last row
        return TN.arrow(200), False
    if name == "row_lengths":                                               # every G boundary
        return TN.row_lengths_case([4, 5, 32, 33, 64, 65, 200]), False
    if name == "random_lower1500":                                          # duplicates
        return TN.random_lower(rng, 1500), False
    if name == "messy400":                                                  # unsorted, both triangles stored
        return TN.messy(rng, 400), True
    assert name == "staircase"                                              # wide and chain launches mixed
    return TN.staircase([300, 5, 300, 5]), False


BUILDERS = ["diagonal1", "bidiagonal300", "grid5_24", "arrow200", "row_lengths", "random_lower1500", "messy400", "staircase"]
MODES = [dict(), dict(chain_rows=4), dict(mode="per_level"), dict(mode="chain")]


# ---------------------------------------------------------------------------------------------------------------------
# 1. every column is the single solve on that column
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BUILDERS)
def test_columns_have_the_single_solves_bits(env, name):
    S, torch, cuda = env
    (rp_l, ci_l), both = build(name)
    n = len(rp_l) - 1
    widths = (1, 3, 8, 11) + ((64, 65) if name == "grid5_24" else ())
    smax = max(widths)
    rng = np.random.default_rng(29)
    for lower in (True, False):
        rp, ci = (rp_l, ci_l) if lower or both else mirror(n, rp_l, ci_l)
        drp, dci = up(torch, cuda, rp, ci)
        for unit in (False, True):
            val = TN.dominant_values(rng, n, rp, ci, lower, unit)
            hb = rng.standard_normal((n, smax)) * 10.0 ** rng.integers(-2, 3, smax)
            dval, = up(torch, cuda, val)
            plans = [S.SptrsvPlan(n, drp, dci, lower=lower, unit_diag=unit, **kw) for kw in MODES]
            # the references, once: the single solve on contiguous copies of the columns
            want = np.stack([plans[0].solve(dval, up(torch, cuda, hb[:, j])[0], alpha=ALPHA).cpu().numpy() for j in range(smax)], axis=1)
            assert np.isfinite(want).all()
            for k, plan in enumerate(plans):
                for s in widths:
                    for ld, offset in layouts(s):
                        what = (name, lower, unit, MODES[k], s, ld, offset)
                        gb = Guarded(torch, cuda, hb[:, :s], ld, offset)
                        gx = Guarded(torch, cuda, np.full((n, s), np.nan), ld, offset)   # an unwritten or ignored column read poisons
                        assert plan.solve_multi(dval, gb.view, X=gx.view, alpha=ALPHA) is gx.view
                        assert same(gx.host(), want[:, :s]), what
                        assert gx.intact() and gb.intact() and same(gb.host(), hb[:, :s]), what
                        assert plan.solve_multi(dval, gb.view, X=gb.view, alpha=ALPHA) is gb.view   # in place
                        assert same(gb.host(), want[:, :s]) and gb.intact(), what
                # operands of different layouts in one launch: B aligned at an even ld, X one element off
                s = 11
                gb, gx = Guarded(torch, cuda, hb[:, :s], s + 1, 0), Guarded(torch, cuda, np.full((n, s), np.nan), s, 1)
                plan.solve_multi(dval, gb.view, X=gx.view, alpha=ALPHA)
                assert same(gx.host(), want[:, :s]) and gx.intact(), (name, lower, unit, MODES[k])
            made = plans[0].solve_multi(dval, up(torch, cuda, hb)[0], alpha=ALPHA)       # X made here, alpha given
            assert tuple(made.shape) == (n, smax) and same(made.cpu().numpy(), want)
            one = plans[0].solve_multi(dval, up(torch, cuda, hb[:, :3])[0])              # alpha = 1, the default
            assert same(one.cpu().numpy()[:, 1], plans[0].solve(dval, up(torch, cuda, hb[:, 1])[0]).cpu().numpy())
            for plan in plans:
                plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# 2. no column can reach another column; the ignored triangle is invisible
# ---------------------------------------------------------------------------------------------------------------------
def test_columns_do_not_touch(env):
    S, torch, cuda = env
    rng = np.random.default_rng(41)
    rp, ci = TN.random_lower(rng, 1500)
    n, s = 1500, 11                                                         # a full tile and a ragged one
    val = TN.dominant_values(rng, n, rp, ci)
    drp, dci, dval = up(torch, cuda, rp, ci, val)
    B = rng.standard_normal((n, s))
    for kw in (dict(), dict(mode="chain")):
        plan = S.SptrsvPlan(n, drp, dci, **kw)
        X = plan.solve_multi(dval, up(torch, cuda, B)[0]).cpu().numpy()
        assert np.isfinite(X).all()
        for j, poison in ((4, np.nan), (9, np.inf), (0, -np.inf)):
            others = [c for c in range(s) if c != j]
            bad = B.copy()
            bad[:, j] = poison
            for layout in ((s, 0), (s + 3, 1)):
                got = plan.solve_multi(dval, Guarded(torch, cuda, bad, *layout).view).cpu().numpy()
                assert same(got[:, others], X[:, others]), (kw, j, poison, layout)
                assert not np.isfinite(got[:, j]).any()                     # its own column, nobody else's
            one = B.copy()                                                  # one poisoned ENTRY: still that column alone
            one[n // 2, j] = poison
            got = plan.solve_multi(dval, up(torch, cuda, one)[0]).cpu().numpy()
            assert same(got[:, others], X[:, others])
            assert same(got[:, j], plan.solve(dval, up(torch, cuda, one[:, j])[0]).cpu().numpy())
        plan.destroy()


@pytest.mark.parametrize("lower,unit", [(True, False), (False, False), (True, True), (False, True)])
def test_values_in_the_ignored_triangle_are_invisible(env, lower, unit):
    S, torch, cuda = env
    rng = np.random.default_rng(43)
    n, s = 400, 11
    rp, ci = TN.messy(rng, n)
    val = TN.dominant_values(rng, n, rp, ci, lower, unit)
    ignored = ~TN.selected(rp, ci, lower)
    if not unit:
        ignored &= ~TN.on_diagonal(rp, ci)
    assert ignored.sum() > 100
    drp, dci, dval = up(torch, cuda, rp, ci, val)
    B = rng.standard_normal((n, s))
    for kw in (dict(), dict(mode="chain"), dict(mode="per_level")):
        plan = S.SptrsvPlan(n, drp, dci, lower=lower, unit_diag=unit, **kw)
        X = plan.solve_multi(dval, up(torch, cuda, B)[0]).cpu().numpy()
        assert np.isfinite(X).all()
        for poison in (np.nan, np.inf):
            dbad, = up(torch, cuda, np.where(ignored, poison, val))
            for layout in ((s, 0), (s + 3, 1)):
                gx = Guarded(torch, cuda, np.full((n, s), np.nan), *layout)
                plan.solve_multi(dbad, Guarded(torch, cuda, B, *layout).view, X=gx.view)
                assert same(gx.host(), X) and gx.intact(), (kw, poison, layout)   # nothing at all changes
        plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# 3. capture
# ---------------------------------------------------------------------------------------------------------------------
def test_solve_multi_replays_in_a_graph_after_val_and_b_are_overwritten(env):
    S, torch, cuda = env
    rng = np.random.default_rng(47)
    rp, ci = TN.staircase([300, 5, 300, 5, 40])
    n, s = len(rp) - 1, 11
    drp, dci = up(torch, cuda, rp, ci)
    plan = S.SptrsvPlan(n, drp, dci, chain_rows=32)                         # both kinds of launch in the graph
    assert plan.info()["wide_launches"] and plan.info()["chain_launches"]
    dval, = up(torch, cuda, TN.dominant_values(rng, n, rp, ci))
    dB, = up(torch, cuda, rng.standard_normal((n, s)))
    dX = torch.zeros((n, s), dtype=torch.float64, device=cuda)
    plan.solve_multi(dval, dB, X=dX)                                        # eager first: loads the code objects
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):                              # a linear chain of launches
            plan.solve_multi(dval, dB, X=dX, alpha=ALPHA, stream=side)
    new_val, new_B = TN.dominant_values(rng, n, rp, ci), rng.standard_normal((n, s))
    dval.copy_(torch.from_numpy(new_val).to(cuda)), dB.copy_(torch.from_numpy(new_B).to(cuda))
    dX.fill_(SENTINEL)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    got = dX.cpu().numpy()
    assert same(got, plan.solve_multi(dval, dB, alpha=ALPHA).cpu().numpy())
    for j in (0, 7, 8, 10):
        assert same(got[:, j], plan.solve(dval, up(torch, cuda, new_B[:, j])[0], alpha=ALPHA).cpu().numpy()), j
    plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# 4. refusals and no-ops
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_and_no_ops(env):
    S, torch, cuda = env
    E, L = S.SblasError, S.lib()
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=cuda)
    # n = 0
    rp0, ci0 = torch.zeros(1, dtype=torch.int32, device=cuda), torch.zeros(0, dtype=torch.int32, device=cuda)
    empty = S.SptrsvPlan(0, rp0, ci0)
    assert tuple(empty.solve_multi(z(0), z(0, 3)).shape) == (0, 3)
    assert L.sblas_hip_sptrsm_tiled_f64_i32_planned(empty.handle, None, rp0.data_ptr(), None, None, 3, 1.0, None, 3, None, 3) == 0
    empty.destroy()
    rp, ci = TN.grid5(6)
    n, s = 36, 5
    drp, dci = up(torch, cuda, rp, ci)
    dval, = up(torch, cuda, TN.dominant_values(np.random.default_rng(3), n, rp, ci))
    plan = S.SptrsvPlan(n, drp, dci)
    # nrhs = 0: nothing is launched
    assert tuple(plan.solve_multi(dval, z(n, 0)).shape) == (n, 0)
    B = torch.ones((n, s), dtype=torch.float64, device=cuda)
    X = torch.full((n, s), SENTINEL, dtype=torch.float64, device=cuda)
    tiled = lambda **k: L.sblas_hip_sptrsm_tiled_f64_i32_planned(k.get("plan", plan.handle), None, k.get("rp", drp.data_ptr()), dci.data_ptr(),
                                                                 dval.data_ptr(), k.get("s", s), 1.0, k.get("B", B.data_ptr()), k.get("ldb", s),
                                                                 k.get("X", X.data_ptr()), k.get("ldx", s))
    assert tiled(s=0, B=None, X=None) == 0
    for k in (dict(ldb=s - 1), dict(ldx=s - 1), dict(s=-1), dict(B=None), dict(X=None), dict(plan=None), dict(rp=dci.data_ptr()),
              dict(B=B.data_ptr() + 4), dict(X=X.data_ptr() + 4)):
        assert tiled(**k) == 1, k
    for match, kw in (("leading dimension", dict(B=torch.as_strided(z(n * s), (n, s), (s - 1, 1)))),
                      ("leading dimension", dict(B=B, X=torch.as_strided(z(n * s), (n, s), (s - 1, 1)))),
                      ("row-major", dict(B=z(s, n).t())), ("row-major", dict(B=B, X=z(s, n).t())),
                      ("float64", dict(B=B.float())), ("float64", dict(B=B, X=X.float())), ("float64", dict(val=dval.float(), B=B)),
                      ("GPU tensor", dict(B=B.cpu())), ("GPU tensor", dict(B=B, X=X.cpu())),
                      ("shape", dict(B=B, X=z(n, s + 1))), ("nrhs", dict(B=z(n + 1, s))), ("nrhs", dict(B=z(n))),
                      ("one value per stored entry", dict(val=dval[:-1], B=B))):
        with pytest.raises(E, match=match):
            plan.solve_multi(kw.pop("val", dval), **kw)
    torch.cuda.synchronize()
    assert bool((X == SENTINEL).all()) and bool((B == 1.0).all())            # nothing ran
    plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# 5. ILU(0): apply_multi is apply on every column
# ---------------------------------------------------------------------------------------------------------------------
def ilu_cases():
    n, rp, ci, val = KN.laplacian(32)
    yield "laplacian32", n, rp, ci, val
    rng = np.random.default_rng(53)
    rp, ci = IN.random_near_diagonal(rng, 700, 6, 40)
    yield "random_near_diagonal", 700, rp, ci, IN.dominant_values(rng, 700, rp, ci)


def test_ilu0_apply_multi_is_apply_on_every_column(env):
    S, torch, cuda = env
    rng = np.random.default_rng(59)
    for name, n, rp, ci, val in ilu_cases():
        drp, dci, dval = up(torch, cuda, rp.astype(np.int32), ci.astype(np.int32), val)
        ilu = S.Ilu0Plan(n, drp, dci)
        lu = ilu.factor(dval)
        for s in (5, 9):
            R = rng.standard_normal((n, s))
            R[:, 2] = 0.0                                                   # M^-1 0 = 0
            want = np.stack([ilu.apply(lu, up(torch, cuda, R[:, j])[0]).cpu().numpy() for j in range(s)], axis=1)
            assert not want[:, 2].any() and np.isfinite(want).all()
            dR, = up(torch, cuda, R)
            for _ in range(2):
                Z = ilu.apply_multi(lu, dR)
                assert tuple(Z.shape) == (n, s) and same(Z.cpu().numpy(), want), (name, s)
            assert same(dR.cpu().numpy(), R)
            for ld, offset in layouts(s):
                gR, gZ = Guarded(torch, cuda, R, ld, offset), Guarded(torch, cuda, np.full((n, s), np.nan), s + 2, offset)
                assert ilu.apply_multi(lu, gR.view, out=gZ.view) is gZ.view
                assert same(gZ.host(), want) and gZ.intact() and gR.intact() and same(gR.host(), R), (name, s, ld, offset)
        ilu.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the solvers with the pair seated against their own composition
# ---------------------------------------------------------------------------------------------------------------------
class PairParts:
    """the device's parts of a lockstep loop: A V by an SpmmPlan of the test's own for width s, called row-major; the
    pinned dot per column; M^-1 by Ilu0Plan.apply on ONE column"""

    def __init__(self, env, A, s):
        S, torch, cuda = self.env = env
        self.n, self.rp, self.ci, self.val = A[0], A[1].astype(np.int32), A[2].astype(np.int32), A[3]
        self.s = s
        self.drp, self.dci, self.dval = up(torch, cuda, self.rp, self.ci, self.val)
        self.spmm = S.SpmmPlan(self.n, self.n, self.drp, self.dci, s)
        self.ws = torch.empty(max(S.spmm_workspace_bytes(self.n, self.n, len(self.ci), s) // 8, 1), dtype=torch.float64, device=cuda)
        self.ilu = S.Ilu0Plan(self.n, self.drp, self.dci)
        self.lu = self.ilu.factor(self.dval)
        self.pair = self.ilu.solvers()

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
        return self.ilu.apply(self.lu, up(torch, cuda, v)[0]).cpu().numpy()

    def destroy(self):
        self.spmm.destroy(), self.ilu.destroy()


MATRICES = {"pcg": lambda: KN.laplacian(32), "bicgstab": lambda: KN.convection_diffusion(24)}
METHODS = ["pcg", "bicgstab"]


@pytest.fixture(scope="module")
def composed(env):
    """the composed loop of every case, run once and shared by the tests that compare against it"""
    made = {}

    def get(method):
        if method not in made:
            A = MATRICES[method]()
            B, X0, names = MC.columns(A[0], lambda v: KN.matvec(*A, v))
            P = PairParts(env, A, B.shape[1])
            loop = MC.composed_pcg_multi if method == "pcg" else MC.composed_bicgstab_multi
            want = loop(P.matvec, P.apply, P.dot, B, X0, RTOL, 1000)
            for w in want:
                w.x.setflags(write=False)
            made[method] = dict(A=A, B=B, X0=X0, names=names, P=P, want=want)
        return made[method]
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
@pytest.mark.parametrize("method", METHODS)
def test_the_solver_with_the_pair_equals_its_own_composition(env, composed, method, check_every):
    S, torch, cuda = env
    c = composed(method)
    P, n, s = c["P"], c["A"][0], c["B"].shape[1]
    assert s == 9
    by = dict(zip(c["names"], c["want"]))
    assert by["nan"].status != "converged"                                   # a NaN never converges
    assert all(w.status == "converged" for k, w in by.items() if k != "nan")  # every other column does
    assert (by["zero"].iterations, by["zero"].x.any()) == (0, False)
    plan = S.KrylovMultiPlan(n, P.drp, P.dci, s, method=method, precond=P.pair)
    dB = Guarded(torch, cuda, c["B"]).view
    gX = Guarded(torch, cuda, c["X0"], s + 3, 1)                            # X: a slice of a wider tensor
    X, st = plan.solve(P.dval, dB, X=gX.view, lu=P.lu, rtol=RTOL, max_iter=1000, check_every=check_every)
    assert X is gX.view
    if check_every == 7:
        print("%s with ILU(0) seated: iterations %s" % (method, dict(zip(c["names"], st["iterations"].tolist()))))
    assert_solved(st, X, c)
    assert gX.intact()
    info = plan.info()
    lo, hi = (q.info()["launches"] for q in P.pair)
    assert (info["n"], info["nrhs"], info["method"], info["precond"]) == (n, s, method, "ilu0")
    assert info["launches"] == S.krylov_multi_launches(method, P.pair, 0) == (7 + lo + hi if method == "pcg" else 8 + 2 * (lo + hi))
    # a second solve on the same plan has the same bits, X contiguous this time
    X2, st2 = plan.solve(P.dval, dB, X=Guarded(torch, cuda, c["X0"]).view, lu=P.lu, rtol=RTOL, max_iter=1000, check_every=check_every)
    assert_solved(st2, X2, c)
    plan.destroy()


@pytest.mark.parametrize("method", METHODS)
def test_iterate_with_the_pair_replays_in_a_graph(env, composed, method):
    S, torch, cuda = env
    c = composed(method)
    P, n, s = c["P"], c["A"][0], c["B"].shape[1]
    plan = S.KrylovMultiPlan(n, P.drp, P.dci, s, method=method, precond=P.pair)
    dB, dX = Guarded(torch, cuda, c["B"]).view, Guarded(torch, cuda, c["X0"], s + 3, 1).view
    ex, est = plan.solve(P.dval, dB, X=dX.clone(), lu=P.lu, rtol=RTOL, check_every=9)   # eager: loads the code objects
    assert_solved(est, ex, c)
    plan.start(P.dval, dB, dX, lu=P.lu, rtol=RTOL)                           # start runs eagerly
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):                              # a linear chain of launches
            plan.iterate(9)
    st = plan.status()
    assert int(st["iterations"].max()) == 0                                  # capturing ran nothing
    most = max(w.iterations for w in c["want"])
    for replay in range(1, 200):
        g.replay()
        st = plan.status()
        if st["running"] == 0:
            break
    assert replay == -(-most // 9), (replay, most)
    assert_solved(st, dX, c)
    plan.destroy()


@pytest.mark.parametrize("method", METHODS)
def test_it_solves_as_well_as_the_single_solver(env, composed, method):
    """Each converged column's true residual |b_j - A x_j| (float64, on the host) against the same column's KrylovPlan
    solve with the same factor: within the factor 4 of test_gpu_krylov_multi.py.  The two differ in the product alone
    (the SpMM's row sums against the SpMV's); M^-1 has the same bits on both sides."""
    S, torch, cuda = env
    c = composed(method)
    P, n, s = c["P"], c["A"][0], c["B"].shape[1]
    B, X0 = c["B"], c["X0"]
    multi = S.KrylovMultiPlan(n, P.drp, P.dci, s, method=method, precond=P.pair)
    X, st = multi.solve(P.dval, Guarded(torch, cuda, B).view, X=Guarded(torch, cuda, X0).view, lu=P.lu, rtol=RTOL)
    x = X.cpu().numpy()
    single = S.KrylovPlan(n, P.drp, P.dci, method=method, precond=P.pair)
    true = lambda b, v: float(np.linalg.norm(b - KN.matvec(n, P.rp, P.ci, P.val, v)))
    ratios, counts = {}, {}
    for j, name in enumerate(c["names"]):
        db, dx = up(torch, cuda, B[:, j], X0[:, j])
        xs, sst = single.solve(P.dval, db, x=dx, lu=P.lu, rtol=RTOL)
        assert st["status"][j] == sst["status"], (name, st["status"][j], sst)
        if sst["status"] != "converged":
            assert name == "nan"
            continue
        mine, theirs = true(B[:, j], x[:, j]), true(B[:, j], xs.cpu().numpy())
        ratios[name] = mine / theirs if theirs > 0.0 else (1.0 if mine == 0.0 else np.inf)
        counts[name] = (int(st["iterations"][j]), sst["iterations"])
        assert mine <= 4.0 * theirs, (name, mine, theirs)
    print("%s with ILU(0) seated: true residual over the single solver's: %s" % (method, {k: "%.6g" % v for k, v in ratios.items()}))
    print("    iterations (batched, single): %s" % counts)
    assert len(ratios) == s - 1
    single.destroy(), multi.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the seat's refusals, each before any launch
# ---------------------------------------------------------------------------------------------------------------------
def test_seat_refusals(env):
    S, torch, cuda = env
    E, L = S.SblasError, S.lib()
    n, rp, ci, val = KN.laplacian(12)
    drp, dci, dval = up(torch, cuda, rp.astype(np.int32), ci.astype(np.int32), val)
    s = 5
    ilu = S.Ilu0Plan(n, drp, dci)
    lu = ilu.factor(dval)
    lower, upper = ilu.solvers()
    h = C.c_void_p()
    create = lambda lo, hi, rp_=drp, ci_=dci, nrhs=s, method=0: L.sblas_hip_krylov_multi_plan_create_pair(
        -1, None, method, n, dci.numel(), rp_.data_ptr(), ci_.data_ptr(), nrhs, lo, hi, C.byref(h))
    # the pair swapped
    with pytest.raises(E, match="pair must be"):
        S.KrylovMultiPlan(n, drp, dci, s, precond=(upper, lower))
    assert create(upper.handle, lower.handle) == 1 and not h.value
    # a pair made on cloned structure tensors
    drp2, dci2 = drp.clone(), dci.clone()
    other = (S.SptrsvPlan(n, drp2, dci2, lower=True, unit_diag=True), S.SptrsvPlan(n, drp2, dci2, lower=False))
    with pytest.raises(E, match="another structure"):
        S.KrylovMultiPlan(n, drp, dci, s, precond=other)
    assert create(other[0].handle, other[1].handle) == 1 and not h.value
    assert create(lower.handle, other[1].handle) == 1 and not h.value
    # a unit or non-unit mismatch
    nonunit, unit_upper = S.SptrsvPlan(n, drp, dci, lower=True, unit_diag=False), S.SptrsvPlan(n, drp, dci, lower=False, unit_diag=True)
    for pair in ((nonunit, upper), (lower, unit_upper), (lower, lower), (upper, upper)):
        with pytest.raises(E, match="pair must be"):
            S.KrylovMultiPlan(n, drp, dci, s, precond=pair)
        assert create(pair[0].handle, pair[1].handle) == 1 and not h.value
    # the C create with a NULL plan, a bad method, a bad width
    assert create(None, upper.handle) == 1 and create(lower.handle, None) == 1 and create(None, None) == 1 and not h.value
    assert create(lower.handle, upper.handle, method=2) == 1 and create(lower.handle, upper.handle, nrhs=0) == 1
    assert create(lower.handle, upper.handle, nrhs=65) == 1 and not h.value
    assert L.sblas_hip_krylov_multi_plan_create_pair(-1, None, 0, n, dci.numel(), drp.data_ptr(), dci.data_ptr(), s, lower.handle, upper.handle, None) == 1
    # the older creates keep refusing ILU(0), with or without a plan
    base = (-1, None, 0, n, dci.numel(), drp.data_ptr(), dci.data_ptr(), s)
    assert L.sblas_hip_krylov_multi_plan_create(*base, S.PRECOND_ILU0, C.byref(h)) == 1
    assert L.sblas_hip_krylov_multi_plan_create_ex(*base, S.PRECOND_ILU0, lower.handle, C.byref(h)) == 1 and not h.value
    # lu = None at start
    plan = S.KrylovMultiPlan(n, drp, dci, s, precond=(lower, upper))
    B = torch.ones((n, s), dtype=torch.float64, device=cuda)
    X = torch.full((n, s), SENTINEL, dtype=torch.float64, device=cuda)
    with pytest.raises(E, match="needs lu"):
        plan.start(dval, B, X)
    with pytest.raises(E, match="needs lu"):
        plan.start(dval, B, X, dinv=lu)                                      # the factor has its own word
    with pytest.raises(E):
        plan.start(dval, B, X, lu=lu[:-1])
    assert L.sblas_hip_krylov_multi_start(plan.handle, None, dval.data_ptr(), None, B.data_ptr(), s, X.data_ptr(), s, 1e-8, 0.0, 10) == 1
    with pytest.raises(E):
        plan.iterate(1)                                                      # not started
    torch.cuda.synchronize()
    assert bool((X == SENTINEL).all())
    X.zero_()
    plan.start(dval, B, X, lu=lu)                                            # with the factor it starts
    plan.iterate(1)
    assert plan.status()["iterations"].max() == 1
    plan.destroy()
    # the names and the Ilu0Plan instance stay refused as they were, pointing at the pair; the one-shots take no pair
    for precond in (ilu, "ilu0"):
        with pytest.raises(E, match="the ilu0 preconditioner has no multi-column apply"):
            S.KrylovMultiPlan(n, drp, dci, s, precond=precond)
        with pytest.raises(E, match="the ilu0 preconditioner has no multi-column apply"):
            S.krylov_multi_launches("pcg", precond)
        with pytest.raises(E, match="the ilu0 preconditioner has no multi-column apply"):
            S.pcg_multi((n, drp, dci, dval), B, precond=precond)
    with pytest.raises(E, match="one-shots take no pair"):
        S.bicgstab_multi((n, drp, dci, dval), B, precond=(lower, upper))
    for q in other + (nonunit, unit_upper):
        q.destroy()
    ilu.destroy()
