"""The multi-right-hand-side Krylov solvers on the GPU (KrylovMultiPlan, krylov_multi_dots, krylov_multi_update, pcg_multi,
bicgstab_multi) against tests/multi_compose.py and tests/krylov_numerics.py.

Every bit is pinned, so most checks are ==: a column's dot against sblas_krylov_dot_ref on that column, each fused update
against numpy's expression of the same shape with the column's own scalars, and a whole solve against the lockstep loop
composed from an SpmmPlan of the test's own, krylov_dot per column and numpy updates.  Only "it solves" holds a
tolerance: a factor 4 on the true residual of the same column's single-right-hand-side solve (both stop at the same test,
possibly an iteration apart, and CG's residual is not monotone)."""
import numpy as np
import pytest

import krylov_numerics as KN
import multi_compose as MC
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


def block(torch, cuda, host, ld=None, offset=0, fill=0.0):
    """host (n, s) as a device block at leading dimension ld, its first element `offset` elements into an allocation"""
    n, s = host.shape
    ld = s if ld is None else ld
    buf = torch.full((offset + n * ld + 1,), fill, dtype=torch.float64, device=cuda)
    view = buf[offset:offset + n * ld].view(n, ld)[:, :s]
    view.copy_(torch.from_numpy(np.ascontiguousarray(host)).to(cuda))
    return view


# ---------------------------------------------------------------------------------------------------------------------
# the multi-dot
# ---------------------------------------------------------------------------------------------------------------------
S_MAX = 11


@pytest.fixture(scope="module")
def dot_columns(sblas):
    """per n: eleven "mixed" column pairs and their reference dots, made once and shared by every width and layout"""
    made = {}

    def get(n):
        if n not in made:
            cols = [KN.vectors("mixed", n, seed=j + 1) for j in range(S_MAX)]
            X, Y = np.stack([c[0] for c in cols], axis=1), np.stack([c[1] for c in cols], axis=1)
            ref = dict(xy=[sblas.krylov_dot_ref(X[:, j], Y[:, j]) for j in range(S_MAX)],
                       xx=[sblas.krylov_dot_ref(X[:, j], X[:, j]) for j in range(S_MAX)],
                       yy=[sblas.krylov_dot_ref(Y[:, j], Y[:, j]) for j in range(S_MAX)])
            made[n] = (X, Y, ref)
        return made[n]
    return get


@pytest.mark.parametrize("n", [1, 255, 257, CELL + 1, 3 * CELL + 5, KN.WIDTH * CELL + 3])
def test_every_columns_dot_has_the_reference_bits(env, dot_columns, n):
    S, torch, cuda = env
    X, Y, ref = dot_columns(n)
    for s in (1, 3, 8, 11):
        for ld in (s, s + 3):
            for offset in (0, 1):                                            # 0 with an even ld: the 16-byte path; 1: never
                dx = block(torch, cuda, X[:, :s], ld, offset)
                dy = block(torch, cuda, Y[:, :s], ld, offset)
                got = S.krylov_multi_dots([(dx, dy)]).cpu().numpy()
                assert got.shape == (1, s) and same(got[0], ref["xy"][:s]), (n, s, ld, offset, got[0], ref["xy"][:s])
        # two and three dots in one pass have the single dot's bits; operands of different layouts in one call
        dx, dy = block(torch, cuda, X[:, :s], s + 3, 1), block(torch, cuda, Y[:, :s])
        two = S.krylov_multi_dots([(dx, dy), (dy, dy)]).cpu().numpy()
        assert same(two, [ref["xy"][:s], ref["yy"][:s]]), (n, s)
        dx = block(torch, cuda, X[:, :s], s + (s % 2), 0)                    # an even ld from an aligned base
        three = S.krylov_multi_dots([(dy, dx), (dx, dx), (dy, dy)]).cpu().numpy()
        assert same(three, [ref["xy"][:s], ref["xx"][:s], ref["yy"][:s]]), (n, s)


def test_dot_on_a_side_stream_with_its_own_workspace_and_its_refusals(env, dot_columns):
    S, torch, cuda = env
    n, s = 3 * CELL + 5, 11
    X, Y, ref = dot_columns(n)
    dx, dy = block(torch, cuda, X), block(torch, cuda, Y, s + 1)
    out = torch.empty((2, s), dtype=torch.float64, device=cuda)
    cells = -(-n // CELL)
    ws = torch.full((2 * s * cells,), -7.0, dtype=torch.float64, device=cuda)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        assert S.krylov_multi_dots([(dx, dy), (dx, dx)], out=out, workspace=ws) is out
    st.synchronize()
    assert same(out.cpu().numpy(), [ref["xy"], ref["xx"]])
    # the first stage's layout: dot k, column j, cell c at ws[(k * s + j) * cells + c], each a single dot's cell sum
    w = ws.cpu().numpy().reshape(2, s, cells)
    for j in (0, 7, 8, 10):
        wj = torch.zeros(cells, dtype=torch.float64, device=cuda)
        S.krylov_dot(*up(torch, cuda, X[:, j], Y[:, j]), workspace=wj)
        assert same(w[0, j], wj.cpu().numpy()), j
    E = S.SblasError
    with pytest.raises(E):
        S.krylov_multi_dots([(dx, dy)] * 4)
    with pytest.raises(E, match="tensor"):
        S.krylov_multi_dots([(dx, dy[:, :-1])])
    with pytest.raises(E, match="float64"):
        S.krylov_multi_dots([(dx, dy.float())])
    with pytest.raises(E, match="row-major"):
        S.krylov_multi_dots([(dx, dy.t().contiguous().t())])                 # column-major
    with pytest.raises(E, match="right-hand sides"):
        S.krylov_multi_dots([(torch.zeros(4, 65, dtype=torch.float64, device=cuda),) * 2])
    with pytest.raises(E):
        S.krylov_multi_dots([(dx, dy)], workspace=torch.empty(s * cells - 1, dtype=torch.float64, device=cuda))   # short: refused, not overrun
    L = S.lib()
    import ctypes as C
    ptr, ld = (C.c_void_p * 1)(dx.data_ptr()), (C.c_int64 * 1)(s - 1)
    good = (C.c_int64 * 1)(s)
    big = torch.empty(s * cells, dtype=torch.float64, device=cuda)
    assert L.sblas_hip_krylov_multi_dot_f64(-1, None, n, s, 1, ptr, ld, ptr, good, out.data_ptr(), big.data_ptr(), big.numel() * 8) == 1
    assert L.sblas_hip_krylov_multi_dot_f64(-1, None, n, 65, 1, ptr, good, ptr, good, out.data_ptr(), big.data_ptr(), big.numel() * 8) == 1
    assert L.sblas_hip_krylov_multi_dot_f64(-1, None, n, s, 1, ptr, good, ptr, good, out.data_ptr(), big.data_ptr(), 8) == 3


# ---------------------------------------------------------------------------------------------------------------------
# the fused updates
# ---------------------------------------------------------------------------------------------------------------------
def stage1(S, torch, cuda, a, b):
    """the cells' sums of every column of (a, b) as the multi-dot's own first stage leaves them: (s, cells)"""
    n, s = a.shape
    cells = -(-n // CELL)
    ws = torch.zeros(s * cells, dtype=torch.float64, device=cuda)
    S.krylov_multi_dots([(a, b)], workspace=ws)
    return ws.cpu().numpy().reshape(s, cells)


def frozen_columns(s, pattern):
    j = np.arange(s)
    if pattern == "none":
        return np.zeros(s, bool)
    if pattern == "some":
        return j % 3 == 1
    return j >= 8 if s > 8 else j == 0                                       # "tile": a whole tile frozen (s = 11), else the first column


@pytest.mark.parametrize("pattern", ["none", "some", "tile"])
@pytest.mark.parametrize("s", [3, 8, 11])
@pytest.mark.parametrize("n", [1, 257, CELL + 1, 3 * CELL + 5])
def test_fused_updates_column_by_column(env, n, s, pattern):
    S, torch, cuda = env
    rng = np.random.default_rng(1000 * n + 10 * s + len(pattern))
    cells = -(-n // CELL)
    frozen = frozen_columns(s, pattern)
    live = ~frozen
    scal = np.zeros((s, 16))
    alpha, beta, omega = (rng.standard_normal(s) for _ in range(3))          # every column its own
    scal[:, 4], scal[:, 5], scal[:, 6] = alpha, beta, omega
    scal.view(np.int64)[:, 0] = np.where(frozen, rng.integers(1, 4, s), 0)   # converged / breakdown / limit: all frozen
    dscal, = up(torch, cuda, scal)
    vec = lambda: rng.standard_normal((n, s)) * 10.0 ** rng.integers(-3, 4, (n, s))

    def out_block(host):
        """an in / out block: the frozen columns hold the sentinel"""
        h = host.copy()
        h[:, frozen] = -7.0
        return h

    def check(name, got, want):
        g = got.cpu().numpy()
        assert same(g[:, live], want[:, live]), (name, n, s, pattern)
        assert (g[:, frozen] == -7.0).all(), (name, n, s, pattern, "a frozen column was written")

    def check_partial(pt, k, a, b):
        g = pt.cpu().numpy()[k * s * cells:(k + 1) * s * cells].reshape(s, cells)
        assert same(g[live], stage1(S, torch, cuda, a, b)[live]), (n, s, pattern, k)
        assert (g[frozen] == -7.0).all()

    part = lambda: torch.full((2 * s * cells,), -7.0, dtype=torch.float64, device=cuda)
    sentinel = lambda: np.full((n, s), -7.0)
    dinv = rng.standard_normal(n) * 10.0 ** rng.integers(-2, 3, n)
    ddinv, = up(torch, cuda, dinv)
    for jac in (False, True):
        for ld, offset in ((s, 0), (s + 3, 1), (s + (s % 2), 0)):            # the last: the 16-byte path where the tile allows it
            B = lambda host: block(torch, cuda, host, ld, offset, fill=-7.0)
            # PCG: x = x + alpha p, r = r - alpha q [, z = dinv r]
            x, r, p, q = out_block(vec()), out_block(vec()), vec(), vec()
            d = [B(x), B(r), B(p), B(q), ddinv, B(sentinel())]
            pt = part()
            S.krylov_multi_update("pcg_xr", dscal, d if jac else d[:4], partial=pt, jacobi=jac)
            r1 = r - alpha * q
            check("pcg x", d[0], x + alpha * p), check("pcg r", d[1], r1)
            check_partial(pt, 0, d[1], d[1])
            if jac:
                check("pcg z", d[5], dinv[:, None] * r1)
                check_partial(pt, 1, d[1], d[5])
            else:
                assert bool((d[5] == -7.0).all()) and bool((pt[s * cells:] == -7.0).all())
            # BiCGStab: p = r + beta (p - omega v) [, p^ = dinv p];  s = r - alpha v [, s^ = dinv s]
            p, r, v = out_block(vec()), vec(), vec()
            d = [B(p), B(r), B(v), ddinv, B(sentinel())]
            S.krylov_multi_update("bicg_p", dscal, d if jac else d[:3], jacobi=jac)
            p1 = r + beta * (p - omega * v)
            check("bicg p", d[0], p1)
            if jac:
                check("bicg p^", d[4], dinv[:, None] * p1)
            else:
                assert bool((d[4] == -7.0).all())
            d = [B(sentinel()), B(r), B(v), ddinv, B(sentinel())]
            S.krylov_multi_update("bicg_s", dscal, d if jac else d[:3], jacobi=jac)
            s1 = r - alpha * v
            check("bicg s", d[0], s1)
            if jac:
                check("bicg s^", d[4], dinv[:, None] * s1)
            else:
                assert bool((d[4] == -7.0).all())
    for ld, offset in ((s, 0), (s + 3, 1), (s + (s % 2), 0)):
        B = lambda host: block(torch, cuda, host, ld, offset, fill=-7.0)
        # PCG: p = z + beta p
        p, z = out_block(vec()), vec()
        d = [B(p), B(z)]
        S.krylov_multi_update("pcg_p", dscal, d)
        check("pcg p", d[0], z + beta * p)
        # BiCGStab: x = (x + alpha p^) + omega s^, r = s - omega t, with (r, r) and (r^, r)
        x, ph, sh, sv, t, rh = out_block(vec()), vec(), vec(), vec(), vec(), vec()
        d = [B(x), B(sentinel()), B(ph), B(sh), B(sv), B(t), B(rh)]
        pt = part()
        S.krylov_multi_update("bicg_xr", dscal, d, partial=pt)
        check("bicg x", d[0], (x + alpha * ph) + omega * sh), check("bicg r", d[1], sv - omega * t)
        check_partial(pt, 0, d[1], d[1]), check_partial(pt, 1, d[6], d[1])
    # the bytes around the blocks (the padding of a wider leading dimension, the element before an offset base) are untouched
    probe = torch.full((1 + n * (s + 3) + 1,), -7.0, dtype=torch.float64, device=cuda)
    pv = probe[1:1 + n * (s + 3)].view(n, s + 3)
    pv[:, :s].copy_(torch.from_numpy(vec()).to(cuda))
    S.krylov_multi_update("pcg_p", dscal, [pv[:, :s], block(torch, cuda, vec())])
    assert bool((pv[:, s:] == -7.0).all()) and float(probe[0]) == -7.0 and float(probe[-1]) == -7.0


def test_update_refusals(env):
    S, torch, cuda = env
    E = S.SblasError
    n, s = 300, 5
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=cuda)
    scal = z(s, 16)
    with pytest.raises(E, match="x 16 slots"):
        S.krylov_multi_update("pcg_p", z(s - 1, 16), [z(n, s), z(n, s)])
    with pytest.raises(E, match="tensor"):
        S.krylov_multi_update("pcg_p", scal, [z(n, s), z(n, s + 1)])
    with pytest.raises(E, match="dinv"):
        S.krylov_multi_update("bicg_s", scal, [z(n, s), z(n, s), z(n, s), z(n, s), z(n, s)], jacobi=True)   # dinv is a vector
    with pytest.raises(E, match="too short"):
        S.krylov_multi_update("pcg_xr", scal, [z(n, s)] * 4, partial=z(s))
    with pytest.raises(E):
        S.krylov_multi_update("pcg_xr", scal, [z(n, s)] * 3, partial=z(2 * s))                             # an operand short
    with pytest.raises(E):
        S.krylov_multi_update("pcg_xr", scal, [z(n, s)] * 4)                                               # no partial


# ---------------------------------------------------------------------------------------------------------------------
# the solver equals its own composition
# ---------------------------------------------------------------------------------------------------------------------
class MultiParts:
    """the device's parts of a lockstep loop: A V by an SpmmPlan of the test's own for width s, called row-major; the
    pinned dot per column; M^-1 by a numpy product with dinv"""

    def __init__(self, env, A, s, jacobi):
        S, torch, cuda = self.env = env
        self.n, self.rp, self.ci, self.val = A
        self.s = s
        self.drp, self.dci, self.dval = up(torch, cuda, self.rp, self.ci, self.val)
        self.spmm = S.SpmmPlan(self.n, self.n, self.drp, self.dci, s)
        self.ws = torch.empty(max(S.spmm_workspace_bytes(self.n, self.n, len(self.ci), s) // 8, 1), dtype=torch.float64, device=cuda)
        self.dinv = 1.0 / self.val[SC.stored_diagonal(self.rp, self.ci)] if jacobi else None
        self.ddinv = up(torch, cuda, self.dinv)[0] if jacobi else None

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
        return self.dinv * v if self.dinv is not None else v

    def destroy(self):
        self.spmm.destroy()


MATRICES = {"pcg": lambda: KN.spd_perturbed(48), "bicgstab": lambda: KN.convection_diffusion(48)}
# (method, Jacobi, layout): "slice" is all nine columns with X a column slice of a wider tensor (no 16-byte path anywhere);
# "aligned" is eight of them, contiguous: one full tile that takes the 16-byte path at start, the predicated one later
SOLVES = [("pcg", False, "slice"), ("pcg", True, "slice"), ("pcg", True, "aligned"), ("bicgstab", False, "slice"),
          ("bicgstab", True, "aligned")]


@pytest.fixture(scope="module")
def composed(env):
    """the composed loop of every case, run once and shared by the tests that compare against it"""
    made = {}

    def get(method, jacobi, layout):
        key = (method, jacobi, layout)
        if key not in made:
            A = MATRICES[method]()
            n = A[0]
            B, X0, names = MC.columns(n, lambda v: KN.matvec(*A, v))
            if layout == "aligned":                                          # one full tile: every kind of column but "large"
                keep = [j for j, name in enumerate(names) if name != "large"]
                B, X0, names = np.ascontiguousarray(B[:, keep]), np.ascontiguousarray(X0[:, keep]), [names[j] for j in keep]
            P = MultiParts(env, A, B.shape[1], jacobi)
            loop = MC.composed_pcg_multi if method == "pcg" else MC.composed_bicgstab_multi
            want = loop(P.matvec, P.apply, P.dot, B, X0, RTOL, 1000)
            for w in want:
                w.x.setflags(write=False)
            made[key] = dict(A=A, B=B, X0=X0, names=names, P=P, want=want)
        return made[key]
    yield get
    for c in made.values():
        c["P"].destroy()


def device_blocks(torch, cuda, c, layout):
    B, X0 = c["B"], c["X0"]
    if layout == "aligned":
        return block(torch, cuda, B), block(torch, cuda, X0)
    s = B.shape[1]
    return block(torch, cuda, B), block(torch, cuda, X0, s + 3, 1, fill=-7.0)  # X: a slice of a wider tensor


def assert_solved(S, st, X, c):
    x = X.cpu().numpy()
    for j, (name, w) in enumerate(zip(c["names"], c["want"])):
        got = dict(status=st["status"][j], iterations=int(st["iterations"][j]), breakdown=st["breakdown"][j])
        assert got == dict(status=w.status, iterations=w.iterations, breakdown=w.breakdown), (name, got, w.asdict())
        for key in ("rnorm", "bnorm", "alpha", "beta", "omega"):
            assert same(st[key][j], getattr(w, key)), (name, key, st[key][j], getattr(w, key))
        assert same(x[:, j], w.x), (name, "x")
    assert st["running"] == 0


@pytest.mark.parametrize("check_every", [1, 7, 50])
@pytest.mark.parametrize("method,jacobi,layout", SOLVES)
def test_the_solver_equals_its_own_composition(env, composed, method, jacobi, layout, check_every):
    S, torch, cuda = env
    c = composed(method, jacobi, layout)
    P, n, s = c["P"], c["A"][0], c["B"].shape[1]
    by = dict(zip(c["names"], c["want"]))
    # the cases are worth having: the NaN column breaks down while the others converge, and the stops are spread out
    assert (by["nan"].status, by["nan"].iterations) == ("breakdown", 0)
    assert by["nan"].breakdown == (SC.DENOM_PQ if method == "pcg" else SC.DENOM_RV)
    assert all(w.status == "converged" for k, w in by.items() if k != "nan")
    assert (by["zero"].iterations, by["zero"].x.any()) == (0, False)
    assert MC.spread_ok([w.iterations for w in c["want"]]), [w.iterations for w in c["want"]]
    plan = S.KrylovMultiPlan(n, P.drp, P.dci, s, method=method, precond="jacobi" if jacobi else None)
    dB, dX = device_blocks(torch, cuda, c, layout)
    X, st = plan.solve(P.dval, dB, X=dX, dinv=P.ddinv, rtol=RTOL, max_iter=1000, check_every=check_every)
    assert X is dX
    if check_every == 7:
        print("%s%s, %s: iterations %s" % (method, " with Jacobi" if jacobi else "", layout, dict(zip(c["names"], st["iterations"].tolist()))))
    assert_solved(S, st, X, c)
    if layout == "slice":                                                   # the wider tensor around X is untouched
        wide = dX._base if dX._base is not None else dX
        assert float(wide.reshape(-1)[0]) == -7.0
    info = plan.info()
    lim = S.krylov_multi_limits()
    assert (info["n"], info["nrhs"], info["method"], info["precond"]) == (n, s, method, "jacobi" if jacobi else None)
    assert info["blocks"] == (lim["pcg_blocks"] if method == "pcg" else lim["bicgstab_blocks"]) and info["block_bytes"] >= 8 * n * s
    assert info["bytes"] >= info["blocks"] * info["block_bytes"] + info["partial_bytes"] + info["scalar_bytes"] + info["workspace_bytes"]
    assert info["launches"] == S.krylov_multi_launches(method, "jacobi" if jacobi else None, 0)
    # a second solve on the same plan has the same bits: nothing of the first is left in the work blocks
    dB2, dX2 = device_blocks(torch, cuda, c, layout)
    X2, st2 = plan.solve(P.dval, dB2, X=dX2, dinv=P.ddinv, rtol=RTOL, max_iter=1000, check_every=check_every)
    assert_solved(S, st2, X2, c)
    plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# graph
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,jacobi,layout", [("pcg", True, "slice"), ("bicgstab", False, "slice")])
def test_iterate_replays_in_a_graph(env, composed, method, jacobi, layout):
    S, torch, cuda = env
    c = composed(method, jacobi, layout)
    P, n, s = c["P"], c["A"][0], c["B"].shape[1]
    plan = S.KrylovMultiPlan(n, P.drp, P.dci, s, method=method, precond="jacobi" if jacobi else None)
    dB, dX = device_blocks(torch, cuda, c, layout)
    ex, est = plan.solve(P.dval, dB, X=dX.clone(), dinv=P.ddinv, rtol=RTOL, check_every=9)   # eager: the bits to meet; loads the code objects
    assert_solved(S, est, ex, c)
    plan.start(P.dval, dB, dX, dinv=P.ddinv, rtol=RTOL)                      # start runs eagerly
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
            _, fresh = device_blocks(torch, cuda, c, layout)
            dX.copy_(fresh)
            plan.start(P.dval, dB, dX, dinv=P.ddinv, rtol=RTOL)
        for replay in range(1, 200):
            g.replay()
            st = plan.status()
            if st["running"] == 0:
                break
        assert replay == -(-most // 9), (replay, most)
        assert_solved(S, st, dX, c)
        for key in ("code", "iterations", "rnorm", "alpha", "beta", "omega", "which"):
            assert same(st[key].astype(np.float64), est[key].astype(np.float64)), key
    plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# it solves
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,jacobi", [("pcg", False), ("pcg", True), ("bicgstab", False), ("bicgstab", True)])
def test_it_solves_as_well_as_the_single_solver(env, method, jacobi):
    """Each converged column's true residual |b_j - A x_j| (float64, on the host) against the same column's KrylovPlan
    solve: within a factor 4.  Measured on an MI355X (the smallest and the largest ratio over the eight converging
    columns; profiles/r23_krylov_multi.json has each): PCG 1 - 2.4e-8 and 1 + 1.2e-7 with the same counts in every
    column; with Jacobi 1 - 7.5e-7 and 1 + 8.8e-8; BiCGStab 0.99997 and 1.159 (e_k, 72 iterations on both sides); with
    Jacobi 0.9095 (e_k, 73 iterations against 70) and 1.00001.  The counts are not compared: BiCGStab's differ by
    three on e_k, as they may between any two roundings of an irregular recurrence."""
    S, torch, cuda = env
    A = MATRICES[method]()
    n, rp, ci, val = A
    B, X0, names = MC.columns(n, lambda v: KN.matvec(*A, v))
    s = B.shape[1]
    drp, dci, dval = up(torch, cuda, rp, ci, val)
    precond = "jacobi" if jacobi else None
    ddinv = up(torch, cuda, 1.0 / val[SC.stored_diagonal(rp, ci)])[0] if jacobi else None
    X, st = S.KrylovMultiPlan(n, drp, dci, s, method=method, precond=precond).solve(dval, block(torch, cuda, B), X=block(torch, cuda, X0),
                                                                                     dinv=ddinv, rtol=RTOL)
    x = X.cpu().numpy()
    single = S.KrylovPlan(n, drp, dci, method=method, precond=precond)
    true = lambda b, v: float(np.linalg.norm(b - KN.matvec(n, rp, ci, val, v)))
    ratios, counts = {}, {}
    for j, name in enumerate(names):
        db, dx = up(torch, cuda, B[:, j], X0[:, j])
        xs, sst = single.solve(dval, db, x=dx, dinv=ddinv, rtol=RTOL)
        assert st["status"][j] == sst["status"], (name, st["status"][j], sst)
        if sst["status"] != "converged":
            assert name == "nan"
            continue
        mine, theirs = true(B[:, j], x[:, j]), true(B[:, j], xs.cpu().numpy())
        ratios[name] = mine / theirs if theirs > 0.0 else (1.0 if mine == 0.0 else np.inf)
        counts[name] = (int(st["iterations"][j]), sst["iterations"])
        assert mine <= 4.0 * theirs, (name, mine, theirs)
    print("%s%s: true residual over the single solver's: %s" % (method, " with Jacobi" if jacobi else "",
                                                                 {k: round(v, 3) for k, v in ratios.items()}))
    print("    iterations (batched, single): %s" % counts)
    assert len(ratios) == s - 1
    single.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# edges and refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lap(env):
    S, torch, cuda = env
    n, rp, ci, val = KN.laplacian(24)
    drp, dci, dval = up(torch, cuda, rp, ci, val)
    return dict(n=n, rp=rp, ci=ci, val=val, drp=drp, dci=dci, dval=dval)


def test_one_column_and_sixty_four(env, lap):
    S, torch, cuda = env
    n, rng = lap["n"], np.random.default_rng(5)
    A = (n, lap["rp"], lap["ci"], lap["val"])
    # s = 1 against its composition, bit for bit
    P = MultiParts(env, A, 1, False)
    B, X0 = rng.standard_normal((n, 1)), np.zeros((n, 1))
    want = MC.composed_pcg_multi(P.matvec, P.apply, P.dot, B, X0, 1e-8, 1000)
    X, st = S.pcg_multi((n, lap["drp"], lap["dci"], lap["dval"]), block(torch, cuda, B), rtol=1e-8)
    assert_solved(S, st, X, dict(names=["only"], want=want))
    assert want[0].status == "converged" and want[0].iterations > 10
    P.destroy()
    # s = 64, the widest: every column converges and solves.  |r| of the recurrence meets rtol |b|; the true residual
    # differs from it by the rounding of some fifty iterations, about 50 eps |A| |x| ~ 1e-13 |b|, far inside a factor 2
    B = rng.standard_normal((n, 64)) * 10.0 ** rng.integers(-2, 3, 64)
    for solve, vals in ((S.pcg_multi, lap["val"]), (S.bicgstab_multi, lap["val"])):
        X, st = solve((n, lap["drp"], lap["dci"], lap["dval"]), block(torch, cuda, B), precond="jacobi", rtol=1e-8, check_every=16)
        assert st["status"] == ["converged"] * 64 and st["running"] == 0
        x = X.cpu().numpy()
        for j in range(64):
            res = np.linalg.norm(B[:, j] - KN.matvec(n, lap["rp"], lap["ci"], vals, x[:, j]))
            assert st["rnorm"][j] <= 1e-8 * st["bnorm"][j] and res <= 2e-8 * np.linalg.norm(B[:, j]), (j, res)
    with pytest.raises(S.SblasError, match="right-hand sides"):
        S.pcg_multi((n, lap["drp"], lap["dci"], lap["dval"]), torch.zeros(n, 65, dtype=torch.float64, device=cuda))


def test_edges_per_column(env, lap):
    S, torch, cuda = env
    n, rng = lap["n"], np.random.default_rng(6)
    s = 4
    xs = rng.standard_normal(n)
    B = np.stack([rng.standard_normal(n), np.zeros(n), KN.matvec(n, lap["rp"], lap["ci"], lap["val"], xs), rng.standard_normal(n)], axis=1)
    X0 = np.stack([np.zeros(n), rng.standard_normal(n), xs, np.zeros(n)], axis=1)   # column 2 starts at its solution
    for method in ("pcg", "bicgstab"):
        plan = S.KrylovMultiPlan(n, lap["drp"], lap["dci"], s, method=method)
        dB, dX = block(torch, cuda, B), block(torch, cuda, X0)
        # max_iter = 0: the limit at iteration 0, unless converged there
        plan.start(lap["dval"], dB, dX, rtol=1e-8, max_iter=0)
        plan.iterate(3)
        st = plan.status()
        assert st["status"] == ["limit", "converged", "converged", "limit"] and not st["iterations"].any() and st["running"] == 0
        x = dX.cpu().numpy()
        assert not x[:, 1].any() and same(x[:, [0, 2, 3]], X0[:, [0, 2, 3]])  # b = 0: x = 0; the others untouched
        assert st["bnorm"][1] == 0.0 and st["rnorm"][2] <= 1e-8 * st["bnorm"][2]
        # the same with iterations to spend: columns 1 and 2 stay frozen at 0 while 0 and 3 go on
        dX = block(torch, cuda, X0)
        X, st = plan.solve(lap["dval"], dB, X=dX, rtol=1e-8, check_every=5)
        assert st["status"] == ["converged"] * 4 and st["iterations"][1] == 0 and st["iterations"][2] == 0
        assert st["iterations"][0] > 10 and st["iterations"][3] > 10
        x = X.cpu().numpy()
        assert not x[:, 1].any() and same(x[:, 2], X0[:, 2])
        plan.destroy()
    # n = 0: nothing is launched and every column reads converged
    rp0, ci0 = torch.zeros(1, dtype=torch.int32, device=cuda), torch.zeros(0, dtype=torch.int32, device=cuda)
    v0 = torch.zeros(0, dtype=torch.float64, device=cuda)
    plan = S.KrylovMultiPlan(0, rp0, ci0, 3)
    e = torch.zeros((0, 3), dtype=torch.float64, device=cuda)
    X, st = plan.solve(v0, e, X=e.clone())
    assert st["status"] == ["converged"] * 3 and not st["iterations"].any() and not st["rnorm"].any() and st["running"] == 0
    assert plan.info()["bytes"] == 0
    plan.destroy()


@pytest.mark.parametrize("method", ["pcg", "bicgstab"])
def test_one_atol_governs_some_columns_and_rtol_the_others(env, method):
    """b, 1e3 b and 1e-3 b under one atol = 3e-9 |b| with rtol = 1e-10: rtol |b_j| is 1e-7, 1e-10 and 1e-13 |b|, so the
    first column stops on rtol |b_j| and the other two on atol -- max(rtol |b_j|, atol) per column, not atol wherever it
    is given and not one tolerance for the block.  Every column equals the composition, and the stops are where the
    tolerances put them: the scaled copies of one right-hand side need more iterations the tighter their relative bound."""
    S, torch, cuda = env
    A = n, rp, ci, val = MATRICES[method]()
    b = np.random.default_rng(17).standard_normal(n)
    B = np.ascontiguousarray(np.stack([1e3 * b, b, 1e-3 * b], axis=1))
    X0 = np.zeros_like(B)
    atol = 3e-9 * float(np.linalg.norm(b))
    P = MultiParts(env, A, 3, True)
    loop = MC.composed_pcg_multi if method == "pcg" else MC.composed_bicgstab_multi
    want = loop(P.matvec, P.apply, P.dot, B, X0, RTOL, 1000, atol=atol)
    assert [w.status for w in want] == ["converged"] * 3
    assert RTOL * want[0].bnorm > atol > RTOL * want[1].bnorm > RTOL * want[2].bnorm
    assert want[0].rnorm <= RTOL * want[0].bnorm and all(RTOL * w.bnorm < w.rnorm <= atol for w in want[1:])
    assert want[2].iterations < want[1].iterations and want[2].iterations < want[0].iterations     # 3e-6, 3e-9 and 1e-10 relative
    plan = S.KrylovMultiPlan(n, P.drp, P.dci, 3, method=method, precond="jacobi")
    X, st = plan.solve(P.dval, up(torch, cuda, B)[0], X=up(torch, cuda, X0)[0], dinv=P.ddinv, rtol=RTOL, atol=atol, max_iter=1000, check_every=5)
    assert_solved(S, st, X, dict(names=["1e3 b", "b", "1e-3 b"], want=want))
    plan.destroy()
    P.destroy()


def test_an_empty_block_that_came_from_numpy_is_taken(env):
    """n = 0: a (0, s) tensor made from a numpy array has strides (0, 0), where torch.zeros((0, s)) has (s, 1).  Without
    rows there are no strides to read: the plans, the one-shots and AmgPlan.apply_multi take either (found by
    tools/fuzz_multi.py, case 3 of seed 5: the one-shots refused the block as not row-major)."""
    S, torch, cuda = env
    rp0, ci0 = torch.zeros(1, dtype=torch.int32, device=cuda), torch.zeros(0, dtype=torch.int32, device=cuda)
    v0 = torch.zeros(0, dtype=torch.float64, device=cuda)
    e = torch.from_numpy(np.zeros((0, 8))).to(cuda)
    assert tuple(e.stride()) == (0, 0)
    for call in (S.pcg_multi, S.bicgstab_multi, S.gmres_multi):
        X, st = call((0, rp0, ci0, v0), e, X=e.clone())
        assert tuple(X.shape) == (0, 8) and st["status"] == ["converged"] * 8 and st["running"] == 0 and not st["iterations"].any()
    amg = S.AmgPlan(0, rp0, ci0)
    amg.setup(v0)
    assert tuple(amg.apply_multi(e).shape) == (0, 8)
    amg.destroy()


def test_refusals_come_before_any_launch(env, lap):
    S, torch, cuda = env
    E = S.SblasError
    n, s = lap["n"], 5
    drp, dci, dval = lap["drp"], lap["dci"], lap["dval"]
    for bad in (0, 65, -1):
        with pytest.raises(E, match="right-hand sides"):
            S.KrylovMultiPlan(n, drp, dci, bad)
    ilu = S.Ilu0Plan(n, drp, dci)
    for precond, what in ((ilu, "ilu0"), ("ilu0", "ilu0"), ("amg", "amg"), ("chebyshev", "chebyshev")):
        with pytest.raises(E, match="the %s preconditioner has no multi-column apply" % what):
            S.KrylovMultiPlan(n, drp, dci, s, precond=precond)
    L = S.lib()
    import ctypes as C
    h = C.c_void_p()
    for kind in (S.PRECOND_ILU0, S.PRECOND_AMG, S.PRECOND_CHEBYSHEV, 7):     # the library itself refuses them at create
        assert L.sblas_hip_krylov_multi_plan_create(-1, None, 0, n, dci.numel(), drp.data_ptr(), dci.data_ptr(), s, kind, C.byref(h)) == 1
        assert not h.value
    for width in (0, 65):
        assert L.sblas_hip_krylov_multi_plan_create(-1, None, 0, n, dci.numel(), drp.data_ptr(), dci.data_ptr(), width, 0, C.byref(h)) == 1
    ilu.destroy()
    plan = S.KrylovMultiPlan(n, drp, dci, s, precond="jacobi")
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=cuda)
    B = torch.ones((n, s), dtype=torch.float64, device=cuda)
    X = torch.full((n, s), -7.0, dtype=torch.float64, device=cuda)
    dinv = torch.full((n,), 0.25, dtype=torch.float64, device=cuda)
    with pytest.raises(E):
        plan.iterate(1)                                                      # before start
    with pytest.raises(E):
        plan.status()
    wide = z(n, 2 * s)
    cases = [
        ("dinv", dict(B=B, X=X)),                                            # Jacobi without dinv
        ("dinv must be contiguous", dict(B=B, X=X, dinv=z(n + 1))),
        ("tensor", dict(B=z(n, s + 1), X=X, dinv=dinv)),                     # another width
        ("tensor", dict(B=z(n * s), X=X, dinv=dinv)),                        # 1-D, as pcg() takes it
        ("row-major", dict(B=B, X=torch.as_strided(z(n * s), (n, s), (s - 1, 1)), dinv=dinv)),     # ld < s
        ("row-major", dict(B=z(s, n).t(), X=X, dinv=dinv)),                  # column-major
        ("float64", dict(B=B.float(), X=X, dinv=dinv)),
        ("float64", dict(B=B, X=X, dinv=dinv.float())),
        ("GPU tensor", dict(B=B.cpu(), X=X, dinv=dinv)),
        ("overlap", dict(B=B, X=B, dinv=dinv)),
        ("overlap", dict(B=wide[:, :s], X=wide[:, s:], dinv=dinv)),          # interleaved slices of one tensor: ranges overlap
        ("rtol and atol", dict(B=B, X=X, dinv=dinv, rtol=-1.0)),
        ("rtol and atol", dict(B=B, X=X, dinv=dinv, atol=float("nan"))),
        ("max_iter", dict(B=B, X=X, dinv=dinv, max_iter=-1)),
    ]
    for match, kw in cases:
        with pytest.raises(E, match=match):
            plan.start(dval, **kw)
    with pytest.raises(E, match="val"):
        plan.start(dval[:-1], B, X, dinv=dinv)
    with pytest.raises(E, match="check_every"):
        plan.solve(dval, B, X=X, dinv=dinv, check_every=0)
    # the library's own checks, for a caller that comes through the C ABI
    start = L.sblas_hip_krylov_multi_start
    args = lambda **k: [k.get("plan", plan.handle), None, dval.data_ptr(), k.get("dinv", dinv.data_ptr()), k.get("B", B.data_ptr()),
                        k.get("ldb", s), k.get("X", X.data_ptr()), k.get("ldx", s), k.get("rtol", 1e-8), 0.0, k.get("max_iter", 10)]
    for k in (dict(ldb=s - 1), dict(ldx=s - 1), dict(X=B.data_ptr()), dict(X=B.data_ptr() + 8), dict(dinv=None), dict(B=None),
              dict(rtol=float("nan")), dict(max_iter=-1), dict(plan=None)):
        assert start(*args(**k)) == 1, k
    with pytest.raises(E):
        plan.iterate(1)                                                      # still not started
    torch.cuda.synchronize()
    assert bool((X == -7.0).all()) and bool((B == 1.0).all())               # nothing ran
    # the single solvers still refuse 2-D input
    with pytest.raises(E):
        S.pcg((n, drp, dci, dval), B)
    with pytest.raises(E):
        S.bicgstab((n, drp, dci, dval), B)
    plan.destroy()
