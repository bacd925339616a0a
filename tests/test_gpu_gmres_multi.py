"""Multi-right-hand-side GMRES on the GPU (GmresMultiPlan, gmres_multi_dots, gmres_multi_project, gmres_multi_combine,
gmres_multi) against tests/gmres_multi_compose.py, the single solver's kernels and tests/gmres_numerics.py.

Every bit is pinned, so most checks are ==: column c of a multi-dot against sblas_krylov_dot_ref on the two columns, the
projection and the combination against gmres_project / gmres_combine on contiguous copies column by column, and a whole
solve against the lockstep loop composed from an SpmmPlan of the test's own, krylov_dot per column, numpy updates and the
Python scalar step.  Only "it solves" holds a tolerance: the single solver's bound, twice the larger of the host
GMRES's true residual and rtol |b|."""
import ctypes as C

import numpy as np
import pytest

import gmres_multi_compose as GMC
import gmres_numerics as GN
import krylov_numerics as KN
import multi_compose as MC
import solver_compose as SC

pytestmark = pytest.mark.gpu

RTOL = 1e-8
CELL = KN.CELL
SENTINEL = -7.0


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


def basis(torch, cuda, V, ld, offset):
    """host (k, n, s) as k device blocks at leading dimension ld, one behind the other, `offset` elements into an allocation"""
    k, n, s = V.shape
    buf = torch.full((offset + k * n * ld + 1,), SENTINEL, dtype=torch.float64, device=cuda)
    view = buf[offset:offset + k * n * ld].view(k, n, ld)[:, :, :s]
    view.copy_(torch.from_numpy(np.ascontiguousarray(V)).to(cuda))
    return view


def layouts(s):
    """(ld, offset): ld = s and s + 3, the base 16-byte aligned and one element off, which forces the 8-byte path"""
    return [(ld, offset) for ld in (s, s + 3) for offset in (0, 1)]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernels alone
# ---------------------------------------------------------------------------------------------------------------------
S_MAX, KS = 17, (1, 4, 5, 65)


def reference(env, n, s_max, ks, seed):
    """operands of s_max columns and max(ks) basis blocks, and what the single kernels give column by column on contiguous
    copies: dots[i, c], and per k the projected w (with its stage 1 of (w, w)) and the combination"""
    S, torch, cuda = env
    rng = np.random.default_rng(seed)
    k_max = max(ks)
    scale = 10.0 ** rng.integers(-3, 4, s_max)
    V = rng.standard_normal((k_max, n, s_max)) * scale
    W = rng.standard_normal((n, s_max)) / scale
    H = rng.standard_normal((s_max, k_max))
    cells = -(-n // CELL)
    ref = dict(V=V, W=W, H=H, cells=cells, dots=np.zeros((k_max, s_max)), w={}, part={}, u={})
    for c in range(s_max):
        wc = np.ascontiguousarray(W[:, c])
        for i in range(k_max):
            ref["dots"][i, c] = S.krylov_dot_ref(np.ascontiguousarray(V[i, :, c]), wc)
        dV, dh = up(torch, cuda, V[:, :, c], H[c])
        for k in ks:
            dw, = up(torch, cuda, wc)
            part = torch.zeros(cells, dtype=torch.float64, device=cuda)
            S.gmres_project(dV[:k], dh[:k].contiguous(), dw, partial=part)
            ref["w"][k, c], ref["part"][k, c] = dw.cpu().numpy(), part.cpu().numpy()
            ref["u"][k, c] = S.gmres_combine(dV[:k], dh[:k].contiguous()).cpu().numpy()
    return ref


def check_kernels(env, ref, n, s, ks, where):
    S, torch, cuda = env
    V, W, H, cells = ref["V"], ref["W"], ref["H"], ref["cells"]
    dH, = up(torch, cuda, H[:s])
    for ld, offset in layouts(s):
        dV = basis(torch, cuda, V[:, :, :s], ld, offset)
        for k in ks:
            tag = (where, n, s, k, ld, offset)
            gW = Guarded(torch, cuda, W[:, :s], ld, offset)
            got = S.gmres_multi_dots(dV[:k], gW.view).cpu().numpy()
            assert got.shape == (k, s) and same(got, ref["dots"][:k, :s]), tag
            want_w = np.stack([ref["w"][k, c] for c in range(s)], axis=1)
            assert S.gmres_multi_project(dV[:k], dH, gW.view) is gW.view
            assert same(gW.host(), want_w) and gW.intact(), tag               # the padding and what lies beyond n: untouched
            gW = Guarded(torch, cuda, W[:, :s], ld, offset)
            part = torch.full((s * cells + 1,), SENTINEL, dtype=torch.float64, device=cuda)
            S.gmres_multi_project(dV[:k], dH, gW.view, partial=part)
            p = part.cpu().numpy()
            assert same(gW.host(), want_w) and gW.intact() and p[-1] == SENTINEL, tag
            assert same(p[:-1].reshape(s, cells), np.stack([ref["part"][k, c] for c in range(s)])), tag
            gU = Guarded(torch, cuda, np.full((n, s), np.nan), ld, offset)
            assert S.gmres_multi_combine(dV[:k], dH, out=gU.view) is gU.view
            assert same(gU.host(), np.stack([ref["u"][k, c] for c in range(s)], axis=1)) and gU.intact(), tag


@pytest.mark.parametrize("n", [1, 255, 257, CELL + 1, 3 * CELL + 5])
def test_the_kernels_have_the_single_kernels_bits_column_by_column(env, n):
    ref = reference(env, n, S_MAX, KS, seed=n)
    for s in (1, 3, 8, 9, 17):
        check_kernels(env, ref, n, s, KS, "kernels")


def test_the_kernels_at_sixty_four_columns(env):
    n = 257
    ref = reference(env, n, 64, (5,), seed=64)
    check_kernels(env, ref, n, 64, (5,), "widest")


def test_a_frozen_column_is_neither_read_nor_written(env):
    S, torch, cuda = env
    n, s, k = CELL + 1, 9, 5
    ref = reference(env, n, s, (k,), seed=3)
    frozen = [2, 8]                                                          # 2: in a mixed tile; 8: a tile of its own, which returns at entry
    live = [c for c in range(s) if c not in frozen]
    scal = torch.zeros((s, 16), dtype=torch.float64, device=cuda)
    scal.view(torch.int64)[frozen, 0] = 1                                    # anything but RUNNING
    V, W, H = ref["V"].copy(), ref["W"].copy(), ref["H"].copy()
    V[:, :, frozen], H[frozen] = np.nan, np.nan                              # what must not be read
    W[:, frozen] = SENTINEL
    dH, = up(torch, cuda, H)
    for ld, offset in layouts(s):
        dV = basis(torch, cuda, V, ld, offset)
        gW = Guarded(torch, cuda, W, ld, offset)
        out = torch.full((k, s), SENTINEL, dtype=torch.float64, device=cuda)
        got = S.gmres_multi_dots(dV, gW.view, scalars=scal, out=out).cpu().numpy()
        assert same(got[:, live], ref["dots"][:k, live]) and (got[:, frozen] == SENTINEL).all(), (ld, offset)
        part = torch.full((s * ref["cells"],), SENTINEL, dtype=torch.float64, device=cuda)
        S.gmres_multi_project(dV, dH, gW.view, partial=part, scalars=scal)
        w, p = gW.host(), part.cpu().numpy().reshape(s, -1)
        assert same(w[:, live], np.stack([ref["w"][k, c] for c in live], axis=1)) and (w[:, frozen] == SENTINEL).all() and gW.intact()
        assert same(p[live], np.stack([ref["part"][k, c] for c in live])) and (p[frozen] == SENTINEL).all()
        gU = Guarded(torch, cuda, np.full((n, s), SENTINEL), ld, offset)
        S.gmres_multi_combine(dV, dH, out=gU.view, scalars=scal)
        u = gU.host()
        assert same(u[:, live], np.stack([ref["u"][k, c] for c in live], axis=1)) and (u[:, frozen] == SENTINEL).all() and gU.intact()


def test_the_kernels_refusals(env):
    S, torch, cuda = env
    E = S.SblasError
    n, s, k = 300, 5, 4
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=cuda)
    V, W, H = z(k, n, s), z(n, s), z(s, k)
    with pytest.raises(E, match="basis blocks"):
        S.gmres_multi_dots(z(66, 4, s), z(4, s))
    with pytest.raises(E, match="right-hand sides"):
        S.gmres_multi_dots(z(2, 4, 65), z(4, 65))
    with pytest.raises(E, match="tensor"):
        S.gmres_multi_dots(V, z(n, s + 1))
    with pytest.raises(E, match="float64"):
        S.gmres_multi_dots(V, W.float())
    with pytest.raises(E, match="block stride"):
        S.gmres_multi_dots(torch.as_strided(z(k * n * s), (k, n, s), (n * s - 1, s, 1)), W)
    with pytest.raises(E, match="leading dimension"):
        S.gmres_multi_dots(torch.as_strided(z(k * n * s), (k, n, s), (n * s, s - 1, 1)), W)
    with pytest.raises(E, match="coefficients"):
        S.gmres_multi_project(V, z(s, k - 1), W)
    with pytest.raises(E, match="too short"):
        S.gmres_multi_project(V, H, W, partial=z(s - 1))
    with pytest.raises(E, match="x 16 slots"):
        S.gmres_multi_combine(V, H, scalars=z(s - 1, 16))
    with pytest.raises(E):                                                   # a short workspace is refused, not overrun
        S.gmres_multi_dots(V, W, workspace=z(k * s - 1))
    L = S.lib()
    out, ws = z(k, s), z(k * s)
    args = lambda ldv, stride, ldw, wbytes: (-1, None, n, s, k, V.data_ptr(), ldv, stride, W.data_ptr(), ldw, None, out.data_ptr(), ws.data_ptr(), wbytes)
    assert L.sblas_hip_gmres_multi_dots_f64(*args(s, n * s, s, ws.numel() * 8)) == 0
    assert L.sblas_hip_gmres_multi_dots_f64(*args(s - 1, n * s, s, ws.numel() * 8)) == 1
    assert L.sblas_hip_gmres_multi_dots_f64(*args(s, n * s - 1, s, ws.numel() * 8)) == 1
    assert L.sblas_hip_gmres_multi_dots_f64(*args(s, n * s, s - 1, ws.numel() * 8)) == 1
    assert L.sblas_hip_gmres_multi_dots_f64(*args(s, n * s, s, ws.numel() * 8 - 8)) == 3
    assert L.sblas_hip_gmres_multi_project_f64(-1, None, n, s, k, V.data_ptr(), s, n * s, H.data_ptr(), k - 1, W.data_ptr(), s, None, None) == 1
    assert L.sblas_hip_gmres_multi_combine_f64(-1, None, n, 65, k, V.data_ptr(), 65, n * 65, H.data_ptr(), k, W.data_ptr(), 65, None) == 1
    torch.cuda.synchronize()
    assert not out.any().item()


# ---------------------------------------------------------------------------------------------------------------------
# 2. whole solves against their own composition
# ---------------------------------------------------------------------------------------------------------------------
class Parts:
    """the device's parts of a lockstep loop: A V by an SpmmPlan of the test's own for width s, called row-major; the
    pinned dot per column (a vector met before is not sent again); M^-1 on ONE column: a numpy product with dinv,
    AmgPlan.apply or Ilu0Plan.apply"""

    def __init__(self, env, A, s, precond):
        S, torch, cuda = self.env = env
        self.n, self.rp, self.ci, self.val = A[0], A[1].astype(np.int32), A[2].astype(np.int32), A[3]
        self.s, self.precond = s, precond
        self.drp, self.dci, self.dval = up(torch, cuda, self.rp, self.ci, self.val)
        self.spmm = S.SpmmPlan(self.n, self.n, self.drp, self.dci, s)
        self.ws = torch.empty(max(S.spmm_workspace_bytes(self.n, self.n, len(self.ci), s) // 8, 1), dtype=torch.float64, device=cuda)
        self.dinv = self.ddinv = self.amg = self.ilu = self.lu = None
        self.seat = precond                                                  # what GmresMultiPlan takes
        if precond == "jacobi":
            self.dinv = 1.0 / self.val[SC.stored_diagonal(self.rp, self.ci)]
            self.ddinv, = up(torch, cuda, self.dinv)
        elif precond in ("amg", "amg_smoothed"):
            self.seat = self.amg = S.AmgPlan(self.n, self.drp, self.dci, prolongator="smoothed" if precond == "amg_smoothed" else "plain")
            self.amg.setup(self.dval)
        elif precond == "ilu0":
            self.ilu = S.Ilu0Plan(self.n, self.drp, self.dci)
            self.lu = self.ilu.factor(self.dval)
            self.seat = self.ilu.solvers()
        self._sent = {}

    def kw(self):
        return dict(dinv=self.ddinv, lu=self.lu)

    def matvec(self, V):
        S, torch, cuda = self.env
        dv, = up(torch, cuda, V)
        out = torch.empty(self.n * self.s, dtype=torch.float64, device=cuda)
        self.spmm.spmm_ordered(self.dval, dv.reshape(-1), self.s, S.ROW_MAJOR, self.s, 1.0, 0.0, out, self.s, S.ROW_MAJOR, self.ws)
        return out.cpu().numpy().reshape(self.n, self.s)

    def _dev(self, a):
        hit = self._sent.get(id(a))
        if hit is None:
            if len(self._sent) > 2048:
                self._sent.clear()
            hit = self._sent[id(a)] = (a, up(self.env[1], self.env[2], a)[0])  # the array is kept, so its id stays its own
        return hit[1]

    def dot(self, a, b):
        S = self.env[0]
        return float(S.krylov_dot(self._dev(a), self._dev(b)).cpu().numpy()[0])

    def apply(self, v):
        S, torch, cuda = self.env
        if self.amg is not None:
            return self.amg.apply(up(torch, cuda, v)[0]).cpu().numpy()
        if self.ilu is not None:
            return self.ilu.apply(self.lu, up(torch, cuda, v)[0]).cpu().numpy()
        return self.dinv * v if self.dinv is not None else v

    def destroy(self):
        self._sent.clear()
        for p in (self.spmm, self.amg, self.ilu):
            if p is not None:
                p.destroy()


MATRICES = {"conv24": lambda: KN.convection_diffusion(24), "conv48": lambda: KN.convection_diffusion(48), "lap32": lambda: KN.laplacian(32)}
# name: (matrix, s, restart, precond, layout, max_iter).  s in {1, 3, 8, 9} and restart in {1, 5, 30, 64} each with none and
# with Jacobi on both convection-diffusion matrices (48^2: two cells, the second ragged); "slice": X a column slice of a
# wider tensor at an odd offset (no 16-byte path anywhere), "aligned": contiguous (s = 8: one full tile on the 16-byte
# path until its first column freezes).  A bounded max_iter keeps a case short and ends its running columns in LIMIT.
CASES = {
    "24-s9-m30-none": ("conv24", 9, 30, None, "slice", 1000),
    "24-s9-m5-jacobi": ("conv24", 9, 5, "jacobi", "slice", 60),
    "24-s8-m64-jacobi": ("conv24", 8, 64, "jacobi", "aligned", 1000),
    "24-s3-m1-none": ("conv24", 3, 1, None, "aligned", 25),
    "24-s1-m5-none": ("conv24", 1, 5, None, "aligned", 40),
    "24-s9-m5-limit7": ("conv24", 9, 5, None, "slice", 7),
    "48-s9-m30-jacobi": ("conv48", 9, 30, "jacobi", "slice", 70),
    "48-s8-m5-none": ("conv48", 8, 5, None, "aligned", 40),
    "48-s3-m64-none": ("conv48", 3, 64, None, "slice", 70),
    "48-s1-m30-jacobi": ("conv48", 1, 30, "jacobi", "aligned", 45),
    "48-s9-m1-jacobi": ("conv48", 9, 1, "jacobi", "slice", 12),
    "24-s9-m30-amg": ("conv24", 9, 30, "amg", "slice", 1000),
    "24-s9-m5-amg_smoothed": ("conv24", 9, 5, "amg_smoothed", "slice", 1000),
    "24-s9-m30-ilu0": ("conv24", 9, 30, "ilu0", "slice", 1000),
    "32-s8-m5-amg": ("lap32", 8, 5, "amg", "aligned", 1000),
    "32-s9-m30-amg_smoothed": ("lap32", 9, 30, "amg_smoothed", "slice", 1000),
    "32-s9-m5-ilu0": ("lap32", 9, 5, "ilu0", "slice", 1000),
}


def case_columns(A, s):
    B, X0, names = MC.columns(A[0], lambda v: KN.matvec(*A, v))
    keep = list(range(9)) if s == 9 else [j for j, name in enumerate(names) if name != "large"] if s == 8 else list(range(s))
    return np.ascontiguousarray(B[:, keep]), np.ascontiguousarray(X0[:, keep]), [names[j] for j in keep]


@pytest.fixture(scope="module")
def composed(env):
    """the composed loop of every case, run once and shared by the tests that compare against it"""
    made = {}

    def get(name):
        if name not in made:
            matrix, s, restart, precond, layout, max_iter = CASES[name]
            A = MATRICES[matrix]()
            B, X0, names = case_columns(A, s)
            P = Parts(env, A, s, precond)
            want = GMC.composed_gmres_multi(P.matvec, P.apply, P.dot, B, X0, restart, RTOL, max_iter)
            for w in want:
                w["x"].setflags(write=False)
            made[name] = dict(A=A, B=B, X0=X0, names=names, P=P, want=want, s=s, restart=restart, precond=precond, layout=layout,
                              max_iter=max_iter)
        return made[name]
    yield get
    for c in made.values():
        c["P"].destroy()


def device_blocks(torch, cuda, c):
    s = c["s"]
    if c["layout"] == "aligned":
        return Guarded(torch, cuda, c["B"]), Guarded(torch, cuda, c["X0"])
    return Guarded(torch, cuda, c["B"], s + 1, 0), Guarded(torch, cuda, c["X0"], s + 3, 1)   # X: a slice of a wider tensor


def assert_solved(st, X, c):
    x = X.cpu().numpy()
    for j, (name, w) in enumerate(zip(c["names"], c["want"])):
        got = dict(status=st["status"][j], iterations=int(st["iterations"][j]), restarts=int(st["restarts"][j]),
                   columns=int(st["columns"][j]), breakdown=st["breakdown"][j])
        assert got == {k: w[k] for k in got}, (name, got, {k: v for k, v in w.items() if k != "x"})
        assert same(st["rnorm"][j], w["rnorm"]) and same(st["bnorm"][j], w["bnorm"]), (name, st["rnorm"][j], w["rnorm"], st["bnorm"][j], w["bnorm"])
        assert same(x[:, j], w["x"]), (name, "x")
    assert st["running"] == 0


@pytest.mark.parametrize("check_every", [1, 7, 50])
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_solver_equals_its_own_composition(env, composed, name, check_every):
    S, torch, cuda = env
    c = composed(name)
    P, n, s, restart, max_iter = c["P"], c["A"][0], c["s"], c["restart"], c["max_iter"]
    by = dict(zip(c["names"], c["want"]))
    # the case is worth having
    if "zero" in by:
        assert (by["zero"]["status"], by["zero"]["iterations"], by["zero"]["x"].any()) == (GN.CONVERGED, 0, False)
    if "nan" in by:
        assert (by["nan"]["status"], by["nan"]["breakdown"], by["nan"]["iterations"]) == (GN.BREAKDOWN, "beta", 0)
    if max_iter == 1000:
        assert all(w["status"] == GN.CONVERGED for k, w in by.items() if k != "nan"), {k: w["status"] for k, w in by.items()}
    if max_iter == 7:                                                        # m = 5: every column that still runs stops at exactly 7
        limited = [w for w in c["want"] if w["status"] == GN.LIMIT]
        assert len(limited) >= 5 and all((w["iterations"], w["restarts"], w["columns"]) == (7, 1, 2) for w in limited)
    plan = S.GmresMultiPlan(n, P.drp, P.dci, s, restart=restart, precond=P.seat)
    gB, gX = device_blocks(torch, cuda, c)
    X, st = plan.solve(P.dval, gB.view, X=gX.view, rtol=RTOL, max_iter=max_iter, check_every=check_every, **P.kw())
    assert X is gX.view
    if check_every == 7:
        print("%s: (iterations, restarts) %s" % (name, {k: (int(i), int(r)) for k, i, r in zip(c["names"], st["iterations"], st["restarts"])}))
    assert_solved(st, X, c)
    assert gX.intact() and gB.intact() and same(gB.host(), c["B"])
    # iterate after the end changes nothing
    x_before = X.clone()
    plan.iterate(9)
    st9 = plan.status()
    assert torch.equal(X, x_before)
    for key in ("code", "iterations", "rnorm", "bnorm", "restarts", "columns", "eta", "which"):
        assert same(st9[key].astype(np.float64), st[key].astype(np.float64)), key
    if check_every == 7:
        info, lim = plan.info(), S.gmres_multi_limits()
        kind = {None: None, "jacobi": "jacobi", "amg": "amg", "amg_smoothed": "amg", "ilu0": "ilu0"}[c["precond"]]
        assert (info["n"], info["nrhs"], info["restart"], info["precond"]) == (n, s, restart, kind)
        assert info["blocks"] == restart + 1 + lim["fixed_blocks"] + (kind == "amg") and info["block_bytes"] >= 8 * n * s
        assert info["bytes"] >= info["blocks"] * info["block_bytes"] + info["partial_bytes"] + info["scalar_bytes"] + info["matrix_bytes"] + \
            info["workspace_bytes"]
        assert info["matrix_bytes"] >= s * lim["matrix_doubles"] * 8 and info["scalar_bytes"] >= s * 128
        counts = S.gmres_multi_launches(restart, P.seat, 0)
        assert (info["step_launches"], info["close_launches"], info["restart_launches"], info["cycle_launches"]) == \
            (counts["step"], counts["close"], counts["restart"], counts["cycle"])
        # a second solve on the same plan has the same bits: nothing of the first is left in the work blocks
        gB2, gX2 = device_blocks(torch, cuda, c)
        X2, st2 = plan.solve(P.dval, gB2.view, X=gX2.view, rtol=RTOL, max_iter=max_iter, check_every=check_every, **P.kw())
        assert_solved(st2, X2, c)
    plan.destroy()


def test_sixty_four_columns_at_restart_sixty_four(env):
    """the widest plan, about 20 MB.  |g| of the recurrence meets rtol |b| in every column; the true residual differs
    from it by the rounding of at most a few hundred steps, about 300 eps |A| |x| ~ 1e-12 |b|, far inside a factor 2"""
    S, torch, cuda = env
    n, rp, ci, val = KN.convection_diffusion(24)
    rng = np.random.default_rng(64)
    B = rng.standard_normal((n, 64)) * 10.0 ** rng.integers(-2, 3, 64)
    drp, dci, dval = up(torch, cuda, rp, ci, val)
    X, st = S.gmres_multi((n, drp, dci, dval), up(torch, cuda, B)[0], precond="jacobi", restart=64, rtol=RTOL, check_every=16)
    assert st["status"] == ["converged"] * 64 and st["running"] == 0
    x = X.cpu().numpy()
    for j in range(64):
        res = np.linalg.norm(B[:, j] - KN.matvec(n, rp, ci, val, x[:, j]))
        assert st["rnorm"][j] <= RTOL * st["bnorm"][j] and res <= 2 * RTOL * np.linalg.norm(B[:, j]), (j, res)
    plan = S.GmresMultiPlan(n, drp, dci, 64, restart=64)
    info = plan.info()
    assert info["blocks"] == 68 and 20e6 < info["bytes"] < 30e6
    plan.destroy()
    with pytest.raises(S.SblasError, match="right-hand sides"):
        S.gmres_multi((n, drp, dci, dval), torch.zeros(n, 65, dtype=torch.float64, device=cuda))
    with pytest.raises(S.SblasError):                                        # gmres keeps refusing a block
        S.gmres((n, drp, dci, dval), torch.zeros(n, 3, dtype=torch.float64, device=cuda))


# ---------------------------------------------------------------------------------------------------------------------
# 3. graph
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["24-s9-m5-jacobi", "24-s9-m30-ilu0"])
def test_iterate_replays_in_a_graph(env, composed, name):
    S, torch, cuda = env
    c = composed(name)
    P, n, s, restart, max_iter = c["P"], c["A"][0], c["s"], c["restart"], c["max_iter"]
    plan = S.GmresMultiPlan(n, P.drp, P.dci, s, restart=restart, precond=P.seat)
    gB, gX = device_blocks(torch, cuda, c)
    dB, dX = gB.view, gX.view
    chunk = restart + 2
    ex, est = plan.solve(P.dval, dB, X=dX.clone(), rtol=RTOL, max_iter=max_iter, check_every=chunk, **P.kw())   # eager: the bits to meet
    assert_solved(est, ex, c)
    # a second problem for the same graph: other right-hand sides, solved eagerly first
    B2 = np.ascontiguousarray(c["B"][:, ::-1]) * 1.5
    X02 = np.ascontiguousarray(c["X0"][:, ::-1])
    dB2, = up(torch, cuda, B2)
    ex2, est2 = plan.solve(P.dval, dB2, X=up(torch, cuda, X02)[0], rtol=RTOL, max_iter=max_iter, check_every=chunk, **P.kw())
    plan.start(P.dval, dB, dX, rtol=RTOL, max_iter=max_iter, **P.kw())       # start runs eagerly
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):                              # a linear chain of launches
            plan.iterate(chunk)
    st = plan.status()
    assert int(st["iterations"].max()) == 0                                  # capturing ran nothing
    for round_, (want_x, want_st) in enumerate(((ex, est), (ex2, est2))):    # the second: the same graph after a NEW start
        if round_:
            dB.copy_(dB2)
            dX.copy_(up(torch, cuda, X02)[0])
            plan.start(P.dval, dB, dX, rtol=RTOL, max_iter=max_iter, **P.kw())
        for replay in range(1, 400):
            g.replay()
            st = plan.status()
            if st["running"] == 0:
                break
        assert st["running"] == 0
        assert same(dX.cpu().numpy(), want_x.cpu().numpy())
        for key in ("code", "iterations", "rnorm", "bnorm", "restarts", "columns", "eta", "which"):
            assert same(st[key].astype(np.float64), want_st[key].astype(np.float64)), (round_, key)
    assert gX.intact()
    plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the freeze
# ---------------------------------------------------------------------------------------------------------------------
def test_a_frozen_column_keeps_its_x_its_basis_its_count_and_its_residual(env):
    S, torch, cuda = env
    A = n, rp, ci, val = KN.convection_diffusion(24)
    rng = np.random.default_rng(9)
    mv = lambda v: KN.matvec(*A, v)
    xs, xw = rng.standard_normal(n), rng.standard_normal(n)
    nan = rng.standard_normal(n)
    nan[n // 2] = np.nan
    # 0: runs long; 1: converged at start; 2: a NaN (BETA breakdown at 0); 3: a warm start that converges cycles before 0 and 4
    B = np.stack([rng.standard_normal(n), mv(xs), nan, mv(xw), rng.standard_normal(n)], axis=1)
    X0 = np.stack([np.zeros(n), xs, 0.1 * rng.standard_normal(n), xw + 1e-7 * rng.standard_normal(n), np.zeros(n)], axis=1)
    s, restart = 5, 5
    drp, dci, dval = up(torch, cuda, rp, ci, val)
    plan = S.GmresMultiPlan(n, drp, dci, s, restart=restart)
    gB, gX = Guarded(torch, cuda, B, s + 3, 1), Guarded(torch, cuda, X0, s + 3, 1)
    plan.start(dval, gB.view, gX.view, rtol=RTOL)

    def snapshot(cols):
        st = plan.status()
        V = torch.stack([plan.block(k) for k in range(restart + 1)]).cpu().numpy()
        return dict(x=gX.host()[:, cols], V=V[:, :, cols], it=st["iterations"][cols], rnorm=st["rnorm"][cols], code=st["code"][cols],
                    restarts=st["restarts"][cols], columns=st["columns"][cols])

    st = plan.status()
    assert st["status"][1] == "converged" and (st["status"][2], st["breakdown"][2]) == ("breakdown", "beta")
    assert [st["status"][c] for c in (0, 3, 4)] == ["running"] * 3
    at_start = snapshot([1, 2])
    assert same(at_start["x"], X0[:, [1, 2]])                                # untouched
    for _ in range(40):                                                      # until the warm start is there, and closed
        plan.iterate(restart)
        st = plan.status()
        if st["status"][3] != "running":
            break
    assert st["status"][3] == "converged" and st["status"][0] == st["status"][4] == "running", st["status"]
    early = snapshot([1, 2, 3])
    for _ in range(400):
        plan.iterate(7)
        st = plan.status()
        if st["running"] == 0:
            break
    assert st["status"] == ["converged", "converged", "breakdown", "converged", "converged"]
    assert st["restarts"][0] >= st["restarts"][3] + 3                        # cycles before the others
    late = snapshot([1, 2, 3])
    for key in early:
        assert same(np.asarray(late[key], np.float64), np.asarray(early[key], np.float64)), key
    at_end = snapshot([1, 2])
    for key in at_start:
        assert same(np.asarray(at_end[key], np.float64), np.asarray(at_start[key], np.float64)), key
    assert gB.intact() and gX.intact() and same(gB.host(), B)
    x = gX.host()
    for c in (0, 3, 4):
        assert np.linalg.norm(B[:, c] - mv(x[:, c])) <= 2 * RTOL * np.linalg.norm(B[:, c])
    plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# 5. it solves
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("restart,precond", [(30, None), (5, "jacobi")])
def test_it_solves(env, restart, precond):
    """Per column, the true residual |b - A x| against twice the larger of the host GMRES's and rtol |b|: the single
    solver's bound (test_gpu_gmres.py)."""
    S, torch, cuda = env
    A = n, rp, ci, val = KN.convection_diffusion(24)
    B, X0, names = MC.columns(n, lambda v: KN.matvec(*A, v))
    drp, dci, dval = up(torch, cuda, rp, ci, val)
    X, st = S.gmres_multi((n, drp, dci, dval), up(torch, cuda, B)[0], precond=precond, restart=restart, X=up(torch, cuda, X0)[0], rtol=RTOL)
    x = X.cpu().numpy()
    dinv = 1.0 / val[SC.stored_diagonal(rp, ci)]
    M = (lambda v: dinv * v) if precond == "jacobi" else None
    true = lambda b, v: float(np.linalg.norm(b - KN.matvec(n, rp, ci, val, v)))
    for j, name in enumerate(names):
        if name == "nan":
            assert st["status"][j] == "breakdown"
            continue
        assert st["status"][j] == "converged", (name, st["status"][j])
        if name == "zero":
            assert not x[:, j].any()
            continue
        steps, restarts, host_x = GN.host_gmres(n, rp, ci, val, B[:, j], X0[:, j], restart, RTOL, precond=M)
        got, host = true(B[:, j], x[:, j]), true(B[:, j], host_x)
        bound = 2.0 * max(host, RTOL * np.linalg.norm(B[:, j]))
        print("GMRES(%d) %s, %s: device %d steps and %d restarts, host %d and %d; true residual %.6e, the host's %.6e, bound %.6e"
              % (restart, precond, name, st["iterations"][j], st["restarts"][j], steps, restarts, got, host, bound))
        assert got <= bound, (name, got, bound)


# ---------------------------------------------------------------------------------------------------------------------
# 6. edges and refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_edges_per_column(env):
    S, torch, cuda = env
    A = n, rp, ci, val = KN.convection_diffusion(8)
    drp, dci, dval = up(torch, cuda, rp, ci, val)
    rng = np.random.default_rng(6)
    xs = rng.standard_normal(n)
    B = np.stack([rng.standard_normal(n), np.zeros(n), KN.matvec(*A, xs), rng.standard_normal(n)], axis=1)
    X0 = np.stack([np.zeros(n), rng.standard_normal(n), xs, np.zeros(n)], axis=1)   # column 2 starts at its solution
    plan = S.GmresMultiPlan(n, drp, dci, 4, restart=5)
    dB, dX = up(torch, cuda, B, X0)
    plan.start(dval, dB, dX, rtol=RTOL, max_iter=0)                          # max_iter = 0: the limit at 0, unless converged there
    plan.iterate(3)
    st = plan.status()
    assert st["status"] == ["limit", "converged", "converged", "limit"] and not st["iterations"].any() and st["running"] == 0
    x = dX.cpu().numpy()
    assert not x[:, 1].any() and same(x[:, [0, 2, 3]], X0[:, [0, 2, 3]])      # b = 0: x = 0; the others untouched
    assert st["bnorm"][1] == 0.0 and st["rnorm"][2] <= RTOL * st["bnorm"][2]
    plan.destroy()
    # the lucky breakdown: on the identity the first step ends with eta = 0, which converges without a division
    eye = (n,) + tuple(up(torch, cuda, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n)))
    E = np.zeros((n, 4))
    E[1, 0], E[5, 2], E[2, 3] = 1.0, 4.0, -1.0                               # v_0 = +-e_k exactly, h = 1, w - h v_0 = 0
    X, st = S.gmres_multi(eye, up(torch, cuda, E)[0], restart=5, rtol=RTOL)
    assert st["status"] == ["converged"] * 4 and st["iterations"].tolist() == [1, 0, 1, 1] and same(X.cpu().numpy(), E)
    assert not st["eta"].any() and not st["rnorm"].any()
    # the one-shot's other doors: an AmgPlan made and set up inside, plain and smoothed; a pair belongs to the plan
    A24 = n24, rp24, ci24, val24 = KN.convection_diffusion(24)
    B24 = rng.standard_normal((n24, 3))
    dA24 = (n24,) + tuple(up(torch, cuda, rp24, ci24, val24))
    for precond in ("amg", "amg_smoothed"):
        X, st = S.gmres_multi(dA24, up(torch, cuda, B24)[0], precond=precond, restart=10, rtol=RTOL)
        assert st["status"] == ["converged"] * 3 and 0 < st["iterations"].max() < 60, (precond, st["status"], st["iterations"])
        x = X.cpu().numpy()
        for c in range(3):                                                   # |g| <= rtol |b|; the true residual is it up to rounding
            assert np.linalg.norm(B24[:, c] - KN.matvec(*A24, x[:, c])) <= 2 * RTOL * np.linalg.norm(B24[:, c]), (precond, c)
    ilu = S.Ilu0Plan(n24, dA24[1], dA24[2])
    ilu.factor(dA24[3])
    with pytest.raises(S.SblasError, match="GmresMultiPlan"):
        S.gmres_multi(dA24, up(torch, cuda, B24)[0], precond=ilu.solvers())
    ilu.destroy()
    # n = 0: nothing is launched and every column reads converged
    rp0, ci0 = torch.zeros(1, dtype=torch.int32, device=cuda), torch.zeros(0, dtype=torch.int32, device=cuda)
    plan = S.GmresMultiPlan(0, rp0, ci0, 3)
    e = torch.zeros((0, 3), dtype=torch.float64, device=cuda)
    X, st = plan.solve(torch.zeros(0, dtype=torch.float64, device=cuda), e, X=e.clone())
    assert st["status"] == ["converged"] * 3 and not st["iterations"].any() and not st["rnorm"].any() and st["running"] == 0
    assert plan.info()["bytes"] == 0
    plan.destroy()


def test_one_atol_governs_some_columns_and_rtol_the_others(env):
    """b, 1e3 b and 1e-3 b under one atol = 3e-7 |b| with rtol = 1e-8: rtol |b_j| is 1e-5, 1e-8 and 1e-11 |b|, so the first
    column stops on rtol |b_j| and the other two on atol: max(rtol |b_j|, atol) per column"""
    S, torch, cuda = env
    A = n, rp, ci, val = KN.convection_diffusion(24)
    b = np.random.default_rng(17).standard_normal(n)
    B = np.ascontiguousarray(np.stack([1e3 * b, b, 1e-3 * b], axis=1))
    X0 = np.zeros_like(B)
    atol = 30.0 * RTOL * float(np.linalg.norm(b))
    P = Parts(env, A, 3, "jacobi")
    want = GMC.composed_gmres_multi(P.matvec, P.apply, P.dot, B, X0, 30, RTOL, 1000, atol=atol)
    assert [w["status"] for w in want] == [GN.CONVERGED] * 3
    assert RTOL * want[0]["bnorm"] > atol > RTOL * want[1]["bnorm"] > RTOL * want[2]["bnorm"]
    assert want[0]["rnorm"] <= RTOL * want[0]["bnorm"] and all(RTOL * w["bnorm"] < w["rnorm"] <= atol for w in want[1:])
    assert want[2]["iterations"] < want[1]["iterations"] < want[0]["iterations"]
    plan = S.GmresMultiPlan(n, P.drp, P.dci, 3, restart=30, precond=P.seat)
    X, st = plan.solve(P.dval, up(torch, cuda, B)[0], X=up(torch, cuda, X0)[0], rtol=RTOL, atol=atol, max_iter=1000, check_every=5, **P.kw())
    assert_solved(st, X, dict(names=["1e3 b", "b", "1e-3 b"], want=want))
    plan.destroy()
    P.destroy()


def test_refusals_come_before_any_launch(env):
    S, torch, cuda = env
    E = S.SblasError
    n, rp, ci, val = KN.convection_diffusion(8)
    s = 5
    drp, dci, dval = up(torch, cuda, rp, ci, val)
    for bad in (0, 65):
        with pytest.raises(E, match="right-hand sides"):
            S.GmresMultiPlan(n, drp, dci, bad)
        with pytest.raises(E, match="restart must be an integer"):
            S.GmresMultiPlan(n, drp, dci, s, restart=bad)
    ilu = S.Ilu0Plan(n, drp, dci)
    ilu.factor(dval)
    cheb = S.ChebyshevPlan(n, drp, dci)
    for precond, what in ((ilu, "ilu0"), (cheb, "chebyshev"), ("ilu0", "ilu0"), ("amg", "amg"), ("chebyshev", "chebyshev")):
        with pytest.raises(E, match="the %s preconditioner has no multi-column apply" % what):
            S.GmresMultiPlan(n, drp, dci, s, precond=precond)
    L = S.lib()
    h = C.c_void_p()
    create = lambda width, restart, kind, lo=None, hi=None: L.sblas_hip_gmres_multi_plan_create(
        -1, None, n, dci.numel(), drp.data_ptr(), dci.data_ptr(), width, restart, kind, lo, hi, C.byref(h))
    lower, upper = ilu.solvers()
    for args in ((0, 5, 0), (65, 5, 0), (s, 0, 0), (s, 65, 0), (s, 5, S.PRECOND_CHEBYSHEV), (s, 5, S.PRECOND_CHEBYSHEV, cheb.handle), (s, 5, 7),
                 (s, 5, S.PRECOND_AMG), (s, 5, S.PRECOND_ILU0), (s, 5, S.PRECOND_ILU0, lower.handle), (s, 5, S.PRECOND_NONE, lower.handle),
                 (s, 5, S.PRECOND_ILU0, upper.handle, lower.handle)):
        assert create(*args) == 1 and not h.value, args
    # plans of another structure
    other = KN.convection_diffusion(7)
    orp, oci = up(torch, cuda, other[1], other[2])
    oilu = S.Ilu0Plan(other[0], orp, oci)
    oilu.factor(up(torch, cuda, other[3])[0])
    with pytest.raises(E, match="another structure"):
        S.GmresMultiPlan(n, drp, dci, s, precond=oilu.solvers())
    oamg = S.AmgPlan(other[0], orp, oci)
    with pytest.raises(E, match="another structure"):
        S.GmresMultiPlan(n, drp, dci, s, precond=oamg)
    assert create(s, 5, S.PRECOND_AMG, oamg.handle) == 1 and not h.value
    # an AmgPlan set up with the Chebyshev smoother is seated, and refused at start
    amg = S.AmgPlan(n, drp, dci)
    amg.setup(dval, smoother="chebyshev")
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=cuda)
    B = torch.ones((n, s), dtype=torch.float64, device=cuda)
    X = torch.full((n, s), SENTINEL, dtype=torch.float64, device=cuda)
    with_cheb = S.GmresMultiPlan(n, drp, dci, s, precond=amg)
    with pytest.raises(E, match="Chebyshev smoother has no block cycle"):
        with_cheb.start(dval, B, X)
    with_cheb.destroy()
    pair = S.GmresMultiPlan(n, drp, dci, s, precond=ilu.solvers())
    with pytest.raises(E, match="lu"):
        pair.start(dval, B, X)                                               # the factor is missing
    pair.destroy()
    plan = S.GmresMultiPlan(n, drp, dci, s, precond="jacobi")
    dinv = torch.full((n,), 0.25, dtype=torch.float64, device=cuda)
    with pytest.raises(E):
        plan.iterate(1)                                                      # before start
    with pytest.raises(E):
        plan.status()
    wide = z(n, 2 * s)
    cases = [
        ("dinv", dict(B=B, X=X)),                                            # Jacobi without dinv
        ("tensor", dict(B=z(n, s + 1), X=X, dinv=dinv)),                     # another width
        ("row-major", dict(B=B, X=torch.as_strided(z(n * s), (n, s), (s - 1, 1)), dinv=dinv)),     # ld < s
        ("row-major", dict(B=z(s, n).t(), X=X, dinv=dinv)),                  # column-major
        ("float64", dict(B=B.float(), X=X, dinv=dinv)),
        ("float64", dict(B=B, X=X, dinv=dinv.float())),
        ("GPU tensor", dict(B=B.cpu(), X=X, dinv=dinv)),
        ("overlap", dict(B=B, X=B, dinv=dinv)),
        ("overlap", dict(B=wide[:, :s], X=wide[:, s:], dinv=dinv)),              # interleaved column slices of one tensor
        ("rtol", dict(B=B, X=X, dinv=dinv, rtol=-1.0)),
        ("rtol", dict(B=B, X=X, dinv=dinv, atol=float("nan"))),
        ("rtol", dict(B=B, X=X, dinv=dinv, max_iter=-1)),
    ]
    for match, kw in cases:
        with pytest.raises(E, match=match):
            plan.start(dval, **kw)
    if torch.cuda.device_count() > 1:
        with pytest.raises(E):
            plan.start(dval, B.to("cuda:1"), X, dinv=dinv)
    # the library itself: ld < s, X overlapping B, a NaN tolerance
    start = lambda ldb, ldx, xptr, rtol: L.sblas_hip_gmres_multi_start(plan.handle, None, dval.data_ptr(), dinv.data_ptr(), B.data_ptr(), ldb, xptr,
                                                                       ldx, rtol, 0.0, 10)
    assert start(s - 1, s, X.data_ptr(), RTOL) == 1 and start(s, s - 1, X.data_ptr(), RTOL) == 1
    assert start(s, s, B.data_ptr() + 8, RTOL) == 1 and start(s, s, X.data_ptr(), float("nan")) == 1
    with pytest.raises(E):
        plan.iterate(1)                                                      # still not started
    torch.cuda.synchronize()
    assert (X == SENTINEL).all().item() and (B == 1.0).all().item()           # nothing was launched
    for p in (plan, ilu, cheb, oilu, oamg, amg):
        p.destroy()
