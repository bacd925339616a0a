"""The solvers composed from their parts, in one place: PCG, BiCGStab and GMRES(m) as loops over four callables on numpy
vectors -- matvec(v), apply(v) (M^-1 v), dot(a, b) and, for GMRES, dots(V, w) -- with every scalar step in Python floats
(one IEEE operation each) in the order csrc/krylov.hip's and csrc/gmres.hip's folds take them.  With device parts (Parts
below: SpmvPlan or the unplanned SpMV, Ilu0Plan.apply / AmgPlan.apply / a numpy product with dinv, the pinned dot) a loop
is what a whole solve on the device must equal on the bits; with host parts (krylov_numerics.matvec, krylov_dot_ref, a
numpy apply) it runs without a GPU.  No GPU call and no library call of its own in here: Parts is handed (sblas, torch,
device) and the loops are handed callables.

The scalar steps, as the folds write them:
  tolerance     t = rtol * |b|, tol = t if t >= atol else atol; b == 0 is x = 0, converged at iteration 0, nothing divided
                (n == 0 launches nothing: converged, and every scalar of the status reads 0)
  first test    |r0| <= tol is converged, else 0 >= max_iter is the limit
  a denominator is bad when it is zero or not finite (bad_denominator)
  PCG           (p, q) before alpha; after the residual test the old rho before beta
  BiCGStab      (r^, v) before alpha; omega = 0 when (t, t) == 0 and |s| <= tol, before (t, t) is tested; after the
                residual test rho, then omega, before beta
A breakdown leaves x, the count, |r|, alpha, beta and omega as they stood and names the denominator (KRYLOV_DENOM)."""
import math

import numpy as np

import gmres_numerics as GN

DENOM_PQ, DENOM_RHO, DENOM_RV, DENOM_TT, DENOM_OMEGA = "(p, q)", "rho", "(r^, v)", "(t, t)", "omega"    # KRYLOV_DENOM's names


class Solved(tuple):
    """(x, iterations, rnorm, status) as the composed Krylov loops always returned them, with the rest of the device's
    status as attributes: bnorm, alpha, beta, omega, breakdown (and the four again, by name)"""

    def __new__(cls, x, iterations, rnorm, status, bnorm, alpha, beta, omega, breakdown=None):
        self = super().__new__(cls, (x, iterations, rnorm, status))
        self.x, self.iterations, self.rnorm, self.status = x, iterations, rnorm, status
        self.bnorm, self.alpha, self.beta, self.omega, self.breakdown = bnorm, alpha, beta, omega, breakdown
        return self

    def asdict(self):
        return dict(x=self.x, iterations=self.iterations, rnorm=self.rnorm, status=self.status, bnorm=self.bnorm, alpha=self.alpha,
                    beta=self.beta, omega=self.omega, breakdown=self.breakdown)


def bad_denominator(d):
    return d == 0.0 or not math.isfinite(d)


def tolerance(rtol, atol, bnorm):
    t = rtol * bnorm
    return t if t >= atol else atol


def composed_pcg(matvec, apply, dot, b, x0, rtol, max_iter, atol=0.0):
    if len(b) == 0:                                                          # n == 0: nothing runs, every scalar reads 0
        return Solved(x0.copy(), 0, 0.0, "converged", 0.0, 0.0, 0.0, 0.0)
    with np.errstate(all="ignore"):
        bb = dot(b, b)
        bnorm = math.sqrt(bb)
        tol = tolerance(rtol, atol, bnorm)
        alpha = beta = 0.0
        if bb == 0.0:
            return Solved(np.zeros_like(x0), 0, 0.0, "converged", bnorm, alpha, beta, 0.0)
        x = x0.copy()
        it = 0
        r = b - matvec(x)
        rnorm = math.sqrt(dot(r, r))
        done = lambda status, why=None: Solved(x, it, rnorm, status, bnorm, alpha, beta, 0.0, why)
        if rnorm <= tol:
            return done("converged")
        if it >= max_iter:
            return done("limit")
        z = apply(r)
        rho = dot(r, z)
        p = z.copy()
        while True:
            q = matvec(p)
            pq = dot(p, q)
            if bad_denominator(pq):
                return done("breakdown", DENOM_PQ)
            alpha = rho / pq
            x = x + alpha * p
            r = r - alpha * q
            rnorm, it = math.sqrt(dot(r, r)), it + 1
            if rnorm <= tol:
                return done("converged")
            if it >= max_iter:
                return done("limit")
            z = apply(r)
            rho_new = dot(r, z)
            if bad_denominator(rho):
                return done("breakdown", DENOM_RHO)
            beta, rho = rho_new / rho, rho_new
            p = z + beta * p


def composed_bicgstab(matvec, apply, dot, b, x0, rtol, max_iter, atol=0.0):
    if len(b) == 0:                                                          # n == 0: nothing runs, every scalar reads 0
        return Solved(x0.copy(), 0, 0.0, "converged", 0.0, 0.0, 0.0, 0.0)
    with np.errstate(all="ignore"):
        bb = dot(b, b)
        bnorm = math.sqrt(bb)
        tol = tolerance(rtol, atol, bnorm)
        alpha, beta, omega = 0.0, 0.0, 1.0
        if bb == 0.0:
            return Solved(np.zeros_like(x0), 0, 0.0, "converged", bnorm, alpha, beta, omega)
        x = x0.copy()
        it = 0
        r = b - matvec(x)
        rho = dot(r, r)
        rnorm = math.sqrt(rho)
        done = lambda status, why=None: Solved(x, it, rnorm, status, bnorm, alpha, beta, omega, why)
        if rnorm <= tol:
            return done("converged")
        if it >= max_iter:
            return done("limit")
        rh, p, v = r.copy(), np.zeros_like(r), np.zeros_like(r)
        while True:
            p = r + beta * (p - omega * v)
            ph = apply(p)
            v = matvec(ph)
            rv = dot(rh, v)
            if bad_denominator(rv):
                return done("breakdown", DENOM_RV)
            alpha = rho / rv
            s = r - alpha * v
            sh = apply(s)
            t = matvec(sh)
            tt = dot(t, t)
            if tt == 0.0 and math.sqrt(dot(s, s)) <= tol:                  # the half step is the answer: omega = 0 takes it
                omega = 0.0
            elif bad_denominator(tt):
                return done("breakdown", DENOM_TT)
            else:
                omega = dot(t, s) / tt
            x = (x + alpha * ph) + omega * sh
            r = s - omega * t
            rnorm, it = math.sqrt(dot(r, r)), it + 1
            if rnorm <= tol:
                return done("converged")
            if it >= max_iter:
                return done("limit")
            rho_new = dot(rh, r)
            if bad_denominator(rho):
                return done("breakdown", DENOM_RHO)
            if bad_denominator(omega):
                return done("breakdown", DENOM_OMEGA)
            beta, rho = (rho_new / rho) * (alpha / omega), rho_new


def composed_gmres(matvec, apply, dot, dots, b, x0, restart, rtol, max_iter, atol=0.0):
    """GMRES(restart) in the written order (gmres_numerics restates the scalar steps); dots(V, w) -> [(v_i, w)] by the single
    pinned dot -> dict(x, status, iterations, restarts, rnorm, bnorm, columns, breakdown)"""
    bb = dot(b, b)
    bnorm = math.sqrt(bb)
    tol = tolerance(rtol, atol, bnorm)
    x = x0.copy()
    it = restarts = k = 0
    result = lambda status, rnorm, why=None: dict(x=x, status=status, iterations=it, restarts=restarts, rnorm=rnorm, bnorm=bnorm, columns=k,
                                                  breakdown=why)
    if bb == 0.0:
        x = np.zeros_like(x)
        return result(GN.CONVERGED, 0.0)
    with np.errstate(all="ignore"):
        r = b - matvec(x)
    beta = math.sqrt(dot(r, r))
    status = GN.begin_py(beta, tol, it, max_iter)
    rnorm = beta
    while status == GN.RUNNING:
        with np.errstate(all="ignore"):
            V = [r / beta]
        g, c, s = [beta], [], []
        R = np.zeros((restart, restart))
        k, why = 0, None
        for j in range(restart):
            with np.errstate(all="ignore"):
                w = matvec(apply(V[j]))
                h = dots(V, w)
                for i in range(j + 1):
                    w = w - h[i] * V[i]
                c2 = dots(V, w)
                h = [h[i] + c2[i] for i in range(j + 1)]
                for i in range(j + 1):
                    w = w - c2[i] * V[i]
            eta = math.sqrt(dot(w, w))
            step = GN.step_py(j, h, eta, c, s, g, tol, it, max_iter)
            status = step["status"]
            if status == GN.BREAKDOWN:                                       # column j is dropped; the ones before it stay
                why = step["breakdown"]
                break
            c, s, g, it, rnorm, k = step["c"], step["s"], step["g"], step["iterations"], step["rnorm"], j + 1
            R[:k, j] = step["rcol"]
            if status != GN.RUNNING:
                break
            with np.errstate(all="ignore"):
                V.append(w / eta)
        if k:                                                                # the close: x = x + M^-1 (V y)
            with np.errstate(all="ignore"):
                y = GN.solve_py(R[:k, :k].tolist(), g)
                u = y[0] * V[0]
                for i in range(1, k):
                    u = u + y[i] * V[i]
                x = x + apply(u)
        if status != GN.RUNNING:
            return result(status, rnorm, why)
        with np.errstate(all="ignore"):
            r = b - matvec(x)                                                # the restart, on the true residual
        beta = math.sqrt(dot(r, r))
        restarts, k, rnorm = restarts + 1, 0, beta
        status = GN.begin_py(beta, tol, it, max_iter)
    return result(status, rnorm, "beta" if status == GN.BREAKDOWN else None)


# ---- the device's parts ---------------------------------------------------------------------------------------------------
AMG_KINDS = dict(amg=dict(), amg_smoothed=dict(prolongator="smoothed"), amg_device=dict(aggregation="device"))


def stored_diagonal(rp, ci):
    """the place of every row's stored diagonal (sorted rows that store one: ilu0_numerics.check's diag_pos)"""
    row = np.repeat(np.arange(len(rp) - 1), np.diff(np.asarray(rp, np.int64)))
    dpos = np.flatnonzero(np.asarray(ci, np.int64) == row)
    assert len(dpos) == len(rp) - 1 and np.array_equal(row[dpos], np.arange(len(rp) - 1)), "every row stores one diagonal"
    return dpos


def up(torch, cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


class Parts:
    """The pieces a composed loop is built from, on the device: A v by SpmvPlan (planned) or the unplanned SpMV, M^-1 v by
    Ilu0Plan.apply, AmgPlan.apply or a numpy product with dinv, the pinned dot; vectors live in numpy between them.
    env: (sblas, torch, device).  precond: None, "jacobi" (dinv: the caller's, or 1 / the stored diagonal), "ilu0", or a
    key of AMG_KINDS.  revalue(val) takes new values on the same structure: the factor and the AMG are set up again."""

    def __init__(self, env, n, rp, ci, val, precond=None, planned=True, dinv=None):
        S, torch, cuda = self.env = env
        self.n, self.precond, self.rp, self.ci = n, precond, rp, ci
        self.drp, self.dci = up(torch, cuda, rp, ci)
        self.spmv = S.SpmvPlan(n, n, self.drp, self.dci) if planned else None
        self.ilu = self.amg = None
        self.given_dinv = dinv
        if precond == "ilu0":
            self.ilu = S.Ilu0Plan(n, self.drp, self.dci)
        elif precond in AMG_KINDS:
            self.amg = S.AmgPlan(n, self.drp, self.dci, **AMG_KINDS[precond])
        elif precond not in (None, "jacobi"):
            raise KeyError(precond)
        self._cols = []
        self.revalue(val)

    def revalue(self, val):
        S, torch, cuda = self.env
        self.val = val
        self.dval, = up(torch, cuda, val)
        self.lu = self.dinv = self.ddinv = None
        if self.ilu is not None:
            self.lu = self.ilu.factor(self.dval)
        elif self.amg is not None:
            self.amg.setup(self.dval)
        elif self.precond == "jacobi":
            self.dinv = np.asarray(self.given_dinv, np.float64) if self.given_dinv is not None else 1.0 / val[stored_diagonal(self.rp, self.ci)]
            self.ddinv, = up(torch, cuda, self.dinv)

    def handle(self):
        """what KrylovPlan and GmresPlan take as precond"""
        return self.ilu if self.ilu is not None else self.amg if self.amg is not None else self.precond

    def plan(self, how):
        """a KrylovPlan of method `how` ("pcg", "bicgstab"), or a GmresPlan of restart `how` (an integer)"""
        S = self.env[0]
        if isinstance(how, str):
            return S.KrylovPlan(self.n, self.drp, self.dci, method=how, spmv_plan=self.spmv, precond=self.handle())
        return S.GmresPlan(self.n, self.drp, self.dci, restart=how, spmv_plan=self.spmv, precond=self.handle())

    def kw(self):
        return dict(lu=self.lu, dinv=self.ddinv)

    def matvec(self, v):
        S, torch, cuda = self.env
        dv, = up(torch, cuda, v)
        q = torch.empty_like(dv)
        if self.spmv is not None:
            self.spmv(self.dval, dv, 1.0, 0.0, q)
        else:
            S.spmv(self.n, self.n, self.drp, self.dci, self.dval, dv, 1.0, 0.0, q)
        return q.cpu().numpy()

    def apply(self, v):
        S, torch, cuda = self.env
        if self.ilu is not None:
            return self.ilu.apply(self.lu, up(torch, cuda, v)[0]).cpu().numpy()
        if self.amg is not None:
            return self.amg.apply(up(torch, cuda, v)[0]).cpu().numpy()
        return self.dinv * v if self.precond == "jacobi" else v

    def dot(self, a, b):
        S, torch, cuda = self.env
        return float(S.krylov_dot(*up(torch, cuda, a, b)).cpu().numpy()[0])

    def dots(self, V, w):
        """[(v_i, w)] by the single pinned dot, one call a column; a column met before (the same array at the same place
        in V) is not sent again"""
        S, torch, cuda = self.env
        keep = 0
        while keep < min(len(V), len(self._cols)) and self._cols[keep][0] is V[keep]:
            keep += 1
        del self._cols[keep:]
        for v in V[keep:]:
            self._cols.append((v, up(torch, cuda, v)[0]))
        dw, = up(torch, cuda, w)
        out = torch.empty(len(V), dtype=torch.float64, device=cuda)
        for i in range(len(V)):
            S.krylov_dot(self._cols[i][1], dw, out=out[i:i + 1])
        return [float(v) for v in out.cpu().numpy()]

    def destroy(self):
        self._cols = []
        for p in (self.spmv, self.ilu, self.amg):
            if p is not None:
                p.destroy()
        self.spmv = self.ilu = self.amg = None
