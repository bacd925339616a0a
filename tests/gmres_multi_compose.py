"""Multi-right-hand-side GMRES(m) composed from its parts: the lockstep loop over a numpy block of s columns with per-column
state and the per-column freeze, in the order csrc/gmres_multi.hip enqueues its launches.  The conventions are
multi_compose.py's: matvec(V) on an (n, s) block is one product for all columns, frozen ones included (with the device's
SpMM its bits may depend on every column of V, so the loop keeps the frozen columns of the block the product reads
exactly what the device keeps); dot(a, b) on two columns; apply(v) (M^-1 v) on one.  The scalar steps are
gmres_numerics' (step_py, begin_py, solve_py), and a column's result is the dict solver_compose.composed_gmres returns:
x, status, iterations, restarts, rnorm, bnorm, columns, breakdown.  With host parts that are separable by column the
loop must equal s single loops field by field; with device parts (an SpmmPlan, krylov_dot per column) it is what a whole
GmresMultiPlan solve must equal.  No GPU call and no library call in here.

What the device does that shows here:
  start      every work block is zero; |b_c|; Q = A X0 (before a zero column's x is cleared); r_c, the first test, and
             v_0 and the operand column of the columns that run only
  a step     one product of the operand block P -- column c of it is M^-1 of column c's newest basis vector, written
             when that vector is, so a frozen column keeps its last one (an applied M^-1 recomputes it to the same bits)
  a close    acts for a column that is pending once its cycle is full or it no longer runs; when it acts cannot reach
             another column, so here a column that stops is closed at once
  a restart  one product of X, whole, behind the closes; only the running columns take their residual from it"""
import math

import numpy as np

import gmres_numerics as GN
import solver_compose as SC


class Column:
    """one column's scalar block and small matrices"""

    def __init__(self, restart):
        self.m = restart
        self.status, self.it, self.restarts, self.k = GN.RUNNING, 0, 0, 0
        self.rnorm, self.bnorm, self.tol, self.why, self.zero, self.pending = 0.0, 0.0, 0.0, None, False, False
        self.V, self.g, self.c, self.s, self.R = [], [], [], [], None

    @property
    def running(self):
        return self.status == GN.RUNNING

    def begin(self, r, dot, max_iter):
        """a cycle's first residual: the test, and v_0 when the column goes on -> v_0 or None"""
        beta = math.sqrt(dot(r, r))
        self.status = GN.begin_py(beta, self.tol, self.it, max_iter)
        self.rnorm, self.k = beta, 0
        if self.status == GN.BREAKDOWN:
            self.why = "beta"
        if not self.running:
            return None
        self.V, self.g, self.c, self.s, self.R = [r / beta], [beta], [], [], np.zeros((self.m, self.m))
        return self.V[0]

    def step(self, w, dot, max_iter):
        """Arnoldi step k on w = A M^-1 v_k, as solver_compose.composed_gmres takes it -> v_{k+1} or None"""
        j, V = self.k, self.V
        h = [dot(V[i], w) for i in range(j + 1)]
        for i in range(j + 1):
            w = w - h[i] * V[i]
        c2 = [dot(V[i], w) for i in range(j + 1)]
        h = [h[i] + c2[i] for i in range(j + 1)]
        for i in range(j + 1):
            w = w - c2[i] * V[i]
        eta = math.sqrt(dot(w, w))
        step = GN.step_py(j, h, eta, self.c, self.s, self.g, self.tol, self.it, max_iter)
        self.status = step["status"]
        if self.status == GN.BREAKDOWN:                                      # column j is dropped; the ones before it stay
            self.why = step["breakdown"]
            return None
        self.c, self.s, self.g, self.it, self.rnorm, self.k = step["c"], step["s"], step["g"], step["iterations"], step["rnorm"], j + 1
        self.R[:self.k, j] = step["rcol"]
        self.pending = True
        if not self.running:
            return None
        V.append(w / eta)
        return V[-1]

    def close(self, x, apply):
        """x + M^-1 (V y) over the finished columns"""
        k = self.k
        y = GN.solve_py(self.R[:k, :k].tolist(), self.g)
        u = y[0] * self.V[0]
        for i in range(1, k):
            u = u + y[i] * self.V[i]
        self.pending = False
        return x + apply(u)

    def result(self, x):
        return dict(x=x, status=self.status, iterations=self.it, restarts=self.restarts, rnorm=self.rnorm, bnorm=self.bnorm, columns=self.k,
                    breakdown=self.why)


def composed_gmres_multi(matvec, apply, dot, B, X0, restart, rtol, max_iter, atol=0.0):
    """-> a list of dicts, one a column, each what solver_compose.composed_gmres returns"""
    n, s = B.shape
    if n == 0:                                                               # nothing runs, every scalar reads 0
        return [dict(x=X0[:, c].copy(), status=GN.CONVERGED, iterations=0, restarts=0, rnorm=0.0, bnorm=0.0, columns=0, breakdown=None)
                for c in range(s)]
    cols = [Column(restart) for _ in range(s)]
    X = X0.copy()
    P = np.zeros_like(X)                                                     # the block the next product multiplies
    with np.errstate(all="ignore"):
        for c, col in enumerate(cols):
            bb = dot(B[:, c], B[:, c])
            col.bnorm = math.sqrt(bb)
            col.tol = SC.tolerance(rtol, atol, col.bnorm)
            col.zero = bb == 0.0
            if col.zero:
                col.status = GN.CONVERGED
        Q = matvec(X)                                                        # the product sees the guesses as they came
        for c, col in enumerate(cols):
            if col.zero:
                X[:, c] = 0.0
                continue
            v = col.begin(B[:, c] - Q[:, c], dot, max_iter)
            if v is not None:
                P[:, c] = apply(v)
        while any(col.running for col in cols):
            for j in range(restart):
                if not any(col.running for col in cols):
                    break
                W = matvec(P)
                for c, col in enumerate(cols):
                    if not col.running:
                        continue
                    assert col.k == j                                        # the running columns share the position
                    v = col.step(W[:, c].copy(), dot, max_iter)
                    if v is not None:
                        P[:, c] = apply(v)
            for c, col in enumerate(cols):                                   # the close: full cycles, and whoever stopped
                if col.pending:
                    X[:, c] = col.close(X[:, c], apply)
            if not any(col.running for col in cols):
                break
            Q = matvec(X)                                                    # the restart, on the true residuals
            for c, col in enumerate(cols):
                if not col.running:
                    continue
                col.restarts += 1
                v = col.begin(B[:, c] - Q[:, c], dot, max_iter)
                if v is not None:
                    P[:, c] = apply(v)
    return [col.result(X[:, c].copy()) for c, col in enumerate(cols)]
