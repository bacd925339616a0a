"""The multi-right-hand-side solvers composed from their parts: PCG and BiCGStab as lockstep loops over a numpy block of
s columns with per-column state and the per-column freeze, in the order csrc/krylov_multi.hip enqueues its launches.  A
loop takes three callables: matvec(V) on an (n, s) block (one product for all columns, frozen ones included -- with the
device's SpMM its bits may depend on every column of V, so the loop keeps the frozen columns of every block exactly what
the device keeps), dot(a, b) on two columns and apply(v) (M^-1 v) on one.  The scalar steps are Python floats, one IEEE
operation each, in solver_compose.py's order; a column's status, count, |r|, |b|, alpha, beta, omega and breakdown are
what that file's single loops return.  With host parts that are separable by column (krylov_numerics.matvec per column,
dot_np) a lockstep loop must equal s single loops bit for bit; with device parts (an SpmmPlan, krylov_dot per column) it
is what a whole KrylovMultiPlan solve must equal.  No GPU call and no library call in here.

What the device does that shows here:
  start      every work block is zero; |b_j|; Q = A X0 (before a zero column's x is cleared); r_j, z_j of EVERY column
             (a zero b_j: x_j = r_j = z_j = 0); the first test; then p_j = z_j of the columns still running only
  iteration  every update touches the columns that are running when it is launched, no others; a column's scalar step
             changes nothing once it is not running; the product runs on whole blocks"""
import math

import numpy as np

import solver_compose as SC

RUNNING = "running"


class Column:
    """one column's scalar block"""

    def __init__(self, omega):
        self.status, self.it, self.rnorm, self.bnorm, self.tol = RUNNING, 0, 0.0, 0.0, 0.0
        self.alpha, self.beta, self.omega, self.rho, self.why, self.zero = 0.0, 0.0, omega, 0.0, None, False

    @property
    def running(self):
        return self.status == RUNNING

    def begin(self, bb, rtol, atol):
        self.bnorm = math.sqrt(bb)
        self.tol = SC.tolerance(rtol, atol, self.bnorm)
        self.zero = bb == 0.0
        if self.zero:
            self.status = "converged"

    def residual(self, rr, max_iter, count):
        """|r|, the count and the test; True when the recurrence goes on"""
        self.rnorm = math.sqrt(rr)
        if count:
            self.it += 1
        if self.rnorm <= self.tol:
            self.status = "converged"
        elif self.it >= max_iter:
            self.status = "limit"
        else:
            return True
        return False

    def break_down(self, why):
        self.status, self.why = "breakdown", why

    def solved(self, x):
        return SC.Solved(x, self.it, self.rnorm, self.status, self.bnorm, self.alpha, self.beta, self.omega, self.why)


def _empty(X0, omega):
    return [SC.Solved(X0[:, j].copy(), 0, 0.0, "converged", 0.0, 0.0, 0.0, 0.0) for j in range(X0.shape[1])]


def _start(matvec, dot, B, X0, rtol, atol, omega):
    s = B.shape[1]
    cols = [Column(omega) for _ in range(s)]
    for j, c in enumerate(cols):
        c.begin(dot(B[:, j], B[:, j]), rtol, atol)
    X = X0.copy()
    Q = matvec(X)                                                            # the product sees the guesses as they came
    R = np.zeros_like(X)
    for j, c in enumerate(cols):
        if c.zero:
            X[:, j] = 0.0
        else:
            R[:, j] = B[:, j] - Q[:, j]
    return cols, X, R


def composed_pcg_multi(matvec, apply, dot, B, X0, rtol, max_iter, atol=0.0):
    """-> a list of solver_compose.Solved, one a column"""
    n, s = B.shape
    if n == 0:
        return _empty(X0, 0.0)
    with np.errstate(all="ignore"):
        cols, X, R = _start(matvec, dot, B, X0, rtol, atol, 0.0)
        Z, P = np.zeros_like(R), np.zeros_like(R)
        for j, c in enumerate(cols):
            if not c.zero:
                Z[:, j] = apply(R[:, j])
            rr, rz = dot(R[:, j], R[:, j]), dot(R[:, j], Z[:, j])
            if c.running:
                c.rho = rz
                c.residual(rr, max_iter, False)
        for j, c in enumerate(cols):
            if c.running:
                P[:, j] = Z[:, j]
        while any(c.running for c in cols):
            Q = matvec(P)
            for j, c in enumerate(cols):
                if c.running:
                    pq = dot(P[:, j], Q[:, j])
                    if SC.bad_denominator(pq):
                        c.break_down(SC.DENOM_PQ)
                    else:
                        c.alpha = c.rho / pq
            for j, c in enumerate(cols):
                if not c.running:
                    continue
                X[:, j] = X[:, j] + c.alpha * P[:, j]
                R[:, j] = R[:, j] - c.alpha * Q[:, j]
                Z[:, j] = apply(R[:, j])
                rr, rz = dot(R[:, j], R[:, j]), dot(R[:, j], Z[:, j])
                if c.residual(rr, max_iter, True):
                    if SC.bad_denominator(c.rho):
                        c.break_down(SC.DENOM_RHO)
                    else:
                        c.beta, c.rho = rz / c.rho, rz
            for j, c in enumerate(cols):
                if c.running:
                    P[:, j] = Z[:, j] + c.beta * P[:, j]
    return [c.solved(X[:, j].copy()) for j, c in enumerate(cols)]


def composed_bicgstab_multi(matvec, apply, dot, B, X0, rtol, max_iter, atol=0.0):
    """-> a list of solver_compose.Solved, one a column"""
    n, s = B.shape
    if n == 0:
        return _empty(X0, 0.0)
    with np.errstate(all="ignore"):
        cols, X, R = _start(matvec, dot, B, X0, rtol, atol, 1.0)
        RH = R.copy()
        P, V, S, T, PH, SH = (np.zeros_like(R) for _ in range(6))
        for j, c in enumerate(cols):
            rr = dot(R[:, j], R[:, j])
            if c.running:
                c.rho = rr
                c.residual(rr, max_iter, False)
        while any(c.running for c in cols):
            for j, c in enumerate(cols):
                if c.running:
                    P[:, j] = R[:, j] + c.beta * (P[:, j] - c.omega * V[:, j])
                    PH[:, j] = apply(P[:, j])
            V = matvec(PH)
            for j, c in enumerate(cols):
                if c.running:
                    rv = dot(RH[:, j], V[:, j])
                    if SC.bad_denominator(rv):
                        c.break_down(SC.DENOM_RV)
                    else:
                        c.alpha = c.rho / rv
            for j, c in enumerate(cols):
                if c.running:
                    S[:, j] = R[:, j] - c.alpha * V[:, j]
                    SH[:, j] = apply(S[:, j])
            T = matvec(SH)
            for j, c in enumerate(cols):
                if c.running:
                    ts, tt, ss = dot(T[:, j], S[:, j]), dot(T[:, j], T[:, j]), dot(S[:, j], S[:, j])
                    if tt == 0.0 and math.sqrt(ss) <= c.tol:                # the half step is the answer: omega = 0 takes it
                        c.omega = 0.0
                    elif SC.bad_denominator(tt):
                        c.break_down(SC.DENOM_TT)
                    else:
                        c.omega = ts / tt
            for j, c in enumerate(cols):
                if not c.running:
                    continue
                X[:, j] = (X[:, j] + c.alpha * PH[:, j]) + c.omega * SH[:, j]
                R[:, j] = S[:, j] - c.omega * T[:, j]
                rr, rhr = dot(R[:, j], R[:, j]), dot(RH[:, j], R[:, j])
                if c.residual(rr, max_iter, True):
                    if SC.bad_denominator(c.rho):
                        c.break_down(SC.DENOM_RHO)
                    elif SC.bad_denominator(c.omega):
                        c.break_down(SC.DENOM_OMEGA)
                    else:
                        c.beta, c.rho = (rhr / c.rho) * (c.alpha / c.omega), rhr
    return [c.solved(X[:, j].copy()) for j, c in enumerate(cols)]


# ---- the columns of the solver cases ------------------------------------------------------------------------------------
WARM = (1e-3, 1e-6, 1e-9)


def columns(n, matvec1, seed=11, k=None):
    """(B, X0, names): the seven kinds of column of the multi-right-hand-side cases, nine columns in all -- a random
    column, e_k, a zero column, 1e6 random, 1e-150 random, a column with one NaN, and b = A x* from the guesses x* + eps
    noise for eps in WARM.  matvec1(v): A v on one host vector."""
    rng = np.random.default_rng(seed)
    k = n // 3 if k is None else k
    B, X0, names = [], [], []

    def add(name, b, x0=None):
        names.append(name), B.append(b), X0.append(np.zeros(n) if x0 is None else x0)

    add("random", rng.standard_normal(n))
    e = np.zeros(n)
    e[k] = 1.0
    add("e_k", e)
    add("zero", np.zeros(n), 0.1 * rng.standard_normal(n))                  # x is cleared, whatever the guess
    add("large", 1e6 * rng.standard_normal(n))
    add("tiny", 1e-150 * rng.standard_normal(n))
    b = rng.standard_normal(n)
    b[(2 * n) // 3] = np.nan
    add("nan", b)
    for eps in WARM:
        xs = rng.standard_normal(n)
        add("warm %g" % eps, matvec1(xs), xs + eps * rng.standard_normal(n))
    return np.ascontiguousarray(np.stack(B, axis=1)), np.ascontiguousarray(np.stack(X0, axis=1)), names


def spread_ok(iterations):
    """the spread that exercises the freeze: at least four distinct stopping iterations among the columns, the largest at
    least twice the smallest non-zero one"""
    its = sorted(set(int(i) for i in iterations))
    pos = [i for i in its if i > 0]
    return len(its) >= 4 and bool(pos) and pos[-1] >= 2 * pos[0]
