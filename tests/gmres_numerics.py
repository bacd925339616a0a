"""What the GMRES tests share: the scalar step and the back substitution restated in Python floats in the written order
(include/sblas_hip.h), and a plain float64 GMRES(m) on the host that "it solves" is held against.  No GPU and no
library call in here."""
import math

import numpy as np

import krylov_numerics as KN

RUNNING, CONVERGED, BREAKDOWN, LIMIT = "running", "converged", "breakdown", "limit"


def step_py(j, h, eta, c, s, g, tol, iterations, max_iter):
    """The scalar step of Arnoldi step j, each operation rounded on its own (a Python float operation is one IEEE
    operation).  h: j + 1 floats; c, s: at least j; g: at least j + 1.  Nothing given is changed.
    -> dict(status, h, c, s, g, rcol, iterations, rnorm, breakdown) shaped as sblas.gmres_step_ref's"""
    h, c, s, g = [float(v) for v in h], [float(v) for v in c[:j]], [float(v) for v in s[:j]], [float(v) for v in g[:j + 1]]
    eta = float(eta)
    for i in range(j):
        t = c[i] * h[i] + s[i] * h[i + 1]
        h[i + 1] = (-s[i]) * h[i] + c[i] * h[i + 1]
        h[i] = t
    q = h[j] * h[j] + eta * eta
    d = math.sqrt(q) if q >= 0.0 else float("nan")                          # q is NaN or >= 0; math.sqrt(inf) = inf
    if d == 0.0 or not math.isfinite(d):
        return dict(status=BREAKDOWN, h=h, c=c, s=s, g=g, rcol=None, iterations=iterations, rnorm=None, breakdown="givens")
    c.append(h[j] / d)
    s.append(eta / d)
    rcol = h[:j] + [d]
    g.append((-s[j]) * g[j])
    g[j] = c[j] * g[j]
    rnorm = abs(g[j + 1])
    iterations += 1
    status = CONVERGED if rnorm <= tol else LIMIT if iterations >= max_iter else RUNNING
    return dict(status=status, h=h, c=c, s=s, g=g, rcol=rcol, iterations=iterations, rnorm=rnorm, breakdown=None)


def solve_py(R, g):
    """y from R y = g over k = len(R) columns: for i = k - 1 .. 0: t = g_i; for l = i + 1 .. k - 1 ascending
    t = t - R_il y_l; y_i = t / R_ii.  R[i][l] row by row."""
    k = len(R)
    y = [0.0] * k
    with np.errstate(all="ignore"):
        for i in range(k - 1, -1, -1):
            t = np.float64(g[i])
            for l in range(i + 1, k):
                t = t - np.float64(R[i][l]) * np.float64(y[l])
            y[i] = float(t / np.float64(R[i][i]))                          # numpy scalars: a zero pivot gives inf / nan, no exception
    return np.array(y)


def begin_py(beta, tol, iterations, max_iter):
    """the first residual of a cycle: the test, the limit, then the breakdown"""
    if beta <= tol:
        return CONVERGED
    if iterations >= max_iter:
        return LIMIT
    return RUNNING if math.isfinite(beta) else BREAKDOWN


def host_gmres(n, rp, ci, val, b, x0, restart, rtol, limit=1000, precond=None):
    """Plain right-preconditioned GMRES(restart) in float64 with CGS2 and np.dot: the yardstick of "it solves".
    precond: a function v -> M^-1 v, or None.  -> (steps, restarts, x at its own stop)"""
    M = precond if precond is not None else (lambda v: v)
    x = x0.copy()
    tol = rtol * np.linalg.norm(b)
    steps = restarts = 0
    while True:
        r = b - KN.matvec(n, rp, ci, val, x)
        beta = np.linalg.norm(r)
        if beta <= tol or steps >= limit:
            return steps, restarts, x
        V = np.zeros((restart + 1, n))
        H = np.zeros((restart + 1, restart))
        V[0] = r / beta
        k = 0
        done = False
        for j in range(restart):
            w = KN.matvec(n, rp, ci, val, M(V[j]))
            h = V[:j + 1] @ w
            w = w - V[:j + 1].T @ h
            c2 = V[:j + 1] @ w
            w = w - V[:j + 1].T @ c2
            H[:j + 1, j] = h + c2
            H[j + 1, j] = np.linalg.norm(w)
            k, steps = j + 1, steps + 1
            e1 = np.zeros(k + 1)
            e1[0] = beta
            y, res = np.linalg.lstsq(H[:k + 1, :k], e1, rcond=None)[:2]
            rn = np.linalg.norm(H[:k + 1, :k] @ y - e1)
            if rn <= tol or steps >= limit or H[j + 1, j] == 0.0:
                done = True
                break
            V[j + 1] = w / H[j + 1, j]
        x = x + M(V[:k].T @ y)
        if done:
            return steps, restarts, x
        restarts += 1
