"""What the eigenvalue plan's tests share (EigshPlan): the test matrices, Python restatements of the Jacobi
rule, the Ritz step and the rotation (held to the library's host references with ==), the whole method composed from the
library's own pieces on the device (the binding reference of the plan), and a plain float64 numpy thick-restart loop.

The matrices have SIMPLE extremal eigenvalues: a single-vector Lanczos method finds one copy of a multiple eigenvalue, so
the square-grid Laplacian and its like are no test of it."""
import math

import numpy as np

EPS = 2.0 ** -52
MAX_SWEEPS = 24
RUNNING, CONVERGED, BREAKDOWN, LIMIT = "running", "converged", "breakdown", "limit"


# ---------------------------------------------------------------------------------------------------------------------
# matrices: (n, rowptr, colidx, val) with int32 indices, and the dense copy
# ---------------------------------------------------------------------------------------------------------------------
def csr_of(dense):
    n = dense.shape[0]
    rowptr, colidx, val = [0], [], []
    for i in range(n):
        cols = np.nonzero(dense[i])[0]
        colidx.extend(cols.tolist()), val.extend(dense[i, cols].tolist())
        rowptr.append(len(colidx))
    return n, np.array(rowptr, np.int32), np.array(colidx, np.int32), np.array(val, np.float64)


def laplace_1d(n=200):
    A = np.zeros((n, n))
    i = np.arange(n)
    A[i, i] = 2.0
    A[i[:-1], i[:-1] + 1] = -1.0
    A[i[:-1] + 1, i[:-1]] = -1.0
    return A


def grid_2d(nx=24, ny=17, cx=1.0, cy=0.6):
    """the five-point grid with coefficient cx along x and cy along y: every eigenvalue is simple for these sizes"""
    n = nx * ny
    A = np.zeros((n, n))
    for y in range(ny):
        for x in range(nx):
            i = y * nx + x
            A[i, i] = 2.0 * cx + 2.0 * cy
            if x + 1 < nx:
                A[i, i + 1] = A[i + 1, i] = -cx
            if y + 1 < ny:
                A[i, i + nx] = A[i + nx, i] = -cy
    return A


def diagonal_random(n=500, per_row=4, scale=0.1, seed=7):
    """diag(1 .. n) plus a symmetric random pattern of about per_row entries a row, scaled"""
    rng = np.random.default_rng(seed)
    A = np.diag(np.arange(1.0, n + 1.0))
    for i in range(n):
        for j in rng.integers(0, n, per_row // 2):
            if i != j:
                A[i, j] = A[j, i] = scale * rng.standard_normal()
    return A


MATRICES = {"laplace": laplace_1d, "grid": grid_2d, "diagrand": diagonal_random}
# (matrix, which, k, ncv): the cases the issue names; LM on these positive definite matrices is LA's spectrum end
SIZES = [(4, 20), (6, 32), (10, 64)]
CASES = [(m, w, k, ncv) for m in ("laplace", "grid", "diagrand") for w in ("LA", "SA", "LM") for k, ncv in SIZES]
CASES += [("grid", "LA", 1, 8), ("grid", "SA", 1, 8)]
_dense = {}


def dense(name):
    if name not in _dense:
        _dense[name] = MATRICES[name]()
    return _dense[name]


def default_keep(k, ncv):
    return k + (ncv - k) // 2


def wanted(lam, which, k):
    """the k extremal values of the ascending spectrum lam in the order of which"""
    if which == "SA":
        return lam[:k]
    if which == "LA":
        return lam[::-1][:k]
    return lam[np.argsort(-np.abs(lam), kind="stable")][:k]


# ---------------------------------------------------------------------------------------------------------------------
# the Jacobi rule in Python floats and numpy element operations (each rounded on its own)
# ---------------------------------------------------------------------------------------------------------------------
def pair(M, r, i):
    ring = M - 1
    a, b = (r + i) % ring, (ring if i == 0 else (r - i + ring) % ring)
    return (a, b) if a < b else (b, a)


def rotation_py(app, aqq, apq):
    """-> (c, s, dpp, dqq, rotated)"""
    f = np.float64
    app, aqq, apq = f(app), f(aqq), f(apq)
    g, fp, fq = abs(apq), abs(app), abs(aqq)
    if g == 0.0 or (fp + g == fp and fq + g == fq):
        return f(1.0), f(0.0), app, aqq, False
    with np.errstate(all="ignore"):                                         # an overflow to inf is data here, as in C
        tau = (aqq - app) / (f(2.0) * apq)
        at = abs(tau)
        if at >= 2.0 ** 500:
            t = f(0.5) / tau
        else:
            t = f(1.0) / (at + np.sqrt(f(1.0) + tau * tau))
            if tau < 0.0:
                t = -t
        c = f(1.0) / np.sqrt(f(1.0) + t * t)
        d = t * apq
        return c, t * c, app - d, aqq + d, True


_jacobi_memo = {}


def jacobi_py(T):
    """-> (theta unordered, Y, sweeps) by the rule of include/sblas_hip_eigsh.h; T: (mm, mm) symmetric and finite.  The
    cases of one T (every `which`, both keeps) share one evaluation."""
    T = np.ascontiguousarray(T, np.float64)
    key = (T.shape, T.tobytes())
    if key not in _jacobi_memo:
        _jacobi_memo[key] = _jacobi_py(T)
    return tuple(np.copy(x) for x in _jacobi_memo[key])


def _jacobi_py(T):
    mm = T.shape[0]
    M = mm + (mm & 1)
    np_ = M // 2
    A = np.zeros((M, M))
    A[:mm, :mm] = T
    Y = np.zeros((M, M))
    Y[np.arange(mm), np.arange(mm)] = 1.0
    sweeps = 0
    for sweeps in range(MAX_SWEEPS + 1):
        if sweeps == MAX_SWEEPS:
            break
        rotated = False
        for r in range(M - 1):
            P, Q = np.zeros(np_, int), np.zeros(np_, int)
            Cc, Ss, Dp, Dq = np.zeros(np_), np.zeros(np_), np.zeros(np_), np.zeros(np_)
            for i in range(np_):
                P[i], Q[i] = pair(M, r, i)
                Cc[i], Ss[i], Dp[i], Dq[i], rot = rotation_py(A[P[i], P[i]], A[Q[i], Q[i]], A[P[i], Q[i]])
                rotated = rotated or rot

            def cols(X):
                out = X.copy()
                out[:, P] = Cc * X[:, P] - Ss * X[:, Q]
                out[:, Q] = Ss * X[:, P] + Cc * X[:, Q]
                return out

            def rows(X):
                out = X.copy()
                out[P, :] = Cc[:, None] * X[P, :] - Ss[:, None] * X[Q, :]
                out[Q, :] = Ss[:, None] * X[P, :] + Cc[:, None] * X[Q, :]
                return out

            of = np.zeros(M, int)
            of[P], of[Q] = np.arange(np_), np.arange(np_)
            upper = of[:, None] < of[None, :]
            new = np.where(upper, rows(cols(A)), cols(rows(A)))
            new[P, P], new[Q, Q], new[P, Q], new[Q, P] = Dp, Dq, 0.0, 0.0
            A = new
            Y = cols(Y)
        if not rotated:
            break
    return np.diag(A)[:mm].copy(), Y[:mm, :mm].copy(), sweeps


def order_py(theta, which):
    mm = len(theta)
    if which == "LA":
        return sorted(range(mm), key=lambda i: (-theta[i], i))
    if which == "SA":
        return sorted(range(mm), key=lambda i: (theta[i], i))
    return sorted(range(mm), key=lambda i: (-abs(theta[i]), i))


def ritz_py(T, beta, k, keep, which, rtol=1e-8, atol=0.0, restarts=0, max_restarts=300, invariant=False, status=RUNNING, eig=jacobi_py):
    """The whole Ritz step -> the keys of sblas_amd.eigsh_ritz_ref that a test compares.  eig: the eigensolver of T
    (jacobi_py is the library's; the plain numpy loop passes LAPACK's)."""
    T = np.asarray(T, np.float64)
    mm = T.shape[0]
    if status != RUNNING:
        return dict(status=status, restarts=restarts, act=0)
    if not np.isfinite(T).all():
        return dict(status=BREAKDOWN, breakdown="t", restarts=restarts, act=0, columns=mm)
    theta_u, Y, _ = eig(T)
    order = order_py(theta_u, which)
    theta = np.array([theta_u[i] for i in order])
    rho = np.array([abs(float(beta) * float(Y[mm - 1, i])) for i in order])
    met = 0
    for r in range(min(k, mm)):
        rel = rtol * abs(float(theta[r]))
        if rho[r] <= (rel if rel >= atol else atol):
            met += 1
    kk = min(keep, mm)
    Q = Y[:, order[:kk]].copy()
    Tn = np.zeros((mm, mm))
    Tn[np.arange(kk), np.arange(kk)] = theta[:kk]
    restarts += 1
    breakdown = None
    if mm < k:
        st, breakdown = BREAKDOWN, "invariant"
    elif met == k or invariant:
        st = CONVERGED
    elif restarts >= max_restarts:
        st = LIMIT
    else:
        st = RUNNING
    return dict(status=st, breakdown=breakdown, restarts=restarts, converged=met, columns=kk, mm=mm, kk=kk, act=1, theta=theta,
                residuals=rho, Q=Q, T=Tn, Y=Y)


def rotate_py(V, Q):
    """V: (mm + 1, n), Q: (mm, keep) -> the rotated copy, gmres_combine's order"""
    V = np.array(V, np.float64)
    mm, keep = Q.shape
    out = V.copy()
    for i in range(keep):
        acc = Q[0, i] * V[0]
        for l in range(1, mm):
            acc = acc + Q[l, i] * V[l]
        out[i] = acc
    out[keep] = V[mm]
    return out


def same_ritz(got, want, keys=("status", "breakdown", "restarts", "converged", "columns", "mm", "kk", "act")):
    """got: a dict of eigsh_ritz_ref / eigsh_ritz; want: ritz_py's or another of those.  Every array with =="""
    from krylov_numerics import same_bits
    for key in keys:
        if key in want:
            assert got[key] == want[key], (key, got[key], want[key])
    mm = want.get("mm")
    if mm is None or want.get("act") == 0:
        return
    for key in ("theta", "residuals"):
        assert same_bits(got[key][:mm], want[key][:mm]), key
    assert same_bits(np.asarray(got["Q"])[:mm, :want["kk"]], np.asarray(want["Q"])[:mm, :want["kk"]]), "Q"
    assert same_bits(np.asarray(got["T"])[:mm, :mm], np.asarray(want["T"])[:mm, :mm]), "T"
    assert same_bits(np.asarray(got["Y"])[:mm, :mm], np.asarray(want["Y"])[:mm, :mm]), "Y"


# ---------------------------------------------------------------------------------------------------------------------
# the method as a loop: thick-restart Lanczos with two Gram-Schmidt passes
# ---------------------------------------------------------------------------------------------------------------------
def lanczos_loop(matvec, dots, project, norm, divide, ritz, rotate, v0, n, k, ncv, keep, max_restarts):
    """The method of DESIGN.md 3.40 over abstract pieces, so that the device composition and the numpy loop are one text.
    V: a list-like of ncv + 1 vectors the pieces understand.  -> dict(status, restarts, matvecs, theta, residuals, V,
    columns, breakdown)."""
    T = np.zeros((ncv, ncv))
    out = dict(status=RUNNING, restarts=0, matvecs=0, theta=np.zeros(k), residuals=np.zeros(k), breakdown=None, columns=0, converged=0)
    nrm = norm(v0)
    if nrm == 0.0 or not math.isfinite(nrm):
        out.update(status=BREAKDOWN, breakdown="v0", V=None)
        return out
    V = [None] * (ncv + 1)
    V[0] = divide(v0, nrm)
    cols, beta, invariant = 0, nrm, False
    while True:
        while cols < ncv and not invariant:
            j = cols
            w = matvec(V[j])
            h = dots(V[:j + 1], w)
            w = project(V[:j + 1], h, w)
            c = dots(V[:j + 1], w)
            h = h + c
            w = project(V[:j + 1], c, w)
            beta = norm(w)
            T[:j + 1, j] = h
            T[j, :j + 1] = h
            out["matvecs"] += 1
            if not math.isfinite(beta):
                out.update(status=BREAKDOWN, breakdown="beta", V=V, columns=0)
                return out
            cols = j + 1
            if beta == 0.0:
                invariant = True
            else:
                V[j + 1] = divide(w, beta)
        mm = cols
        res = ritz(T[:mm, :mm], beta, out["restarts"], invariant)
        if res.get("act") == 0:                                             # a value of T is not finite
            out.update(status=res["status"], breakdown=res.get("breakdown"), V=V)
            return out
        kk = res["kk"]
        T[:, :] = 0.0
        T[np.arange(kk), np.arange(kk)] = res["theta"][:kk]
        if V[mm] is None:                                                   # an invariant subspace: the column is never read as data
            V[mm] = V[0]
        V = rotate(V, res["Q"], mm, kk)
        kt = min(k, mm)
        out["theta"][:kt], out["residuals"][:kt] = res["theta"][:kt], res["residuals"][:kt]
        out.update(status=res["status"], restarts=res["restarts"], breakdown=res["breakdown"], columns=mm, converged=res["converged"])
        if res["status"] != RUNNING:
            out["V"] = V
            return out
        cols = kk


def numpy_eigsh(A, k, ncv, which, v0, keep=None, rtol=1e-8, atol=0.0, max_restarts=300, ritz_ref=None):
    """The plain float64 numpy loop on a dense symmetric A.  ritz_ref None: numpy.linalg.eigh for T; else
    sblas_amd.eigsh_ritz_ref, the library's host Ritz step, with sblas_amd.eigsh_rotate_ref for the rotation."""
    n = A.shape[0]
    keep = default_keep(k, ncv) if keep is None else keep
    S = ritz_ref

    def project(V, h, w):
        for i in range(len(V)):
            w = w - h[i] * V[i]
        return w

    def ritz(T, beta, restarts, invariant):
        if S is not None:
            return S.eigsh_ritz_ref(T, beta, k, keep, which, rtol, atol, restarts, max_restarts, invariant)
        lapack = lambda t: np.linalg.eigh(t) + (0,)
        return ritz_py(T, beta, k, keep, which, rtol, atol, restarts, max_restarts, invariant, eig=lapack)

    def rotate(V, Q, mm, kk):
        block = np.stack(V[:mm + 1])
        new = S.eigsh_rotate_ref(block, Q) if S is not None else rotate_py(block, Q)
        return [new[i] for i in range(kk + 1)] + [None] * (len(V) - kk - 1)

    return lanczos_loop(lambda v: A @ v, lambda V, w: np.array([float(v @ w) for v in V]), project, lambda w: math.sqrt(float(w @ w)),
                        lambda w, b: w / b, ritz, rotate, np.asarray(v0, np.float64), n, k, ncv, keep, max_restarts)


def composed_eigsh(S, torch, dev, csr, k, ncv, which, v0=None, keep=None, rtol=1e-8, atol=0.0, max_restarts=300, planned=False, seed=0):
    """The whole method composed from the library's own pieces on the device: A v by SpmvPlan (planned) or the unplanned
    SpMV, the dots by gmres_dots, the two projections by gmres_project, |w| by krylov_dot and a Python square root, the
    division by torch (a rounded division per element, vector by vector), the Ritz step by the host reference and the rotation by keep calls
    of gmres_combine.  csr: (n, rowptr, colidx, val) as device tensors.  -> lanczos_loop's dict with V as a (k, n) array."""
    n, drp, dci, dval = csr
    keep = default_keep(k, ncv) if keep is None else keep
    plan = S.SpmvPlan(n, n, drp, dci) if planned else None
    if v0 is None:
        v0 = torch.from_numpy(S.cheby_start_ref(n, seed=seed)).to(dev)

    def matvec(v):
        q = torch.empty(n, dtype=torch.float64, device=dev)
        if plan is not None:
            plan.spmv(dval, v, 1.0, 0.0, q)
        else:
            S.spmv(n, n, drp, dci, dval, v, 1.0, 0.0, q)
        return q

    def divide(w, b):
        """a rounded division per element: by a vector, since torch turns a division by a host scalar into a product with
        its reciprocal"""
        return w / torch.full((n,), b, dtype=torch.float64, device=dev)

    def project(V, h, w):
        S.gmres_project(torch.stack(V), torch.from_numpy(np.ascontiguousarray(h)).to(dev), w)
        return w

    def rotate(V, Q, mm, kk):
        block = torch.stack(V[:mm])
        dQ = torch.from_numpy(np.ascontiguousarray(Q.T)).to(dev)
        new = [S.gmres_combine(block, dQ[i]) for i in range(kk)]
        return new + [V[mm]] + [None] * (len(V) - kk - 1)

    try:
        out = lanczos_loop(matvec, lambda V, w: S.gmres_dots(torch.stack(V), w).cpu().numpy(), project,
                           lambda w: math.sqrt(float(S.krylov_dot(w, w).cpu().numpy()[0])), divide,
                           lambda T, beta, restarts, inv: S.eigsh_ritz_ref(T, beta, k, keep, which, rtol, atol, restarts, max_restarts, inv),
                           rotate, v0, n, k, ncv, keep, max_restarts)
    finally:
        if plan is not None:
            plan.destroy()
    if out.get("V") is not None:
        out["V"] = torch.stack(out["V"][:min(k, max(out["columns"], 1))]).cpu().numpy()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the bounds of a finished solve (tests/test_eigsh_host.py states where they come from)
# ---------------------------------------------------------------------------------------------------------------------
def check_pairs(A, lam, which, theta, X, rtol, atol, factor=2.0):
    """theta: k values; X: (k, n) vectors.  |theta_i - lambda_i| <= |A x_i - theta_i x_i| + n eps |A|_F against the i-th
    extremal value, and |A x_i - theta_i x_i| <= factor max(rtol |theta_i|, atol) + n eps |A|_F.  -> the largest ratios
    (value error over its bound, residual over its bound)."""
    n = A.shape[0]
    slack = n * EPS * np.linalg.norm(A)
    want = wanted(lam, which, len(theta))
    worst = [0.0, 0.0]
    for i, th in enumerate(theta):
        res = np.linalg.norm(A @ X[i] - th * X[i])
        assert abs(np.linalg.norm(X[i]) - 1.0) <= 64 * n * EPS, ("norm", i)
        bound_v, bound_r = res + slack, factor * max(rtol * abs(th), atol) + slack
        assert abs(th - want[i]) <= bound_v, ("value", i, th, want[i], res)
        assert res <= bound_r, ("residual", i, res, bound_r)
        worst = [max(worst[0], abs(th - want[i]) / bound_v), max(worst[1], res / bound_r)]
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# the cases of the Ritz step that the host test and the GPU test share
# ---------------------------------------------------------------------------------------------------------------------
RITZ_SIZES = (1, 2, 3, 20, 63, 64)


def small_matrix(kind, mm, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        B = rng.standard_normal((mm, mm))
        return (B + B.T) / 2.0
    if kind == "diagonal":
        return np.diag(rng.standard_normal(mm))
    if kind == "identity":
        return np.eye(mm)
    if kind == "rank_one":
        u = rng.standard_normal(mm)
        return np.eye(mm) + np.outer(u, u)
    # what a restart produces: diag(theta) on the kept block, the arrow in row and column kept, a tridiagonal behind it
    kept = max(mm // 2, 1) if mm > 1 else 0
    T = np.zeros((mm, mm))
    T[np.arange(mm), np.arange(mm)] = np.sort(rng.uniform(0.0, 4.0, mm))[::-1]
    if kept < mm:
        T[:kept, kept] = T[kept, :kept] = 1e-3 * rng.standard_normal(kept)
    for j in range(kept, mm - 1):
        T[j, j + 1] = T[j + 1, j] = abs(rng.standard_normal())
    return T


def ritz_cases():
    """-> a list of (label, T, beta, k, keep, which, keywords) for eigsh_ritz_ref / eigsh_ritz / ritz_py"""
    cases = []
    for mm in RITZ_SIZES:
        k = 1 if mm < 4 else 4
        keeps = sorted({min(k, 63), max(min(mm - 1, 63), k)})
        for n_kind, kind in enumerate(("random", "diagonal", "identity", "rank_one", "arrow")):
            T = small_matrix(kind, mm, 100 * mm + n_kind)
            for which in ("LA", "SA", "LM"):
                for keep in keeps:
                    cases.append(("%s-%d-%s-%d" % (kind, mm, which, keep), T, 0.37, k, keep, which, {}))
        T = small_matrix("arrow", mm, 7 + mm)
        R = small_matrix("random", mm, 9 + mm)
        keep = keeps[-1]
        cases.append(("big-%d" % mm, R * 1e150, 1e150, k, keep, "LM", {}))
        cases.append(("tiny-%d" % mm, R * 1e-150, 1e-150, k, keep, "SA", {}))
        cases.append(("mixed-%d" % mm, R * np.outer(10.0 ** np.linspace(-8, 8, mm), 10.0 ** np.linspace(-8, 8, mm)), 1.0, k, keep, "LA", {}))
        nan = T.copy()
        nan[mm - 1, 0] = nan[0, mm - 1] = np.nan
        cases.append(("nan-%d" % mm, nan, 1.0, k, keep, "LA", {}))
        inf = T.copy()
        inf[0, 0] = np.inf
        cases.append(("inf-%d" % mm, inf, 1.0, k, keep, "LA", {}))
        cases.append(("beta0-%d" % mm, T, 0.0, k, keep, "LA", dict(invariant=True)))
        cases.append(("beta0-short-%d" % mm, T, 0.0, mm + 1 if mm < 63 else k, max(keep, mm + 1 if mm < 63 else k), "SA", dict(invariant=True)))
        cases.append(("betanan-%d" % mm, T, np.nan, k, keep, "LA", {}))
        cases.append(("limit-%d" % mm, T, 5.0, k, keep, "LA", dict(restarts=2, max_restarts=3)))
        cases.append(("met-%d" % mm, T, 1e-30, k, keep, "SA", dict(rtol=1e-8)))
        cases.append(("atol-%d" % mm, T, 1e-3, k, keep, "LM", dict(rtol=0.0, atol=1.0)))
        cases.append(("frozen-%d" % mm, T, 1.0, k, keep, "LA", dict(status=1)))
    return cases
