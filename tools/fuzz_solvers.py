"""Randomised differential test of the solvers (KrylovPlan, GmresPlan, pcg, bicgstab, gmres), one GPU.

  python tools/fuzz_solvers.py [--op pcg|bicgstab|gmres|all] [--cases N] [--seed S] [--only K] [--max-rows R]

It follows tools/fuzz_plans.py, whose generator structure(), families, damage kinds and degenerate shapes it imports.
Case k of operation op draws from case_rng(seed, op, k); its parameters are printed when it fails (and with --only), so
`--op X --seed S --only K` replays it.  Exit status 1 on the first mismatch; nothing retries a failing case.

Every output of a solve is judged on its bits against the same solver composed from its parts on the device
(tests/solver_compose.py: SpmvPlan or the unplanned SpMV, Ilu0Plan.apply / AmgPlan.apply / dinv, the pinned dot, the
scalar steps in Python floats), integers and strings on ==.  No tolerance is defined here but one: a converged solve
without a preconditioner or with Jacobi is also held to a plain float64 host loop, at the bar of
tests/test_gpu_krylov.py (true residual <= 2 max(the host loop's, tol)).  The one-shot wrappers are called wherever their
arguments can express the case and must return the plan's bits; a second solve on the same plan with new values on the
same structure (the factor and the AMG set up again) must equal its composition too.

Each operation has draw_<op>() (host only), judge_<op>() (host only, raises AssertionError) and case_<op>(), which draws,
solves on the device, composes, judges and returns what the case exercised.  tests/test_fuzz_solvers_host.py runs the
host-only pieces without a GPU, with the loops composed from host parts; tests/test_gpu_fuzz_solvers.py runs case_<op>
and asserts a census of the returned dicts.

What rotates with the case number (turn()), each at a period that has no factor in common with another's, all below RUN:
the preconditioner, spmv_plan given or not, n planted at the cell's edges or drawn, GMRES's restart, the stopping regime,
check_every, the guess and the right-hand side.  Family, degenerate shape and the planted row against SPMV_SPLIT_MIN
rotate as structure() and drawn_plant() have them.  PLANTS is the fixed list of tiny exact systems that reach the
breakdowns, outside the rotation."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "s-blas_amd", "python"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import sblas_amd as S
import fuzz_plans as FP
from fuzz_plans import FAMILIES, DAMAGE, DEGENERATE, RELATIONS, RUN, MIN_ROWS, structure, need   # imported, not copied: the census reads them here
import numerics as NM
import krylov_numerics as KN
import gmres_numerics as GN
import amg_numerics as AN
import solver_compose as SC

OPS = ["pcg", "bicgstab", "gmres"]
CELL = S.krylov_limits()["cell"]
# the turns: a value of each list by case % len(list); the lengths are pairwise coprime and below RUN
PRECOND_TURN = [None, "jacobi", "ilu0", "amg", "jacobi", None, "amg_smoothed", "jacobi", "ilu0", "jacobi", "amg_device", None, "jacobi"]
PLANNED_TURN = [True, False]
SIZES = [CELL - 1, CELL, CELL + 1, 2 * CELL + 5]                          # n against the cell of the partial sums
SIZE_TURN = [SIZES[(r // 2) % 4] if r % 2 else None for r in range(29)]   # None: a drawn size
RESTARTS = [1, 2, 3, 4, 5, 8, 30, 63, 64]                                  # both sides of GMRES_DOT_GROUP, the ends of [1, GMRES_MAX_RESTART]
RESTART_TURN = [RESTARTS[r % 9] for r in range(23)]
REGIMES = ["a", "b", "c", "d", "e", "f"]
REGIME_TURN = [REGIMES[r % 6] for r in range(11)]
CHECK_EVERY = [1, 3, 8, 50]
CHECK_TURN = [CHECK_EVERY[r % 4] for r in range(17)]
X0_KINDS = ["none", "random", "exact"]
X0_TURN = ["exact" if r in (5, 17, 28) else "none" if r % 2 == 0 else "random" for r in range(31)]
B_KINDS = ["random", "zero", "mixed"]
B_TURN = ["zero" if r in (7, 15) else "mixed" if r % 3 == 1 else "random" for r in range(19)]
TURNS = dict(precond=PRECOND_TURN, planned=PLANNED_TURN, size=SIZE_TURN, restart=RESTART_TURN, regime=REGIME_TURN,
             check_every=CHECK_TURN, x0=X0_TURN, b=B_TURN)
PRECONDS = [None, "jacobi", "ilu0", "amg", "amg_smoothed", "amg_device"]
WRAPPER_PRECOND = {None: None, "jacobi": "jacobi", "ilu0": "ilu0", "amg": "amg", "amg_smoothed": "amg_smoothed"}
# Measured on the host over the committed seed's draws: with Jacobi a float64 loop meets 1e-10 on every drawn matrix in at
# most 33 iterations (GMRES(1) apart, which stalls on an arrow); without a preconditioner the same matrices take 60 to
# over 200, because their diagonals spread with the row lengths.  So regimes (a) to (c) allow MAX_ITER iterations, nearly
# twice the Jacobi count: a solve that needs more ends in "limit" there, in the composition and on the device alike, and
# convergence is expected (expects_convergence()) only where the host loop shows it.
RTOL, MAX_ITER = 1e-10, 60
HOST_LIMIT = 200                                          # the host test's bound on a host loop that is expected to converge
I32, F64 = np.int32, np.float64
FLOATS = dict(pcg=["x", "rnorm", "bnorm", "alpha", "beta", "omega"], bicgstab=["x", "rnorm", "bnorm", "alpha", "beta", "omega"],
              gmres=["x", "rnorm", "bnorm"])
EXACT = dict(pcg=["status", "iterations", "breakdown"], bicgstab=["status", "iterations", "breakdown"],
             gmres=["status", "iterations", "breakdown", "restarts", "columns"])


def turn(case):
    return {name: values[case % len(values)] for name, values in TURNS.items()}


# ---------------------------------------------------------------------------------------------------------------------
# the problem (host only)
# ---------------------------------------------------------------------------------------------------------------------
def _csr_of_pairs(n, row, col):
    """the pairs sorted by (row, col), nothing doubled"""
    key = np.unique(np.asarray(row, np.int64) * n + np.asarray(col, np.int64))
    return np.concatenate([[0], np.cumsum(np.bincount(key // n, minlength=n))]).astype(np.int64), key % n


def _resize(n, rp, ci, size):
    """the pattern cut or padded (with empty rows) to `size` rows and columns"""
    if n > size:
        row = NM.row_of_entries(rp)
        keep = (row < size) & (ci < size)
        rp = np.concatenate([[0], np.cumsum(np.bincount(row[keep], minlength=size))]).astype(np.int64)
        return rp, ci[keep]
    return np.concatenate([rp, np.full(size - n, rp[-1])]), ci


def conform(op, rng, st, precond, size):
    """-> (n, rp, ci, planted row or None): the drawn structure conformed to the solve.  pcg: the pattern made symmetric;
    with a preconditioner: rows sorted, nothing doubled; always one stored diagonal a row.  Without a preconditioner
    bicgstab and gmres keep the pattern as drawn (unsorted rows, doubled columns); pcg gets its damage back in
    damaged_again()."""
    n, rp, ci, plant = st["rows"], st["rp"], st["ci"], st["plant"]
    if size is not None:
        rp, ci = _resize(n, rp, ci, size)
        n = size
    pr = int(rng.integers(n)) if plant else None
    if op == "pcg" or precond is not None:
        row = NM.row_of_entries(rp)
        off = ci != row
        r, c = row[off], ci[off]
        if op == "pcg":
            r, c = np.concatenate([r, c]), np.concatenate([c, r])
        if plant:                                         # the row of exactly L stored entries; for pcg the column too: an arrow
            cols = FP.distinct(rng, 0, n, plant["L"] - 1, without=pr)
            keep = (r != pr) & (c != pr) if op == "pcg" else r != pr
            r, c = np.concatenate([r[keep], np.full(len(cols), pr)]), np.concatenate([c[keep], cols])
            if op == "pcg":
                r, c = np.concatenate([r, cols]), np.concatenate([c, np.full(len(cols), pr)])
        rp, ci = _csr_of_pairs(n, np.concatenate([r, np.arange(n)]), np.concatenate([c, np.arange(n)]))
    else:
        rp, ci = FP._one_diagonal(rng, n, rp, ci)
        if plant:
            new = np.concatenate([FP.distinct(rng, 0, n, plant["L"] - 1, without=pr), [pr]])
            rp, ci = FP.replace_row(rp, ci, pr, rng.permutation(new))
    return n, rp, ci, pr


def values(rng, n, rp, ci, symmetric, integer):
    """off-diagonals in [-1, -0.25] u [0.25, 1] (integer: +-1 .. +-4), symmetric for pcg; the diagonal (1 + delta) * the
    row's absolute off-diagonal sum + 0.1 with delta in [0.25, 1] (integer: twice the sum + 1): SPD when symmetric,
    strictly dominant otherwise"""
    row = NM.row_of_entries(rp)
    nnz = len(ci)
    mag = rng.integers(1, 5, nnz).astype(F64) if integer else rng.uniform(0.25, 1.0, nnz)
    val = mag * rng.choice([-1.0, 1.0], nnz)
    if symmetric:                                         # the pattern is sorted and symmetric: the keys ascend
        mirror = np.searchsorted(row * n + ci, ci * n + row)
        lower = row > ci
        val[lower] = val[mirror[lower]]
    dg = ci == row
    s = np.bincount(row, np.where(dg, 0.0, np.abs(val)), minlength=n)
    delta = rng.uniform(0.25, 1.0, n)
    val[dg] = 2.0 * s + 1.0 if integer else (1.0 + delta) * s + 0.1
    return val


def damaged_again(rng, kind, n, rp, ci, val, planted_row=None):
    """pcg without a preconditioner: the damage the symmetric pattern lost, put back with the values -- some rows
    shuffled, and under "dups" some off-diagonal entries stored as two halves (v / 2 twice: their sum is v exactly); the planted row keeps
    its length"""
    if kind not in ("shuffle", "dups") or len(ci) == 0:
        return rp, ci, val
    row = NM.row_of_entries(rp)
    if kind == "dups":
        offd = np.flatnonzero((ci != row) & (row != (-1 if planted_row is None else planted_row)))
        if len(offd):
            twice = np.unique(rng.choice(offd, max(1, len(offd) // 30)))
            val = val.copy()
            val[twice] = val[twice] / 2.0
            ci, val, row = np.insert(ci, twice, ci[twice]), np.insert(val, twice, val[twice]), np.insert(row, twice, row[twice])
            rp = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n))]).astype(np.int64)
    ci, val = ci.copy(), val.copy()
    for r in rng.integers(0, n, size=max(1, n // 5)):
        a, b = rp[r], rp[r + 1]
        order = rng.permutation(b - a)
        ci[a:b], val[a:b] = ci[a:b][order], val[a:b][order]
    return rp, ci, val


def congruent(rng, n, rp, ci, val):
    """D A D with a positive diagonal D in [0.9, 1.1]: symmetric stays symmetric (d_i d_j is formed first), dominant stays
    dominant (1.25 * 0.9 / 1.1 > 1), and every value changes"""
    d = rng.uniform(0.9, 1.1, n)
    row = NM.row_of_entries(rp)
    return (d[row] * d[ci]) * val


def draw(op, case, rng, max_rows):
    t = turn(case)
    size = t["size"]
    st = structure(rng, max_rows, True, None if size is not None else dict(spmv_split=S.SPMV_SPLIT_MIN), case, grow=1)
    degenerate = st["degenerate"]
    if degenerate:                                        # no preconditioner, the shape and the values as drawn
        t["precond"], size = None, None
        n, rp, ci, pr = st["rows"], st["rp"], st["ci"], None
    else:
        n, rp, ci, pr = conform(op, rng, st, t["precond"], size)
    exact = t["x0"] == "exact"
    if degenerate:
        val = [rng.integers(-4, 5, len(ci)).astype(F64) if exact else rng.standard_normal(len(ci)), rng.standard_normal(len(ci))]
    else:
        first = values(rng, n, rp, ci, op == "pcg", exact)
        if op == "pcg" and t["precond"] is None:
            rp, ci, first = damaged_again(rng, st["damage"], n, rp, ci, first, pr)
        val = [first, congruent(rng, n, rp, ci, first)]
    if exact:                                             # small integers on integer values: b = A x is exact, r0 = 0
        x0 = rng.integers(-8, 9, n).astype(F64)
        b, t["b"] = np.asarray(KN.matvec(n, rp, ci, val[0], x0), F64), "exact"    # (no entries: bincount counts)
    else:
        x0 = None if t["x0"] == "none" else 0.1 * rng.standard_normal(n)
        b = np.zeros(n) if t["b"] == "zero" else rng.standard_normal(n)
        if t["b"] == "mixed":
            b = b * 10.0 ** rng.integers(-6, 7, n)
    bnorm = float(np.linalg.norm(b))
    regime = t["regime"]
    stop = dict(a=(RTOL, 0.0), b=(RTOL, 1e-6 * bnorm), c=(0.0, 1e-8 * bnorm), d=(RTOL, 0.0), e=(RTOL, 0.0), f=(0.0, 0.0))[regime]
    P = dict(op=op, st=st, n=n, rp=rp.astype(I32), ci=ci.astype(I32), val=val, b=b, x0=x0, planted_row=pr, size=size,
             precond=t["precond"], planned=t["planned"], restart=t["restart"] if op == "gmres" else None, regime=regime,
             rtol=stop[0], atol=stop[1], max_iter=int(rng.integers(1, 13)) if regime == "f" else MAX_ITER,
             check_every=t["check_every"], x0_kind=t["x0"], b_kind=t["b"])
    P["params"] = FP.params_of(op, case, st, n=n, nnz=len(ci), size=size, precond=P["precond"], planned=P["planned"], restart=P["restart"],
                               regime=regime, rtol=P["rtol"], atol=P["atol"], max_iter=P["max_iter"], check_every=P["check_every"],
                               x0=P["x0_kind"], b=P["b_kind"], planted_row=pr)
    return P


def draw_pcg(case, rng, max_rows):
    return draw("pcg", case, rng, max_rows)


def draw_bicgstab(case, rng, max_rows):
    return draw("bicgstab", case, rng, max_rows)


def draw_gmres(case, rng, max_rows):
    return draw("gmres", case, rng, max_rows)


def expects_convergence(P):
    """regimes (a) to (c) on a drawn (SPD or dominant) matrix with Jacobi, where D^-1 A has a unit diagonal and
    off-diagonal row sums of at most 0.8 (GMRES(1), a one-dimensional minimisation, apart): a float64 host loop
    converges within a few dozen iterations (the host test asserts it), so the composition and the solver must.  Without
    a preconditioner the count depends on the spread of the diagonal, and with ILU(0) or AMG no cheap host loop shows
    it: there the solver must end in whatever the composition ends in."""
    return P["st"]["degenerate"] is None and P["regime"] in "abc" and P["precond"] == "jacobi" and P["restart"] != 1


# ---------------------------------------------------------------------------------------------------------------------
# the composition, the stopping regime and the judges (host only: the parts are callables)
# ---------------------------------------------------------------------------------------------------------------------
def compose(op, parts, b, x0, restart, rtol, atol, max_iter):
    """the composed loop of `op` on parts (matvec, apply, dot, dots) -> the answer as a dict"""
    matvec, apply, dot, dots = parts
    x0 = np.zeros(len(b)) if x0 is None else x0
    if op == "gmres":
        return SC.composed_gmres(matvec, apply, dot, dots, b, x0, restart, rtol, max_iter, atol=atol)
    loop = SC.composed_pcg if op == "pcg" else SC.composed_bicgstab
    return loop(matvec, apply, dot, b, x0, rtol, max_iter, atol=atol).asdict()


def host_parts(n, rp, ci, val, dinv=None):
    """the parts on the host: the matrix product by rows in numpy, the pinned dot's host restatement, dinv or nothing"""
    dot = lambda a, b: float(S.krylov_dot_ref(a, b))
    apply = (lambda v: v) if dinv is None else (lambda v: dinv * v)
    return (lambda v: np.asarray(KN.matvec(n, rp, ci, val, v), F64)), apply, dot, (lambda V, w: [dot(v, w) for v in V])


def stopping(P, loop):
    """(rtol, atol, max_iter, what the regime expects of the composition or None).  loop(rtol, atol, max_iter) is the
    composition; regimes (d) and (e) run it once at regime (a) to learn its count."""
    rtol, atol, max_iter = P["rtol"], P["atol"], P["max_iter"]
    if P["regime"] in "de":
        learnt = loop(RTOL, 0.0, MAX_ITER)
        if learnt["status"] == "converged" and learnt["iterations"] >= 1:
            if P["regime"] == "d":
                return rtol, atol, learnt["iterations"] - 1, ("limit", learnt["iterations"] - 1)
            return rtol, atol, learnt["iterations"], ("converged", learnt["iterations"])
        return rtol, atol, learnt["iterations"], None    # nothing to cut short: whatever the composition ends in
    if expects_convergence(P):
        return rtol, atol, max_iter, ("converged", None)
    return rtol, atol, max_iter, None


def judge_expectation(P, want, expected, first=True):
    """what the regime says about the composition itself (first: the drawn values, to which an exact guess belongs)"""
    if expected is not None:
        need(want["status"] == expected[0], P, "the composition", "ends in", want["status"], "where the regime expects", expected[0])
        need(expected[1] is None or want["iterations"] == expected[1], P, "the composition", "stops at", want["iterations"], "for", expected[1])
    if (first and P["x0_kind"] == "exact") or P["b_kind"] == "zero":
        need((want["status"], want["iterations"], want["rnorm"]) == ("converged", 0, 0.0), P, "an exact guess or b = 0", "does not end at iteration 0")


def judge(op, P, got, want, what="solve"):
    """integers and strings on ==, floats on their bits (NaN as NaN)"""
    for key in EXACT[op]:
        need(got[key] == want[key], P, what, key, "is", got[key], "for", want[key])
    for key in FLOATS[op]:
        if key == "x":
            need(np.shape(got[key]) == np.shape(want[key]), P, what, "x has shape", np.shape(got[key]))
            need(KN.same_bits(got[key], want[key]), P, what, "x differs on the bits in",
                 int((KN.bits(got[key]) != KN.bits(want[key])).sum()), "of", len(want[key]), "entries")
        else:
            need(KN.same_bits(got[key], want[key]), P, what, key, "is %r for %r" % (got[key], want[key]))


def judge_pcg(P, got, want, what="solve"):
    judge("pcg", P, got, want, what)


def judge_bicgstab(P, got, want, what="solve"):
    judge("bicgstab", P, got, want, what)


def judge_gmres(P, got, want, what="solve"):
    judge("gmres", P, got, want, what)


def true_residual(P, val, x):
    return float(np.linalg.norm(P["b"] - KN.matvec(P["n"], P["rp"], P["ci"], val, np.asarray(x, F64))))


def carries_the_bar(P, want):
    """the independent half applies to a converged solve of a drawn matrix without a preconditioner or with Jacobi"""
    return P["st"]["degenerate"] is None and P["precond"] in (None, "jacobi") and want["status"] == "converged"


def host_solution(P, val, rtol, atol):
    """x of a plain float64 host loop of the same method at the same stopping test (tests/amg_numerics.py,
    tests/gmres_numerics.py) -> (iterations, x)"""
    n, rp, ci, b, x0 = P["n"], P["rp"], P["ci"], P["b"], P["x0"]
    bnorm = float(np.linalg.norm(b))
    if bnorm == 0.0:
        return 0, np.zeros(n)
    rel = max(rtol * bnorm, atol) / bnorm
    dinv = 1.0 / val[ci == NM.row_of_entries(rp)] if P["precond"] == "jacobi" else None
    apply = (lambda v: v.copy()) if dinv is None else (lambda v: dinv * v)
    guess = np.zeros(n) if x0 is None else x0
    if P["op"] == "pcg":
        return AN.host_pcg(n, rp, ci, val, b, apply, rel, limit=HOST_LIMIT, x0=guess)
    if P["op"] == "bicgstab":
        return AN.host_bicgstab(n, rp, ci, val, b, apply, rel, limit=HOST_LIMIT, x0=guess)
    steps, _, x = GN.host_gmres(n, rp, ci, val, b, guess, P["restart"], rel, limit=HOST_LIMIT, precond=apply if dinv is not None else None)
    return steps, x


def residual_bound(P, val, host_x, rtol, atol):
    """the bar of tests/test_gpu_krylov.py: 2 max(the host loop's true residual, tol), tol = max(rtol |b|, atol)"""
    return 2.0 * max(true_residual(P, val, host_x), max(rtol * float(np.linalg.norm(P["b"])), atol))


def judge_residual(P, val, x, host_x, rtol, atol):
    got, bound = true_residual(P, val, x), residual_bound(P, val, host_x, rtol, atol)
    need(got <= bound, P, "the true residual", "%.6e" % got, "is above the bound", "%.6e" % bound)


# ---------------------------------------------------------------------------------------------------------------------
# a case on the device
# ---------------------------------------------------------------------------------------------------------------------
def answer(op, x, st):
    out = {k: st[k] for k in EXACT[op] + FLOATS[op] if k != "x"}
    out["x"] = x.cpu().numpy().copy()
    return out


def wrapper_serves(P):
    """the one-shot wrappers make their own plans: no SpmvPlan, the preconditioners they name with their defaults"""
    return not P["planned"] and P["precond"] in WRAPPER_PRECOND


def case_any(op, case, rng, dev, max_rows):
    import torch
    P = draw(op, case, rng, max_rows)
    n, b, x0 = P["n"], P["b"], P["x0"]
    env = (S, torch, dev)
    parts = SC.Parts(env, n, P["rp"], P["ci"], P["val"][0], P["precond"], planned=P["planned"])
    plan = None
    seen = dict(split_rows=None, wide=None, chain=None, levels=None)
    try:
        plan = parts.plan(op if op != "gmres" else P["restart"])
        if parts.spmv is not None:
            seen["split_rows"] = parts.spmv.info()["split_rows"]
        if parts.ilu is not None:
            info = parts.ilu.info()
            seen["wide"], seen["chain"] = info["wide_launches"], info["chain_launches"]
        if parts.amg is not None:
            seen["levels"] = parts.amg.info()["levels"]
        db = FP.up(dev, b)
        solves = []
        for which, val in enumerate(P["val"]):
            if which:
                parts.revalue(val)                        # the factor and the AMG are set up again, on the same plans
            loop = lambda rtol, atol, max_iter: compose(op, (parts.matvec, parts.apply, parts.dot, parts.dots), b, x0, P["restart"],
                                                        rtol, atol, max_iter)
            rtol, atol, max_iter, expected = stopping(P, loop)
            want = loop(rtol, atol, max_iter)
            what = "the second solve" if which else "solve"
            judge_expectation(P, want, expected, first=not which)
            kw = dict(rtol=rtol, atol=atol, max_iter=max_iter, check_every=P["check_every"])
            x, st = plan.solve(parts.dval, db, x=None if x0 is None else FP.up(dev, x0), **kw, **parts.kw())
            got = answer(op, x, st)
            judge(op, P, got, want, what)
            if which == 0 and wrapper_serves(P):
                call = dict(pcg=S.pcg, bicgstab=S.bicgstab, gmres=S.gmres)[op]
                more = dict(restart=P["restart"]) if op == "gmres" else {}
                wx, wst = call((n, parts.drp, parts.dci, parts.dval), db, precond=WRAPPER_PRECOND[P["precond"]],
                               x=None if x0 is None else FP.up(dev, x0), **more, **kw)
                judge(op, P, answer(op, wx, wst), got, "the one-shot wrapper against the plan")
            bar = carries_the_bar(P, want)
            if bar:
                judge_residual(P, val, got["x"], host_solution(P, val, rtol, atol)[1], rtol, atol)
            solves.append(dict(status=st["status"], iterations=st["iterations"], max_iter=max_iter, bar=bar,
                               atol_governed=bool(st["status"] == "converged" and st["iterations"] > 0 and st["rnorm"] > rtol * st["bnorm"]),
                               restarts=st.get("restarts"), columns=st.get("columns")))
    finally:
        if plan is not None:
            plan.destroy()
        parts.destroy()
    torch.cuda.synchronize()
    return census_of(P, solves=solves, wrapper=wrapper_serves(P), **seen)


def census_of(P, **more):
    out = FP.census_of(P["st"], n=P["n"], size=P["size"], precond=P["precond"], planned=P["planned"], restart=P["restart"], regime=P["regime"],
                       check_every=P["check_every"], x0=P["x0_kind"], b=P["b_kind"])
    out.update(more)
    return out


def case_pcg(case, rng, dev, max_rows):
    return case_any("pcg", case, rng, dev, max_rows)


def case_bicgstab(case, rng, dev, max_rows):
    return case_any("bicgstab", case, rng, dev, max_rows)


def case_gmres(case, rng, dev, max_rows):
    return case_any("gmres", case, rng, dev, max_rows)


# ---------------------------------------------------------------------------------------------------------------------
# the planted breakdowns: tiny exact systems (small integers, so every sum is exact and the host composition and the
# device's agree on the bits), every entry stored, dinv the caller's.  expect: (status, breakdown, iterations).
# ---------------------------------------------------------------------------------------------------------------------
INF = float("inf")
PLANTS = [
    dict(name="pcg (p, q)", op="pcg", A=[[-2, -1], [-1, 0]], dinv=[-1, -1], b=[0, 1], expect=("breakdown", "(p, q)", 0)),
    dict(name="pcg rho", op="pcg", A=[[-2, -1], [-1, -2]], dinv=[-1, 1], b=[1, 1], expect=("breakdown", "rho", 1)),
    dict(name="bicgstab (r^, v)", op="bicgstab", A=[[-2, -1], [-1, -2]], dinv=[-1, 1], b=[1, 1], expect=("breakdown", "(r^, v)", 0)),
    dict(name="bicgstab (t, t)", op="bicgstab", A=[[-2, -1], [0, 0]], dinv=[-1, -1], b=[2, 1], expect=("breakdown", "(t, t)", 0)),
    dict(name="bicgstab omega", op="bicgstab", A=[[-2, -1], [0, -1]], dinv=[-1, 1], b=[2, 1], expect=("breakdown", "omega", 1)),
    # not reachable with 2 x 2 integers; a search of 3 x 3 ones with entries in [-2, 2] finds it: (r^, r) = 0 after the first
    # iteration, so beta = 0 and alpha = 0 in the second, whose residual test is followed by the test of the old rho
    dict(name="bicgstab rho", op="bicgstab", A=[[2, 0, 2], [1, 1, -1], [0, 1, 1]], dinv=[1, -1, -1], b=[1, 0, 0], expect=("breakdown", "rho", 2)),
    # both at once: the old rho is 0 and the second iteration's omega is 0 as well; rho is tested first and is the one named
    dict(name="bicgstab rho before omega", op="bicgstab", A=[[-2, 0, -2], [0, 0, -2], [-2, -2, 2]], dinv=[-1, 1, -1], b=[0, 0, 2],
         expect=("breakdown", "rho", 2)),
    # s = r - alpha v vanishes, so t = A s^ = 0 with |s| = 0 <= tol: omega = 0 takes the half step, and that converges
    dict(name="bicgstab omega = 0", op="bicgstab", A=[[1, 0], [0, 1]], dinv=[1, 1], b=[1, 1], expect=("converged", None, 1)),
    # diag(1, 0, 1, 0) x = 1: the second column finds w = 0 and rotates h = (1/2, 1/2) to d = 0; the first column stays
    dict(name="gmres givens", op="gmres", A=[[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]], dinv=None, b=[1, 1, 1, 1], restart=30,
         expect=("breakdown", "givens", 1)),
    # a non-finite value: 0 * inf = NaN in A x0, so the first residual's norm is not finite
    dict(name="gmres beta", op="gmres", A=[[INF, 0], [0, 1]], dinv=None, b=[1, 1], restart=30, expect=("breakdown", "beta", 0)),
]
PLANT_KW = dict(rtol=RTOL, atol=0.0, max_iter=50)


def plant_system(plant):
    """-> (n, rowptr, colidx, val, dinv, b): every entry stored, zeros too"""
    A = np.asarray(plant["A"], F64)
    n = len(A)
    rp = (np.arange(n + 1) * n).astype(I32)
    ci = np.tile(np.arange(n), n).astype(I32)
    return n, rp, ci, A.reshape(-1).copy(), None if plant["dinv"] is None else np.asarray(plant["dinv"], F64), np.asarray(plant["b"], F64)


def plant_params(plant):
    return dict(params=dict(plant=plant["name"], A=plant["A"], dinv=plant["dinv"], b=plant["b"], restart=plant.get("restart")))


def judge_plant(plant, want):
    """the literal (status, breakdown, iterations) against a composition (the host's, or the device's)"""
    need((want["status"], want["breakdown"], want["iterations"]) == plant["expect"], plant_params(plant), "the planted system",
         "ends in", (want["status"], want["breakdown"], want["iterations"]), "for", plant["expect"])


def host_plant(plant):
    """the plant under the host composition -> the answer"""
    n, rp, ci, val, dinv, b = plant_system(plant)
    return compose(plant["op"], host_parts(n, rp, ci, val, dinv), b, None, plant.get("restart"), **PLANT_KW)


def case_plant(plant, dev):
    """the plant on the device: the literal, and the bits of the device's composition and of the host's"""
    import torch
    n, rp, ci, val, dinv, b = plant_system(plant)
    op, P = plant["op"], plant_params(plant)
    parts = SC.Parts((S, torch, dev), n, rp, ci, val, None if dinv is None else "jacobi", planned=False, dinv=dinv)
    plan = None
    try:
        plan = parts.plan(op if op != "gmres" else plant["restart"])
        want = compose(op, (parts.matvec, parts.apply, parts.dot, parts.dots), b, None, plant.get("restart"), **PLANT_KW)
        x, st = plan.solve(parts.dval, FP.up(dev, b), check_every=3, **PLANT_KW, **parts.kw())
        got = answer(op, x, st)
    finally:
        if plan is not None:
            plan.destroy()
        parts.destroy()
    torch.cuda.synchronize()
    judge_plant(plant, got)
    judge(op, P, got, want, "the planted system against the device's composition")
    judge(op, P, got, host_plant(plant), "the planted system against the host's composition")
    return dict(name=plant["name"], status=got["status"], breakdown=got["breakdown"])


DRAW = dict(pcg=draw_pcg, bicgstab=draw_bicgstab, gmres=draw_gmres)
JUDGE = dict(pcg=judge_pcg, bicgstab=judge_bicgstab, gmres=judge_gmres)
CASE = dict(pcg=case_pcg, bicgstab=case_bicgstab, gmres=case_gmres)


def case_rng(seed, op, case):
    return np.random.default_rng([seed, len(FP.OPS) + OPS.index(op), case])


def run_case(op, case, seed, dev, max_rows):
    """case `case` of `op` on the device -> what it exercised; AssertionError (with the parameters) on a mismatch, and
    also when the library refuses a call of a generated case: every generated case is within the contracts"""
    try:
        return CASE[op](case, case_rng(seed, op, case), dev, max_rows)
    except S.SblasError as e:
        params = DRAW[op](case, case_rng(seed, op, case), max_rows)["params"]
        raise AssertionError("the library refused a call: %s %s" % (e, params)) from e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", default="all", choices=OPS + ["all"])
    ap.add_argument("--cases", type=int, default=RUN)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-rows", type=int, default=1500)
    ap.add_argument("--only", type=int, default=-1)
    args = ap.parse_args()
    if args.max_rows < MIN_ROWS:
        ap.error("--max-rows must be at least %d" % MIN_ROWS)
    import torch
    dev = torch.device("cuda:0")
    for op in (OPS if args.op == "all" else [args.op]):
        for case in ([args.only] if args.only >= 0 else range(args.cases)):
            try:
                seen = run_case(op, case, args.seed, dev, args.max_rows)
            except AssertionError as e:
                print("MISMATCH %s case %d: %s" % (op, case, e), flush=True)
                print("fuzz: FAILED (replay: --op %s --seed %d --max-rows %d --only %d)" % (op, args.seed, args.max_rows, case))
                return 1
            if args.only >= 0:
                print(DRAW[op](case, case_rng(args.seed, op, case), args.max_rows)["params"])
                print("exercised:", seen)
        print("%s: all cases match their compositions" % op, flush=True)
    if args.only < 0:
        for plant in PLANTS:
            try:
                case_plant(plant, dev)
            except AssertionError as e:
                print("MISMATCH planted %s: %s" % (plant["name"], e), flush=True)
                return 1
        print("planted breakdowns: all reach their literals and match their compositions", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
