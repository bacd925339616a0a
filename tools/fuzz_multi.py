"""Randomised differential test of the multi-right-hand-side family (KrylovMultiPlan, GmresMultiPlan, pcg_multi,
bicgstab_multi, gmres_multi, SptrsvPlan.solve_multi, Ilu0Plan.apply_multi, AmgPlan.apply_multi), one GPU.

  python tools/fuzz_multi.py [--op pcg_multi|bicgstab_multi|gmres_multi|sptrsm_tiled|amg_multi|all] [--cases N] [--seed S]
                             [--only K] [--max-rows R]

It follows tools/fuzz_solvers.py in every convention and imports that file's problem (structure(), conform(), values(),
damaged_again(), congruent(), the judges, the residual bar and PLANTS); nothing of it is copied.  Case k of operation op
draws from case_rng(seed, op, k); its parameters are printed when it fails (and with --only), so `--op X --seed S --only K`
replays it.  Exit status 1 on the first mismatch; nothing retries a failing case.

The three solver operations solve an (n, s) block and judge every column's every output on its bits (floats) and on ==
(integers, strings) against the lockstep loop of tests/multi_compose.py / tests/gmres_multi_compose.py run on the device's
parts (tests/multi_parts.py: an SpmmPlan of width s called row-major, krylov_dot per column, M^-1 on one column by dinv,
AmgPlan.apply or Ilu0Plan.apply).  A second solve on the same plan with D A D values (the factor and the AMG set up again)
must equal its own composition; the one-shot wrappers, where their arguments can express the case, must return the
plan's bits; the canaries round B and X must be intact and B unchanged.  No tolerance is defined here: a converged column
without a preconditioner or with Jacobi is also held to fuzz_solvers.judge_residual, the bar of tests/test_gpu_krylov.py,
and sptrsm_tiled holds one column to sptrsv_numerics.check_residual.  sptrsm_tiled and amg_multi compare a block apply
with the single-column entry column by column, on the bits.

The work of a case is bounded: the composition calls the device once per dot per column, so a case costs about
s * iterations * dots per iteration (PCG 3, BiCGStab 6, GMRES restart + 2, a cycle's mean of the 2 (j + 1) + 1 of step j).
bounded() lowers GMRES's restart until one iteration fits and then max_iter until that product is at most DOT_BUDGET; a
bounded solve ends in "limit" in the composition and on the device alike.  Regimes (d) and (e) -- one short of and equal
to the composition's count -- refer to the bounded count of the column that converges last.  Regime (b) comes twice in a
round of the regimes, the second time with atol near rtol |b| and every other warm column scaled up, so that one positive
atol governs some converging columns of a block and rtol |b_j| the others (draw()).

What rotates with the case number, each at a period with no factor in common with another's or with one of
fuzz_solvers.TURNS, all below RUN: the width s over both sides of every tile boundary, 1, 2 and max_rhs; the layout of B
and X; n planted at the edges of the multi cell or drawn; the preconditioner's door; for amg_multi the AmgPlan's kind.
The stopping regime, check_every and GMRES's restart turn as in fuzz_solvers; family, degenerate shape and the planted row
(against SPMM_SPLIT_MIN: the product is an SpMM) rotate as structure() and drawn_plant() have them; a column's kind is
drawn.  Each operation has draw_<op>() and judge_<op>() (host only) and case_<op>() (device), which returns what the case
exercised; tests/test_fuzz_multi_host.py runs the host half, tests/test_gpu_fuzz_multi.py the cases and their census."""
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
import fuzz_solvers as FS
from fuzz_plans import FAMILIES, DAMAGE, DEGENERATE, RELATIONS, RUN, MIN_ROWS, structure, need   # imported, not copied: the census reads them here
from fuzz_solvers import conform, values, damaged_again, congruent, PLANTS, REGIMES, CHECK_EVERY, RESTARTS, RTOL, MAX_ITER
import numerics as NM
import krylov_numerics as KN
import sptrsv_numerics as TN
import solver_compose as SC
import multi_compose as MC
import gmres_multi_compose as GMC
import multi_parts as MP

OPS = ["pcg_multi", "bicgstab_multi", "gmres_multi", "sptrsm_tiled", "amg_multi"]
BASE = dict(pcg_multi="pcg", bicgstab_multi="bicgstab", gmres_multi="gmres")
LIMITS = S.krylov_multi_limits()
TILE, MAX_RHS, CELL = LIMITS["tile"], LIMITS["max_rhs"], LIMITS["cell"]
# both sides of every tile boundary up to max_rhs, and 1, 2
WIDTHS = sorted({1, 2} | {w for k in range(0, 7) for w in (TILE << k) + np.array([-1, 0, 1]) if 1 <= w <= MAX_RHS})
WIDTH_TURN = [int(WIDTHS[r % len(WIDTHS)]) for r in range(37)]
LAYOUTS = MP.LAYOUTS
LAYOUT_TURN = [LAYOUTS[r % 3] for r in range(41)]
SIZES = [CELL - 1, CELL, CELL + 1, 2 * CELL + 5]                          # n against the multi cell of the partial sums
SIZE_TURN = [SIZES[(r // 2) % 4] if r % 2 else None for r in range(43)]   # None: a drawn size
# the doors _multi_precond accepts; an AmgPlan is named kind/smoother
SEATED = ["ilu0", "amg/jacobi", "amg_smoothed/l1", "amg_device/jacobi", "amg/l1", "amg_smoothed/jacobi", "amg_device/l1"]
PRECONDS = [None, "jacobi"] + SEATED
# (the seated doors shift by one each round of seven, or one of them would fall on the degenerate cases, k % 7 == 3, every time)
# (and ILU(0) takes one more slot in nine: its level structures, wide and chain launches both, are the seat's hard part)
PRECOND_TURN = [SEATED[(r // 3 + r // 21) % 7] if r % 3 == 2 else "ilu0" if r % 9 == 4 else [None, "jacobi"][(r - r // 3) % 2] for r in range(47)]
AMG_DOORS = [p for p in SEATED if p != "ilu0"]
AMG_TURN = [AMG_DOORS[r % 6] for r in range(9)]                           # amg_multi only (not 7: k % 7 == 3 is always degenerate)
TURNS = dict(width=WIDTH_TURN, layout=LAYOUT_TURN, size=SIZE_TURN, precond=PRECOND_TURN, amg=AMG_TURN)
UNCHANGED = dict(regime=FS.REGIME_TURN, check_every=FS.CHECK_TURN, restart=FS.RESTART_TURN)
WRAPPER_PRECOND = {None: None, "jacobi": "jacobi", "amg/jacobi": "amg", "amg_smoothed/jacobi": "amg_smoothed"}
KINDS = ["random", "e_k", "zero", "large", "tiny", "nan"] + ["warm %g" % eps for eps in MC.WARM] + ["exact"]
# The composition's device calls a solve may cost: s * iterations * dots per iteration (the docstring).  Set from one
# timed run of tests/test_gpu_fuzz_multi.py beside tests/test_gpu_fuzz_plans.py (the test file's header has the times).  It
# cannot go below max_rhs * 6: one BiCGStab iteration at the widest width.
DOT_BUDGET = 384
DOTS = dict(pcg=3, bicgstab=6)
# A planted row makes a matrix of at least SPMM_SPLIT_MIN rows, on which every part of the composition is slow (an AMG cycle
# on such an arrow takes milliseconds), so the row is planted in one case of PLANT_EVERY only: the timed run asked for it.
# Any RUN consecutive cases still meet every relation to SPMM_SPLIT_MIN, on the test's seed with and without a seat.
PLANT_EVERY, PLANT_AT = 5, 1
B_NEAR, B_SCALE, B_NEAR_AT = 1e3, 1e4, 7                  # see draw(): regime (b)'s second place in REGIME_TURN
I32, F64 = np.int32, np.float64
FLOATS, EXACT = FS.FLOATS, FS.EXACT


def turn(case):
    out = {name: turns[case % len(turns)] for name, turns in TURNS.items()}
    out.update({name: turns[case % len(turns)] for name, turns in UNCHANGED.items()})
    return out


def door(precond):
    """a door's name -> (the key of multi_parts.Parts, the AmgPlan's smoother)"""
    if precond is None or "/" not in precond:
        return precond, "jacobi"
    return tuple(precond.split("/"))


def bounded(base, s, restart, max_iter, budget=None):
    """(restart, max_iter) lowered until s * max_iter * dots per iteration <= DOT_BUDGET: the restart first, and only as
    far as one iteration needs, then max_iter (at least 1)"""
    budget = DOT_BUDGET if budget is None else budget
    if base == "gmres":
        restart = max(1, min(restart, budget // s - 2))
        per = restart + 2
    else:
        per = DOTS[base]
    return restart, max(1, min(max_iter, budget // (s * per)))


def dot_product(P):
    """the bounded product of a drawn case"""
    per = P["restart"] + 2 if P["base"] == "gmres" else DOTS[P["base"]]
    return P["s"] * P["max_iter"] * per


# ---------------------------------------------------------------------------------------------------------------------
# the problem (host only)
# ---------------------------------------------------------------------------------------------------------------------
def matrix(base, case, rng, max_rows, precond, size, integer, seated=False):
    """fuzz_solvers.draw()'s matrix: -> (st, n, rp, ci, [val, D val D], planted row, size).  A degenerate shape comes as
    drawn, values too, and takes no preconditioner -- unless the operation is the preconditioner's own (seated): then it
    is conformed like every other shape."""
    plants = size is None and case % PLANT_EVERY == PLANT_AT
    st = structure(rng, max_rows, True, dict(spmm_split=S.SPMM_SPLIT_MIN) if plants else None, case, grow=1)
    if st["degenerate"] and not seated:                     # the shape and the values as drawn
        n, rp, ci, pr, size = st["rows"], st["rp"], st["ci"], None, None
        val = [rng.integers(-4, 5, len(ci)).astype(F64) if integer else rng.standard_normal(len(ci)), rng.standard_normal(len(ci))]
        return st, n, rp.astype(I32), ci.astype(I32), val, pr, size
    if st["degenerate"]:
        size = None
    if st["rows"] == 0:                                     # nothing to conform
        return st, 0, np.zeros(1, I32), np.zeros(0, I32), [np.zeros(0), np.zeros(0)], None, None
    n, rp, ci, pr = conform(base, rng, st, precond, size)
    first = values(rng, n, rp, ci, base == "pcg", integer)
    if base == "pcg" and precond is None:
        rp, ci, first = damaged_again(rng, st["damage"], n, rp, ci, first, pr)
    return st, n, rp.astype(I32), ci.astype(I32), [first, congruent(rng, n, rp, ci, first)], pr, size


def columns(rng, n, s, matvec1, integer):
    """(B, X0, kinds): every column's kind drawn from KINDS -- multi_compose.columns' seven and fuzz_solvers' exact guess
    on integer values -- with a random column always there and, from four columns on, a warm guess and a zero or NaN
    column too, so that a block's columns stop at different iterations"""
    pool = KINDS[:-1] + ["random", "random"] + (["exact"] if integer else [])
    kinds = [str(k) for k in rng.choice(pool, s)]
    where = rng.permutation(s)
    kinds[where[0]] = "random"
    if s >= 4:
        kinds[where[1]] = "warm %g" % MC.WARM[int(rng.integers(3))]
        kinds[where[2]] = str(rng.choice(["zero", "nan"]))
    B, X0 = np.zeros((n, s)), np.zeros((n, s))
    for j, kind in enumerate(kinds):
        b, x0 = rng.standard_normal(n), np.zeros(n)
        if kind == "e_k":
            b = np.zeros(n)
            b[int(rng.integers(n)) if n else 0:][:1] = 1.0
        elif kind == "zero":
            b, x0 = np.zeros(n), 0.1 * rng.standard_normal(n)               # x is cleared, whatever the guess
        elif kind == "large":
            b = 1e6 * b
        elif kind == "tiny":
            b = 1e-150 * b
        elif kind == "nan":
            b[int(rng.integers(n)) if n else 0:][:1] = np.nan
        elif kind.startswith("warm"):
            xs = rng.standard_normal(n)
            b, x0 = np.asarray(matvec1(xs), F64), xs + float(kind.split()[1]) * rng.standard_normal(n)
        elif kind == "exact":                                               # small integers on integer values: b = A x0 exactly
            x0 = rng.integers(-8, 9, n).astype(F64)
            b = np.asarray(matvec1(x0), F64)
        B[:, j], X0[:, j] = b, x0
    return B, X0, kinds


def draw(op, case, rng, max_rows):
    base, t = BASE[op], turn(case)
    s, integer = t["width"], bool(rng.random() < 0.3)
    st, n, rp, ci, val, pr, size = matrix(base, case, rng, max_rows, t["precond"], t["size"], integer)
    precond = None if st["degenerate"] else t["precond"]
    B, X0, kinds = columns(rng, n, s, lambda v: KN.matvec(n, rp, ci, val[0], v), integer)
    regime = t["regime"]
    ref = [j for j, k in enumerate(kinds) if k == "random"][0]              # atol is one number: a random column's |b| scales it
    bnorm = float(np.linalg.norm(B[:, ref]))
    # regime (b) comes twice in a round of the regimes: once with fuzz_solvers' atol, the larger bound for every column that
    # is not 1e6 times the scaling one, and once (near) with atol = B_NEAR rtol |b| and every other warm column -- b = A x*
    # and its guess alike, so it stays the same warm problem -- scaled by B_SCALE: that one stops on rtol |b_j|, far above
    # atol, the unscaled warm columns on atol, in one block, each after a few iterations
    near = regime == "b" and case % len(FS.REGIME_TURN) == B_NEAR_AT
    if near:
        for j in [j for j, k in enumerate(kinds) if k.startswith("warm")][::2]:
            B[:, j], X0[:, j] = B_SCALE * B[:, j], B_SCALE * X0[:, j]
    b_atol = B_NEAR * RTOL if near else 1e-6
    stop = dict(a=(RTOL, 0.0), b=(RTOL, b_atol * bnorm), c=(0.0, 1e-8 * bnorm), d=(RTOL, 0.0), e=(RTOL, 0.0), f=(0.0, 0.0))[regime]
    wanted = int(rng.integers(1, 13)) if regime == "f" else MAX_ITER
    # half the budget where the composition costs twice: a seated preconditioner is applied per column at the price of
    # several dots, and regimes (d) and (e) run the composition once more to learn its count
    budget = DOT_BUDGET // ((2 if precond in SEATED else 1) * (2 if regime in "de" else 1))
    restart, max_iter = bounded(base, s, t["restart"], wanted, budget)
    P = dict(op=op, base=base, st=st, n=n, rp=rp, ci=ci, val=val, B=B, X0=X0, kinds=kinds, s=s, layout=t["layout"], size=size,
             planted_row=pr, precond=precond, regime=regime, rtol=stop[0], atol=stop[1], max_iter=max_iter, bounded=max_iter < wanted,
             restart=restart if base == "gmres" else None, restart_drawn=t["restart"] if base == "gmres" else None,
             check_every=t["check_every"], integer=integer, budget=budget)
    P["params"] = FP.params_of(op, case, st, n=n, nnz=len(ci), size=size, s=s, layout=P["layout"], precond=precond, restart=P["restart"],
                               restart_drawn=P["restart_drawn"], regime=regime, rtol=P["rtol"], atol=P["atol"], max_iter=max_iter,
                               check_every=P["check_every"], kinds=kinds, planted_row=pr, integer=integer)
    return P


def draw_pcg_multi(case, rng, max_rows):
    return draw("pcg_multi", case, rng, max_rows)


def draw_bicgstab_multi(case, rng, max_rows):
    return draw("bicgstab_multi", case, rng, max_rows)


def draw_gmres_multi(case, rng, max_rows):
    return draw("gmres_multi", case, rng, max_rows)


# ---------------------------------------------------------------------------------------------------------------------
# the composition, the stopping regime and the judges (host only: the parts are callables)
# ---------------------------------------------------------------------------------------------------------------------
def compose(base, parts, B, X0, restart, rtol, atol, max_iter):
    """the lockstep loop of `base` on parts (matvec of a block, apply and dot of a column) -> a list of answers, one a column"""
    matvec, apply, dot = parts
    if base == "gmres":
        return GMC.composed_gmres_multi(matvec, apply, dot, B, X0, restart, rtol, max_iter, atol=atol)
    loop = MC.composed_pcg_multi if base == "pcg" else MC.composed_bicgstab_multi
    return [r.asdict() for r in loop(matvec, apply, dot, B, X0, rtol, max_iter, atol=atol)]


def host_parts(n, rp, ci, val, dinv=None):
    """the parts on the host, separable by column: the product by rows in numpy per column, the pinned dot's restatement"""
    one = lambda v: np.asarray(KN.matvec(n, rp, ci, val, v), F64)
    matvec = lambda V: np.stack([one(np.ascontiguousarray(V[:, j])) for j in range(V.shape[1])], axis=1) if V.shape[1] else V.copy()
    apply = (lambda v: v) if dinv is None else (lambda v: dinv * v)
    return matvec, apply, (lambda a, b: float(S.krylov_dot_ref(np.ascontiguousarray(a), np.ascontiguousarray(b))))


def single(P, val, j, rtol, atol, max_iter, dinv=None):
    """column j alone under fuzz_solvers' single composition on host parts"""
    x0 = np.ascontiguousarray(P["X0"][:, j])
    return FS.compose(P["base"], FS.host_parts(P["n"], P["rp"], P["ci"], val, dinv), np.ascontiguousarray(P["B"][:, j]), x0, P["restart"],
                      rtol, atol, max_iter)


def stopping(P, loop):
    """(rtol, atol, max_iter, what the regime expects of the composition or None).  loop(rtol, atol, max_iter) is the
    composition; regimes (d) and (e) run it once at regime (a) to learn the count of the column that converges last
    within the bounded max_iter, and stop one short of it or at it: expected = (column, status, iterations)."""
    rtol, atol, max_iter = P["rtol"], P["atol"], P["max_iter"]
    if P["regime"] in "de":
        learnt = loop(RTOL, 0.0, max_iter)
        there = [(w["iterations"], j) for j, w in enumerate(learnt) if w["status"] == "converged" and w["iterations"] >= 1]
        if there:
            count, j = max(there)
            if P["regime"] == "d":
                return rtol, atol, count - 1, (j, "limit", count - 1)
            return rtol, atol, count, (j, "converged", count)
    return rtol, atol, max_iter, None


def judge_expectation(P, want, expected, first=True):
    """what the regime and the columns' kinds say about the composition itself (first: the drawn values, to which an
    exact guess belongs)"""
    if expected is not None:
        j, status, count = expected
        need((want[j]["status"], want[j]["iterations"]) == (status, count), P, "the composition's column %d" % j, "ends in",
             (want[j]["status"], want[j]["iterations"]), "where the regime expects", (status, count))
    for j, kind in enumerate(P["kinds"]):
        if kind == "zero" or (kind == "exact" and first):
            w = want[j]
            need((w["status"], w["iterations"], w["rnorm"]) == ("converged", 0, 0.0), P, "column %d (%s)" % (j, kind), "does not end at iteration 0")
        if kind == "zero":
            need(not np.any(want[j]["x"]), P, "the zero column %d" % j, "is not cleared")


def judge(op, P, got, want, what="solve"):
    """every column: integers and strings on ==, floats on their bits (NaN as NaN)"""
    need(len(got) == len(want), P, what, "has", len(got), "columns for", len(want))
    for j, (g, w) in enumerate(zip(got, want)):
        FS.judge(BASE[op], P, g, w, "%s, column %d (%s)" % (what, j, P["kinds"][j] if "kinds" in P else "-"))


def judge_pcg_multi(P, got, want, what="solve"):
    judge("pcg_multi", P, got, want, what)


def judge_bicgstab_multi(P, got, want, what="solve"):
    judge("bicgstab_multi", P, got, want, what)


def judge_gmres_multi(P, got, want, what="solve"):
    judge("gmres_multi", P, got, want, what)


def column_problem(P, j):
    """column j as a fuzz_solvers problem, for that file's residual bar"""
    return dict(P, op=P["base"], b=np.ascontiguousarray(P["B"][:, j]), x0=np.ascontiguousarray(P["X0"][:, j]),
                precond=P["precond"] if P["precond"] in (None, "jacobi") else "other")


def bar_columns(P, want):
    """the columns that carry fuzz_solvers' residual bar: converged, on a drawn matrix without a preconditioner or with Jacobi"""
    if P["st"]["degenerate"] is not None or P["precond"] not in (None, "jacobi"):
        return []
    return [j for j, w in enumerate(want) if w["status"] == "converged"]


def judge_bar(P, val, got, want, rtol, atol):
    """fuzz_solvers.judge_residual per converged column -> the columns judged"""
    cols = bar_columns(P, want)
    for j in cols:
        Pj = column_problem(P, j)
        FS.judge_residual(Pj, val, got[j]["x"], FS.host_solution(Pj, val, rtol, atol)[1], rtol, atol)
    return cols


def _mixed_stop(want, rtol, atol):
    """one atol > 0 governed a column that converged after at least one iteration, and rtol |b_j| another of the block"""
    by = {rtol * w["bnorm"] >= atol for w in want if w["status"] == "converged" and w["iterations"] > 0}
    return bool(atol > 0.0 and by == {True, False})


def summary(P, want, rtol, atol, max_iter, bar):
    """what a solve's statuses exercised, for the census"""
    its = [int(w["iterations"]) for w in want]
    return dict(status=[w["status"] for w in want], iterations=its, max_iter=max_iter, bar=bar, spread=bool(MC.spread_ok(its)),
                atol_governed=[bool(w["status"] == "converged" and w["iterations"] > 0 and w["rnorm"] > rtol * w["bnorm"]) for w in want],
                mixed_stop=_mixed_stop(want, rtol, atol),
                restarts=[w.get("restarts") for w in want], columns=[w.get("columns") for w in want],
                zero_cleared=any(k == "zero" and P["X0"][:, j].any() and not np.any(w["x"]) for j, (k, w) in enumerate(zip(P["kinds"], want))))


# ---------------------------------------------------------------------------------------------------------------------
# a solver case on the device
# ---------------------------------------------------------------------------------------------------------------------
def answers(base, X, st):
    """a plan's (X, status dict) -> one answer a column"""
    x = X.cpu().numpy()
    out = []
    for j in range(x.shape[1]):
        a = dict(x=x[:, j].copy(), status=st["status"][j], iterations=int(st["iterations"][j]), breakdown=st["breakdown"][j],
                 rnorm=float(st["rnorm"][j]), bnorm=float(st["bnorm"][j]))
        if base == "gmres":
            a.update(restarts=int(st["restarts"][j]), columns=int(st["columns"][j]))
        else:
            a.update(alpha=float(st["alpha"][j]), beta=float(st["beta"][j]), omega=float(st["omega"][j]))
        out.append(a)
    return out


def make_plan(base, parts, restart):
    if base == "gmres":
        return S.GmresMultiPlan(parts.n, parts.drp, parts.dci, parts.s, restart=restart, precond=parts.seat)
    return S.KrylovMultiPlan(parts.n, parts.drp, parts.dci, parts.s, method=base, precond=parts.seat)


def wrapper_serves(P):
    """the one-shot wrappers make their own plans: the preconditioners they name, with their defaults"""
    return P["precond"] in WRAPPER_PRECOND


def solve_guarded(P, plan, parts, env, kw):
    """one solve in guarded blocks of the case's layout -> the answers; the canaries and B are checked"""
    _, torch, dev = env
    gB, gX = MP.blocks(torch, dev, P["layout"], P["B"], P["X0"])
    X, st = plan.solve(parts.dval, gB.view, X=gX.view, **kw, **parts.kw())
    need(X is gX.view and st["running"] == 0, P, "solve", "returns another X or leaves a column running")
    got = answers(P["base"], X, st)
    need(gB.intact() and gX.intact(), P, "solve", "wrote outside its blocks")
    need(KN.same_bits(gB.host(), P["B"]), P, "solve", "changed B")
    return got


def case_any(op, case, rng, dev, max_rows):
    import torch
    P = draw(op, case, rng, max_rows)
    base, n, s, B, X0 = P["base"], P["n"], P["s"], P["B"], P["X0"]
    env = (S, torch, dev)
    key, smoother = door(P["precond"])
    parts = MP.Parts(env, (n, P["rp"], P["ci"], P["val"][0]), s, key, smoother)
    plan = None
    seen = dict(split_rows=parts.spmm.split_info()["split_rows"] if parts.spmm is not None else None, wide=None, chain=None, levels=None)
    try:
        plan = make_plan(base, parts, P["restart"])
        if parts.ilu is not None:
            info = parts.ilu.info()
            seen["wide"], seen["chain"] = info["wide_launches"], info["chain_launches"]
        if parts.amg is not None:
            seen["levels"] = parts.amg.info()["levels"]
        solves = []
        for which, val in enumerate(P["val"]):
            if which:
                parts.revalue(val)                        # the factor and the AMG are set up again, on the same plans
            loop = lambda rtol, atol, max_iter: compose(base, (parts.matvec, parts.apply, parts.dot), B, X0, P["restart"], rtol, atol, max_iter)
            rtol, atol, max_iter, expected = stopping(P, loop)
            want = loop(rtol, atol, max_iter)
            what = "the second solve" if which else "solve"
            judge_expectation(P, want, expected, first=not which)
            kw = dict(rtol=rtol, atol=atol, max_iter=max_iter, check_every=P["check_every"])
            got = solve_guarded(P, plan, parts, env, kw)
            judge(op, P, got, want, what)
            if which == 0 and wrapper_serves(P):
                call = dict(pcg=S.pcg_multi, bicgstab=S.bicgstab_multi, gmres=S.gmres_multi)[base]
                more = dict(restart=P["restart"]) if base == "gmres" else {}
                wX, wst = call((n, parts.drp, parts.dci, parts.dval), FP.up(dev, B), precond=WRAPPER_PRECOND[P["precond"]],
                               X=FP.up(dev, X0) if X0.any() else None, **more, **kw)
                judge(op, P, answers(base, wX, wst), got, "the one-shot wrapper against the plan")
            bar = len(judge_bar(P, val, got, want, rtol, atol))
            solves.append(summary(P, want, rtol, atol, max_iter, bar))
    finally:
        if plan is not None:
            plan.destroy()
        parts.destroy()
    torch.cuda.synchronize()
    return census_of(P, solves=solves, wrapper=wrapper_serves(P), **seen)


def census_of(P, **more):
    out = FP.census_of(P["st"], n=P["n"], size=P["size"], s=P["s"], layout=P["layout"], precond=P["precond"], restart=P["restart_drawn"],
                       restart_used=P["restart"], regime=P["regime"], check_every=P["check_every"], kinds=sorted(set(P["kinds"])),
                       bounded=P["bounded"])
    out.update(more)
    return out


def case_pcg_multi(case, rng, dev, max_rows):
    return case_any("pcg_multi", case, rng, dev, max_rows)


def case_bicgstab_multi(case, rng, dev, max_rows):
    return case_any("bicgstab_multi", case, rng, dev, max_rows)


def case_gmres_multi(case, rng, dev, max_rows):
    return case_any("gmres_multi", case, rng, dev, max_rows)


# ---------------------------------------------------------------------------------------------------------------------
# sptrsm_tiled: SptrsvPlan.solve_multi and Ilu0Plan.apply_multi against their single-column entries
# ---------------------------------------------------------------------------------------------------------------------
SCHEDULES = 6                                             # fuzz_plans.schedules() has six


def draw_sptrsm_tiled(case, rng, max_rows):
    """draw_sptrsv's triangle and draw_ilu0's pattern, each with a block of the case's width and layout"""
    t = turn(case)
    s = t["width"]
    T, L = FP.draw_sptrsv(case, rng, max_rows), FP.draw_ilu0(case, rng, max_rows)
    P = dict(op="sptrsm_tiled", st=T["st"], T=T, L=L, s=s, layout=t["layout"], n=T["n"], B=NM.log_uniform(rng, (T["n"], s), 8),
             R=NM.log_uniform(rng, (L["n"], s), 8), schedule=int(rng.integers(SCHEDULES)), column=int(rng.integers(s)))
    P["params"] = dict(T["params"], op="sptrsm_tiled", s=s, layout=P["layout"], schedule=P["schedule"], column=P["column"],
                       ilu0=dict(rows=L["n"], nnz=len(L["ci"]), family=L["st"]["family"], plant=L["st"]["plant"]))
    return P


def judge_sptrsm_tiled(P, got, want, what="solve_multi"):
    """a block against the single-column entry's columns, on the bits"""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    need(got.shape == want.shape, P, what, "shape", got.shape, "for", want.shape)
    for j in range(want.shape[1]):
        need(KN.same_bits(got[:, j], want[:, j]), P, what, "column %d differs on the bits in" % j,
             int((KN.bits(got[:, j]) != KN.bits(want[:, j])).sum()), "of", want.shape[0], "entries")


def _columns_of(dev, host, solve_one):
    """solve_one on every column of the host block, as contiguous device vectors -> the (n, s) result"""
    n, s = host.shape
    out = np.zeros((n, s))
    for j in range(s):
        out[:, j] = solve_one(FP.up(dev, host[:, j])).cpu().numpy()
    return out


def _block_entry(P, env, host, entry, what):
    """a block entry out of place (B and X at the layout's two leading dimensions) and in place -> the two results"""
    _, torch, dev = env
    n, s = host.shape
    gB, gX = MP.blocks(torch, dev, P["layout"], host, np.full((n, s), MP.SENTINEL))
    X = entry(gB.view, gX.view)
    need(X is gX.view, P, what, "returns another X")
    apart = X.cpu().numpy()
    need(gB.intact() and gX.intact() and KN.same_bits(gB.host(), host), P, what, "wrote outside X or changed B")
    gI = MP.blocks(torch, dev, P["layout"], host, host)[1]
    need(entry(gI.view, gI.view) is gI.view, P, what, "in place returns another X")
    need(gI.intact(), P, what, "in place wrote outside its block")
    return apart, gI.host()


def case_sptrsm_tiled(case, rng, dev, max_rows):
    import torch
    P = draw_sptrsm_tiled(case, rng, max_rows)
    env, T, L = (S, torch, dev), P["T"], P["L"]
    label, kw = FP.schedules(T["widest"])[P["schedule"]]
    drp, dci, dval = FP.up(dev, T["rp"]), FP.up(dev, T["ci"]), FP.up(dev, T["val"])
    plan = S.SptrsvPlan(T["n"], drp, dci, lower=T["lower"], unit_diag=T["unit"], **kw)
    try:
        tinfo = plan.info()
        want = _columns_of(dev, P["B"], lambda b: plan.solve(dval, b, alpha=T["alpha"]))
        for got, how in zip(_block_entry(P, env, P["B"], lambda B, X: plan.solve_multi(dval, B, X=X, alpha=T["alpha"]), "solve_multi"),
                            ("out of place", "in place")):
            judge_sptrsm_tiled(P, got, want, "solve_multi %s (%s)" % (how, label))
        if T["n"]:                                        # the project's own bound on one column: the entry itself is sound
            try:
                TN.check_residual(T["n"], T["rp"], T["ci"], T["val"], P["B"][:, P["column"]], want[:, P["column"]], T["lower"], T["unit"],
                                  T["alpha"], what="fuzz")
            except AssertionError as e:
                need(False, P, "sptrsv residual", e)
    finally:
        plan.destroy()
    lrp, lci = FP.up(dev, L["rp"]), FP.up(dev, L["ci"])
    ilu = S.Ilu0Plan(L["n"], lrp, lci)
    try:
        linfo = ilu.info()
        for val in L["val"]:
            lu = ilu.factor(FP.up(dev, val))
            want = _columns_of(dev, P["R"], lambda r: ilu.apply(lu, r))
            for got, how in zip(_block_entry(P, env, P["R"], lambda R, out: ilu.apply_multi(lu, R, out=out), "apply_multi"),
                                ("out of place", "in place")):
                judge_sptrsm_tiled(P, got, want, "Ilu0Plan.apply_multi %s" % how)
    finally:
        ilu.destroy()
    torch.cuda.synchronize()
    return FP.census_of(P["st"], s=P["s"], layout=P["layout"], lower=T["lower"], unit=T["unit"], schedule=label, n=T["n"],
                        wide=tinfo["wide_launches"], chain=tinfo["chain_launches"], ilu_family=L["st"]["family"],
                        ilu_planted=(L["st"]["plant"]["name"], L["st"]["plant"]["rel"]) if L["st"]["plant"] else None,
                        ilu_wide=linfo["wide_launches"], ilu_chain=linfo["chain_launches"])


# ---------------------------------------------------------------------------------------------------------------------
# amg_multi: AmgPlan.apply_multi against apply per column
# ---------------------------------------------------------------------------------------------------------------------
def draw_amg_multi(case, rng, max_rows):
    """fuzz_solvers' SPD (even cases) and row-dominant (odd) problems, conformed as for a preconditioner; R and out are
    column slices of wider tensors; the second call, after a second setup, is narrower and reuses the reservation"""
    t = turn(case)
    base = "pcg" if case % 2 == 0 else "bicgstab"
    st, n, rp, ci, val, pr, size = matrix(base, case, rng, max_rows, t["amg"], t["size"], False, seated=True)
    s = t["width"]
    s2 = int(rng.integers(1, s + 1))
    layout = t["layout"] if t["layout"] != "contiguous" or case % 2 else "odd"     # contiguous only on odd cases: slices are the point
    P = dict(op="amg_multi", base=base, st=st, n=n, rp=rp, ci=ci, val=val, size=size, planted_row=pr, precond=t["amg"], s=s, s2=s2,
             layout=layout, R=[NM.log_uniform(rng, (n, s), 8), NM.log_uniform(rng, (n, s2), 8)])
    P["R"][0][:, int(rng.integers(s))] = 0.0               # a zero column among them
    P["params"] = FP.params_of("amg_multi", case, st, n=n, nnz=len(ci), size=size, base=base, precond=P["precond"], s=s, s2=s2, layout=layout,
                               planted_row=pr)
    return P


def judge_amg_multi(P, got, want, what="apply_multi"):
    judge_sptrsm_tiled(P, got, want, what)


def case_amg_multi(case, rng, dev, max_rows):
    import torch
    P = draw_amg_multi(case, rng, max_rows)
    n, env = P["n"], (S, torch, dev)
    key, smoother = door(P["precond"])
    drp, dci = FP.up(dev, P["rp"]), FP.up(dev, P["ci"])
    amg = S.AmgPlan(n, drp, dci, **SC.AMG_KINDS[key])
    try:
        levels, widths = amg.info()["levels"], []
        for which, (val, R) in enumerate(zip(P["val"], P["R"])):
            amg.setup(FP.up(dev, val), smoother=smoother)
            want = _columns_of(dev, R, lambda r: amg.apply(r))
            gR, gZ = MP.blocks(torch, dev, P["layout"], R, np.full(R.shape, MP.SENTINEL))
            out = amg.apply_multi(gR.view, out=gZ.view)
            need(out is gZ.view, P, "apply_multi", "returns another out")
            judge_amg_multi(P, out.cpu().numpy(), want, "apply_multi after setup %d" % which)
            need(gR.intact() and gZ.intact() and KN.same_bits(gR.host(), R), P, "apply_multi", "wrote outside out or changed R")
            widths.append(amg.multi_info()["width"])
        need(widths == [P["s"], P["s"]], P, "the reservation", "is", widths, "for", P["s"], "kept by the narrower call")
    finally:
        amg.destroy()
    torch.cuda.synchronize()
    return FP.census_of(P["st"], n=n, size=P["size"], base=P["base"], precond=P["precond"], s=P["s"], s2=P["s2"], layout=P["layout"], levels=levels)


# ---------------------------------------------------------------------------------------------------------------------
# the planted breakdowns, one column of a block: a breakdown in column j reaches no other column
# ---------------------------------------------------------------------------------------------------------------------
PLANT_WIDTH = TILE + 1                                    # two tiles; the planted column sits inside the first
PLANT_COLUMN = TILE // 2


def plant_block(plant):
    """-> (n, rp, ci, val, dinv, B, X0): fuzz_solvers' plant as column PLANT_COLUMN, small integer right-hand sides of the
    same tiny matrix round it (every sum stays exact)"""
    n, rp, ci, val, dinv, b = FS.plant_system(plant)
    rng = np.random.default_rng([len(plant["name"]), n])
    B = rng.integers(-3, 4, (n, PLANT_WIDTH)).astype(F64)
    B[:, PLANT_COLUMN] = b
    return n, rp, ci, val, dinv, B, np.zeros((n, PLANT_WIDTH))


def host_plant(plant):
    n, rp, ci, val, dinv, B, X0 = plant_block(plant)
    return compose(plant["op"], host_parts(n, rp, ci, val, dinv), B, X0, plant.get("restart"), **FS.PLANT_KW)


def case_plant(plant, dev):
    """the plant inside a block on the device: the planted column's literal, every column against the device's
    composition and the host's"""
    import torch
    n, rp, ci, val, dinv, B, X0 = plant_block(plant)
    base, P = plant["op"], FS.plant_params(plant)
    P["params"]["width"], P["base"], P["B"], P["X0"], P["layout"] = PLANT_WIDTH, base, B, X0, "odd"
    env = (S, torch, dev)
    parts = MP.Parts(env, (n, rp, ci, val), PLANT_WIDTH, None if dinv is None else "jacobi", dinv=dinv)
    plan = None
    try:
        plan = make_plan(base, parts, plant.get("restart"))
        want = compose(base, (parts.matvec, parts.apply, parts.dot), B, X0, plant.get("restart"), **FS.PLANT_KW)
        got = solve_guarded(P, plan, parts, env, dict(check_every=3, **FS.PLANT_KW))
    finally:
        if plan is not None:
            plan.destroy()
        parts.destroy()
    torch.cuda.synchronize()
    FS.judge_plant(plant, got[PLANT_COLUMN])
    op = base + "_multi"
    judge(op, P, got, want, "the planted block against the device's composition")
    judge(op, P, got, host_plant(plant), "the planted block against the host's composition")
    return dict(name=plant["name"], status=got[PLANT_COLUMN]["status"], breakdown=got[PLANT_COLUMN]["breakdown"],
                others=sorted(set(g["status"] for j, g in enumerate(got) if j != PLANT_COLUMN)))


DRAW = dict(pcg_multi=draw_pcg_multi, bicgstab_multi=draw_bicgstab_multi, gmres_multi=draw_gmres_multi, sptrsm_tiled=draw_sptrsm_tiled,
            amg_multi=draw_amg_multi)
JUDGE = dict(pcg_multi=judge_pcg_multi, bicgstab_multi=judge_bicgstab_multi, gmres_multi=judge_gmres_multi, sptrsm_tiled=judge_sptrsm_tiled,
             amg_multi=judge_amg_multi)
CASE = dict(pcg_multi=case_pcg_multi, bicgstab_multi=case_bicgstab_multi, gmres_multi=case_gmres_multi, sptrsm_tiled=case_sptrsm_tiled,
            amg_multi=case_amg_multi)


def case_rng(seed, op, case):
    return np.random.default_rng([seed, len(FP.OPS) + len(FS.OPS) + OPS.index(op), case])


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
        print("%s: all cases match" % op, flush=True)
    if args.only < 0:
        for plant in PLANTS:
            try:
                case_plant(plant, dev)
            except AssertionError as e:
                print("MISMATCH planted %s: %s" % (plant["name"], e), flush=True)
                return 1
        print("planted breakdowns: every planted column reaches its literal and every column matches its composition", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
