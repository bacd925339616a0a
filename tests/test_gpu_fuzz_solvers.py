"""A bounded run of tools/fuzz_solvers.py inside the GPU suite: PCG, BiCGStab and GMRES(m) on random structures, every
output of every solve held on its bits to the same solver composed from its parts on the device (tests/solver_compose.py),
the one-shot wrappers to the plans, a second solve with new values to its own composition, and a converged solve without
a preconditioner or with Jacobi also to a plain float64 host loop's residual (the tool's docstring has the details; a
failing case prints its parameters and the command line that replays it).

Every test ends with a census of what its cases exercised, so that the loop cannot pass by never reaching the hard
paths: every family, damage kind, degenerate shape, preconditioner, stopping regime, check_every, guess and right-hand
side, n at the edges of the partial sums' cell, the planted row around SPMV_SPLIT_MIN, and -- from the plans' info() and
the statuses -- a split row, ILU(0) with both kinds of launch, an AMG of three levels, restarts, all three endings, a
limit at exactly max_iter and a stop that atol governed.  tests/test_fuzz_solvers_host.py holds the same seed's
generators and judges to the host half of it without a GPU.  The planted breakdowns and one solve with more cells than
the fold has lanes are tests of their own."""
import importlib.util
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
import krylov_numerics as KN
import solver_compose as SC

pytestmark = pytest.mark.gpu

SEED = 5
CASES = 60
MAX_ROWS = 1500
# To be lowered for an operation whose test takes longer than the slowest of test_gpu_fuzz_plans.py in the same run on
# the same MI355X (the case count, the planted sizes and the planted row would stay).  Measured at max_rows = 1500 in one
# run of both files: test_pcg 3.9 s, test_bicgstab 3.2 s, test_gmres 4.7 s, against 4.9 s for test_gpu_fuzz_plans.py's
# test_softmax; the planted breakdowns and the three solves on 256 * 2048 + 3 rows take 0.2 s together.  Nothing is lowered.
LOWERED = dict()
BAR_CASES = 15                                            # cases of a run that must have carried the residual bar


def max_rows(op):
    return LOWERED.get(op, MAX_ROWS)


def load():
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)                         # the tool imports tools/fuzz_plans.py
    spec = importlib.util.spec_from_file_location("fuzz_solvers", os.path.join(tools, "fuzz_solvers.py"))
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    return fuzz


@pytest.fixture(scope="module")
def fuzz(sblas):
    return load()


def run(fuzz, op, cuda):
    """what every case exercised; the first mismatch fails the test with the case's parameters and its replay"""
    seen = []
    for case in range(CASES):
        try:
            seen.append(fuzz.run_case(op, case, SEED, cuda, max_rows(op)))
        except AssertionError as e:
            pytest.fail("%s\nreplay: python tools/fuzz_solvers.py --op %s --seed %d --max-rows %d --only %d" % (e, op, SEED, max_rows(op), case))
    return seen


def some(seen, cond):
    return any(cond(s) for s in seen)


def host_census(fuzz, seen, op):
    """the host half, all of it seen"""
    assert {s["family"] for s in seen if s["degenerate"] is None} == set(fuzz.FAMILIES)
    assert all(s["family"] is None for s in seen if s["degenerate"])       # a degenerate shape uses no family
    assert {s["damage"] for s in seen} == set(fuzz.DAMAGE)
    assert {s["degenerate"] for s in seen} == set(fuzz.DEGENERATE) | {None}
    assert all(s["precond"] is None for s in seen if s["degenerate"])      # ... and no preconditioner
    assert {s["precond"] for s in seen} == set(fuzz.PRECONDS)
    assert {s["planned"] for s in seen} == {True, False}
    assert {s["regime"] for s in seen} == set(fuzz.REGIMES)
    assert {s["check_every"] for s in seen} == set(fuzz.CHECK_EVERY)
    assert {s["x0"] for s in seen} == set(fuzz.X0_KINDS)
    assert {s["b"] for s in seen} == set(fuzz.B_KINDS) | {"exact"}
    if op == "gmres":
        assert {s["restart"] for s in seen} == set(fuzz.RESTARTS)
    assert {s["size"] for s in seen} == set(fuzz.SIZES) | {None}
    assert all(s["n"] == s["size"] for s in seen if s["size"] is not None)
    assert some(seen, lambda s: 0 < s["n"] < fuzz.CELL)
    planted = {s["planted"] for s in seen}
    assert None in planted
    for rel in fuzz.RELATIONS:
        assert ("spmv_split", rel) in planted, rel


def census(fuzz, seen, op):
    host_census(fuzz, seen, op)
    # from the plans' info()
    assert some(seen, lambda s: s["split_rows"] is not None and s["split_rows"] > 0)
    assert some(seen, lambda s: s["split_rows"] == 0)
    assert some(seen, lambda s: s["wide"] is not None and s["wide"] > 0 and s["chain"] > 0)
    assert some(seen, lambda s: s["levels"] is not None and s["levels"] >= 3)
    assert some(seen, lambda s: s["wrapper"]) and some(seen, lambda s: not s["wrapper"])
    solves = [(s, v) for s in seen for v in s["solves"]]
    assert all(len(s["solves"]) == 2 for s in seen)                         # the solve and the second solve with new values
    if op == "gmres":
        assert any(v["restarts"] >= 2 for s, v in solves)
        assert any(v["status"] == "converged" and 0 < v["columns"] < s["restart"] for s, v in solves)      # mid-cycle
        assert any(v["status"] == "converged" and v["columns"] == s["restart"] for s, v in solves)         # on a cycle's last column
    # the statuses
    assert {v["status"] for s, v in solves} == {"converged", "limit", "breakdown"}
    assert any(v["status"] == "limit" and v["iterations"] == v["max_iter"] > 0 for s, v in solves)
    assert any(v["atol_governed"] and s["regime"] in "bc" for s, v in solves)
    # the residual bar
    assert sum(1 for s in seen if s["solves"][0]["bar"]) >= BAR_CASES


def test_pcg(fuzz, cuda):
    census(fuzz, run(fuzz, "pcg", cuda), "pcg")


def test_bicgstab(fuzz, cuda):
    census(fuzz, run(fuzz, "bicgstab", cuda), "bicgstab")


def test_gmres(fuzz, cuda):
    census(fuzz, run(fuzz, "gmres", cuda), "gmres")


def test_planted_breakdowns(fuzz, cuda):
    """every denominator of the three solvers by a tiny exact system: the literal (status, name, iterations), and the bits
    of the device's composition and of the host's"""
    seen = []
    for plant in fuzz.PLANTS:
        try:
            seen.append(fuzz.case_plant(plant, cuda))
        except AssertionError as e:
            pytest.fail(str(e))
    assert {s["breakdown"] for s in seen} == {None, "(p, q)", "rho", "(r^, v)", "(t, t)", "omega", "givens", "beta"}
    assert {(p["op"], p["expect"][1]) for p in fuzz.PLANTS} >= {("pcg", "(p, q)"), ("pcg", "rho"), ("bicgstab", "(r^, v)"), ("bicgstab", "(t, t)"),
                                                               ("bicgstab", "omega"), ("bicgstab", "rho"), ("gmres", "givens"), ("gmres", "beta")}


BIG = KN.WIDTH * KN.CELL + 3                                                 # more cells than the fold has lanes, and a ragged last one


@pytest.fixture(scope="module")
def tridiagonal():
    """(-1, 4, -1) on BIG rows: the condition number is below 3, so every solver converges in a few dozen iterations"""
    n = BIG
    col = np.stack([np.arange(n) - 1, np.arange(n), np.arange(n) + 1], axis=1).reshape(-1)
    keep = (col >= 0) & (col < n)
    rp = np.concatenate([[0], np.cumsum(keep.reshape(n, 3).sum(axis=1))]).astype(np.int32)
    ci = col[keep].astype(np.int32)
    val = np.where(ci == np.repeat(np.arange(n), np.diff(rp)), 4.0, -1.0)
    return n, rp, ci, val, np.random.default_rng(30).standard_normal(n)


@pytest.mark.parametrize("op,precond,restart,rtol", [("pcg", "jacobi", None, 1e-10), ("bicgstab", None, None, 1e-10), ("gmres", None, 3, 1e-6)])
def test_a_solve_with_more_cells_than_the_fold_has_lanes(fuzz, sblas, cuda, tridiagonal, op, precond, restart, rtol):
    import torch
    n, rp, ci, val, b = tridiagonal
    parts = SC.Parts((sblas, torch, cuda), n, rp, ci, val, precond)
    plan = parts.plan(op if op != "gmres" else restart)
    try:
        want = fuzz.compose(op, (parts.matvec, parts.apply, parts.dot, parts.dots), b, None, restart, rtol, 0.0, 200)
        x, st = plan.solve(parts.dval, fuzz.FP.up(cuda, b), rtol=rtol, max_iter=200, check_every=8, **parts.kw())
        got = fuzz.answer(op, x, st)
    finally:
        plan.destroy()
        parts.destroy()
    print("%s on %d rows: %s after %d iterations, |r| = %.3e" % (op, n, st["status"], st["iterations"], st["rnorm"]))
    assert want["status"] == "converged" and 0 < want["iterations"] < 60
    fuzz.judge(op, dict(params=dict(op=op, n=n, precond=precond, restart=restart)), got, want)
