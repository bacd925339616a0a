"""A bounded run of tools/fuzz_multi.py inside the GPU suite: the multi-right-hand-side PCG, BiCGStab and GMRES(m) on random
structures, every output of every column held on its bits to the lockstep loop composed from its parts on the device
(tests/multi_compose.py, tests/gmres_multi_compose.py on tests/multi_parts.py), the one-shot wrappers to the plans, a
second solve with new values to its own composition, a converged column without a preconditioner or with Jacobi also to
a plain float64 host loop's residual; and the block applies (SptrsvPlan.solve_multi, Ilu0Plan.apply_multi,
AmgPlan.apply_multi) column by column on the bits against their single-column entries (the tool's docstring has the
details; a failing case prints its parameters and the command line that replays it).

Every test ends with a census of what its cases exercised, so that the loop cannot pass by never reaching the hard
paths.  tests/test_fuzz_multi_host.py holds the same seed's generators, compositions and judges to the host half of it
without a GPU.  One census item of the solver operations rests on a fact of the library: the
multi-right-hand-side plans make an UNSPLIT SpMM plan (sblas_hip_spmm_plan_create), so no row is ever cut into pieces
under them, however long; the census therefore asserts the planted row at every relation to SPMM_SPLIT_MIN (drawn) and
that the plan's product, made as the solvers make theirs, reports no split row -- a split plan under the solvers would
show here first.

Times, from one run of this file and tests/test_gpu_fuzz_plans.py on the same MI355X: test_pcg_multi 3.4 s,
test_bicgstab_multi 2.9 s, test_gmres_multi 2.0 s, test_amg_multi 1.3 s, test_sptrsm_tiled 0.8 s, test_planted_breakdowns
0.2 s, against 5.0 s for test_gpu_fuzz_plans.py's test_softmax.  The first timed run, at 60 cases an operation with the
row planted in four cases of five, took 16 s a solver test: what brought it down is in the comments below and at
DOT_BUDGET and PLANT_EVERY in the tool."""
import importlib.util
import os
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SEED = 8
# the smallest counts at which each operation's census holds for SEED, found in one run of 60 cases an operation on the GPU
CASES = dict(pcg_multi=37, bicgstab_multi=37, gmres_multi=37, sptrsm_tiled=44, amg_multi=37)
MAX_ROWS = 1500
# max_rows would be lowered here for an operation whose test takes longer than the slowest of test_gpu_fuzz_plans.py in the
# same run, after DOT_BUDGET.  It is not: DOT_BUDGET already stands at its floor (one BiCGStab iteration at max_rhs
# columns), and the rows of a case come from the planted row (at least SPMM_SPLIT_MIN of them) and the planted sizes, not
# from max_rows -- so the tool plants the row in one case of five, halves the budget where the composition costs twice
# (a seated preconditioner; regimes (d), (e)), and the case counts are the smallest at which the census holds.
LOWERED = dict()
BAR_CASES = 15                                            # blocks of a run that must have carried the residual bar
SPREAD_BLOCKS = 3                                         # blocks whose stopping iterations meet multi_compose.spread_ok


def max_rows(op):
    return LOWERED.get(op, MAX_ROWS)


def load():
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)                         # the tool imports tools/fuzz_solvers.py and tools/fuzz_plans.py
    spec = importlib.util.spec_from_file_location("fuzz_multi", os.path.join(tools, "fuzz_multi.py"))
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    return fuzz


@pytest.fixture(scope="module")
def fuzz(sblas):
    return load()


def run(fuzz, op, cuda):
    """what every case exercised; the first mismatch fails the test with the case's parameters and its replay"""
    seen = []
    for case in range(CASES[op]):
        try:
            seen.append(fuzz.run_case(op, case, SEED, cuda, max_rows(op)))
        except AssertionError as e:
            pytest.fail("%s\nreplay: python tools/fuzz_multi.py --op %s --seed %d --max-rows %d --only %d" % (e, op, SEED, max_rows(op), case))
    return seen


def some(seen, cond):
    return any(cond(s) for s in seen)


def structure_census(fuzz, seen, limit=None):
    """the shared generator's half: every family, damage kind and degenerate shape, every width and layout"""
    assert {s["family"] for s in seen if s["degenerate"] is None} == set(fuzz.FAMILIES)
    assert all(s["family"] is None for s in seen if s["degenerate"])       # a degenerate shape uses no family
    assert {s["damage"] for s in seen} == set(fuzz.DAMAGE)
    assert {s["degenerate"] for s in seen} == set(fuzz.DEGENERATE) | {None}
    assert {s["s"] for s in seen} == set(fuzz.WIDTHS)
    assert {s["layout"] for s in seen} == set(fuzz.LAYOUTS)
    planted = {s["planted"] for s in seen}
    assert None in planted
    for name in ([limit] if isinstance(limit, str) else limit or []):
        for rel in fuzz.RELATIONS:
            assert (name, rel) in planted, (name, rel)


def sizes_census(fuzz, seen):
    assert {s["size"] for s in seen} == set(fuzz.SIZES) | {None}
    assert all(s["n"] == s["size"] for s in seen if s["size"] is not None)
    assert some(seen, lambda s: 0 < s["n"] < fuzz.CELL)


def host_census(fuzz, seen, op):
    """the host half of a solver operation's census, all of it drawn"""
    structure_census(fuzz, seen, "spmm_split")
    sizes_census(fuzz, seen)
    assert all(s["precond"] is None for s in seen if s["degenerate"])      # a degenerate shape takes no preconditioner
    assert {s["precond"] for s in seen if s["degenerate"] is None} == set(fuzz.PRECONDS)       # every door on a drawn family
    assert {s["regime"] for s in seen} == set(fuzz.REGIMES)
    assert {s["check_every"] for s in seen} == set(fuzz.CHECK_EVERY)
    assert {k for s in seen for k in s["kinds"]} == set(fuzz.KINDS)
    if op == "gmres_multi":
        assert {s["restart"] for s in seen} == set(fuzz.RESTARTS)
    assert some(seen, lambda s: s["bounded"]) and some(seen, lambda s: not s["bounded"])


def status_census(seen, op, bar_cases, spread_blocks, mixed=True):
    """from the statuses of the compositions (which the device has been held to, column by column); mixed=False: without
    the block of mixed stops, which for PCG occurs under a seat only (the host test cannot compose those cases)"""
    solves = [(s, v) for s in seen for v in s["solves"]]
    columns = [(s, v, j) for s, v in solves for j in range(len(v["status"]))]
    assert {v["status"][j] for s, v, j in columns} == {"converged", "limit", "breakdown"}
    assert any(set(v["status"]) == {"converged", "limit", "breakdown"} for s, v in solves)          # one block with all three
    assert sum(1 for s, v in solves if v["spread"]) >= spread_blocks                                # the freeze is exercised
    assert any(v["status"][j] == "limit" and v["iterations"][j] == v["max_iter"] > 0 for s, v, j in columns)
    assert any(v["atol_governed"][j] and s["regime"] in "bc" for s, v, j in columns)
    assert not mixed or any(v["mixed_stop"] and s["regime"] == "b" for s, v in solves)     # one atol > 0: some columns stop on it, others on rtol |b_j|
    assert any(v["zero_cleared"] for s, v in solves)
    if op == "gmres_multi":
        assert any(v["restarts"][j] >= 2 for s, v, j in columns)
        assert any(v["status"][j] == "converged" and 0 < v["columns"][j] < s["restart_used"] for s, v, j in columns)      # mid-cycle
        assert any(v["status"][j] == "converged" and v["columns"][j] == s["restart_used"] for s, v, j in columns)         # on a cycle's last column
    assert sum(1 for s in seen if s["solves"][0]["bar"]) >= bar_cases


def census(fuzz, seen, op):
    host_census(fuzz, seen, op)
    assert all(len(s["solves"]) == 2 for s in seen)                         # the solve and the second solve with new values
    # from the plans' info(): the product is the unsplit plan's (the header); ILU(0) with both kinds of launch; a deep AMG
    assert all(s["split_rows"] in (None, 0) for s in seen) and some(seen, lambda s: s["split_rows"] == 0)
    assert some(seen, lambda s: s["wide"] is not None and s["wide"] > 0 and s["chain"] > 0)
    assert some(seen, lambda s: s["levels"] is not None and s["levels"] >= 3)
    assert some(seen, lambda s: s["wrapper"]) and some(seen, lambda s: not s["wrapper"])
    status_census(seen, op, BAR_CASES, SPREAD_BLOCKS)


def test_pcg_multi(fuzz, cuda):
    census(fuzz, run(fuzz, "pcg_multi", cuda), "pcg_multi")


def test_bicgstab_multi(fuzz, cuda):
    census(fuzz, run(fuzz, "bicgstab_multi", cuda), "bicgstab_multi")


def test_gmres_multi(fuzz, cuda):
    census(fuzz, run(fuzz, "gmres_multi", cuda), "gmres_multi")


def sptrsm_census(fuzz, seen):
    structure_census(fuzz, seen, ["g4_max", "g16_max"])
    assert {s["lower"] for s in seen} == {True, False} and {s["unit"] for s in seen} == {True, False}
    assert len({s["schedule"] for s in seen}) == fuzz.SCHEDULES
    assert {s["ilu_family"] for s in seen if s["degenerate"] is None} == set(fuzz.FAMILIES)
    for name in ("g4_max", "g16_max", "lds_max"):
        for rel in fuzz.RELATIONS:
            assert some(seen, lambda s: s["ilu_planted"] == (name, rel)), (name, rel)


def test_sptrsm_tiled(fuzz, cuda):
    seen = run(fuzz, "sptrsm_tiled", cuda)
    sptrsm_census(fuzz, seen)
    assert some(seen, lambda s: s["wide"] > 0 and s["chain"] > 0) and some(seen, lambda s: s["wide"] == 0 and s["chain"] > 0)     # a chain-only triangle
    assert some(seen, lambda s: s["ilu_wide"] > 0 and s["ilu_chain"] > 0)


def amg_census(fuzz, seen):
    structure_census(fuzz, seen, "spmm_split")
    sizes_census(fuzz, seen)
    assert {s["precond"] for s in seen if s["degenerate"] is None} == set(fuzz.AMG_DOORS)      # every door on a drawn family
    assert {s["base"] for s in seen} == {"pcg", "bicgstab"}
    assert some(seen, lambda s: s["s2"] < s["s"])                           # a narrower call inside a wider reservation


def test_amg_multi(fuzz, cuda):
    seen = run(fuzz, "amg_multi", cuda)
    amg_census(fuzz, seen)
    assert some(seen, lambda s: s["levels"] >= 3) and some(seen, lambda s: s["levels"] == 1)


def test_planted_breakdowns(fuzz, cuda):
    """every denominator of the three solvers by a tiny exact system, placed as one column of a block: that column reports
    the literal (status, name, iterations) of the single plant, and every column has the bits of the device's composition
    and of the host's -- a breakdown in column j reaches no other column"""
    seen = []
    for plant in fuzz.PLANTS:
        try:
            seen.append(fuzz.case_plant(plant, cuda))
        except AssertionError as e:
            pytest.fail(str(e))
    assert {s["breakdown"] for s in seen} == {None, "(p, q)", "rho", "(r^, v)", "(t, t)", "omega", "givens", "beta"}
    assert some(seen, lambda s: s["status"] == "breakdown" and "converged" in s["others"])              # the others went on
