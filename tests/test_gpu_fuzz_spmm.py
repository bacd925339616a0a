"""A bounded run of tools/fuzz_spmm.py inside the GPU suite: SpMM through every entry point, order pair and type pair,
and SpMV through every selection, the plan and the typed entry, on random structures, row blocks, leading dimensions,
widths and switches, each output held to the numerics judges of tests/numerics.py -- the exact grids on ==, the
gamma(L+2) bound against the double-double reference, the IEEE classes -- and everything around the block to the bits it
had (the tool's docstring has the details; a failing case prints its parameters and the command line that replays it).

Every test ends with a census of what its cases exercised, so that the loop cannot pass by never reaching the hard
paths.  Its host half (census_host: the structures, the case mix, the switches, what the host rule launches for the call,
the staged widths and the column chunks, the split rows, the SpMV plan's item kinds and the planted row against its
limits) needs no device and is also held by tests/test_fuzz_spmm_host.py on the same seed; the device half reads the
library's own counters: panel_census() around the call, SpmmPlan.info() / split_info(), SpmvPlan.info()."""
import importlib.util
import os

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SEED = 3                     # (the other fuzz files' 5 draws no 384-column staging copy among its 60 spmm cases)
CASES = 60
MAX_ROWS = 1500
# Per operation: (max_rows, cap on nnz * n) where they had to come down for the time rule of test_gpu_fuzz_solvers.py: no
# test here may take longer than the slowest of test_gpu_fuzz_plans.py in the same run on the same MI355X.  Measured in
# one run at max_rows = 1500 and the tool's own cap: test_spmm 1.14 s, test_spmm_typed 0.68 s, test_spmv 0.13 s (and 2.0 s
# once for loading the tool) beside 4.92 s for test_gpu_fuzz_plans.py::test_softmax: nothing is lowered.
LOWERED = dict()


def max_rows(op):
    return LOWERED.get(op, (MAX_ROWS, None))[0]


def cap(fuzz, op):
    return LOWERED.get(op, (MAX_ROWS, None))[1] or fuzz.CAP


def load():
    spec = importlib.util.spec_from_file_location("fuzz_spmm", os.path.join(ROOT, "tools", "fuzz_spmm.py"))
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
            seen.append(fuzz.run_case(op, case, SEED, cuda, max_rows(op), cap(fuzz, op)))
        except AssertionError as e:
            pytest.fail("%s\nreplay: python tools/fuzz_spmm.py --op %s --seed %d --max-rows %d --cap %g --only %d" % (
                e, op, SEED, max_rows(op), cap(fuzz, op), case))
    assert not any(name in os.environ for name in fuzz.SWITCHES)             # the tool leaves no switch behind
    return seen


def some(seen, cond):
    return any(cond(s) for s in seen)


def census_host(fuzz, op, seen):
    """the half of the census that needs no device"""
    S = fuzz.S
    # structure and case mix
    assert {s["family"] for s in seen if s["degenerate"] is None} == set(fuzz.FAMILIES)
    assert all(s["family"] is None for s in seen if s["degenerate"])       # a degenerate shape uses no family
    assert {s["damage"] for s in seen} == set(fuzz.DAMAGE)
    assert {s["degenerate"] for s in seen} == set(fuzz.DEGENERATE) | {None}
    planted = {s["planted"] for s in seen}
    assert planted == {None} | {(name, rel) for name in fuzz.limits_of(op) for rel in fuzz.RELATIONS}, planted
    for key in ("rect", "block", "beta0") + (() if op == "spmv" else ("pad_b", "pad_c")):
        assert {s[key] for s in seen} == {False, True}, key
    assert {s["regime"] for s in seen} == set(fuzz.GRID) | {"general", "nonfinite"}
    assert {s["where"] for s in seen} == {None, "A", "B", "C"}
    entries = dict(spmm=fuzz.SPMM_ENTRIES, spmm_typed=fuzz.TYPED_ENTRIES, spmv=fuzz.SPMV_ENTRIES)[op]
    assert {s["entry"] for s in seen} == set(entries)
    name = lambda pair: (pair[0].__name__, pair[1].__name__)
    if op == "spmm":
        assert {s["types"] for s in seen} == {("float64", "int32")}
        for entry in ("split_plan", "ordered", "plan_ordered", "tensor", "tensor_plan"):
            assert {s["orders"] for s in seen if s["entry"] == entry} == set(fuzz.ORDERS), entry
    elif op == "spmm_typed":
        assert {(s["types"], s["entry"]) for s in seen} == {(name(t), e) for t in fuzz.TYPED for e in entries}
        assert {s["orders"] for s in seen if s["entry"] == "ordered"} == set(fuzz.ORDERS)
    else:
        assert {s["types"] for s in seen if s["entry"] == "typed"} == {name(t) for t in fuzz.TYPED}
        assert {s["env"].get("SBLAS_SPMV_VARIANT") for s in seen if s["entry"] == "variant"} == set(fuzz.SPMV_VARIANTS)
        assert all(s["n"] == 1 for s in seen)
    if op != "spmv":
        assert {s["n"] for s in seen} <= set(fuzz.WIDTHS) and len({s["n"] for s in seen}) >= 12
        assert {s["env"].get("SBLAS_SPMM_VARIANT", "auto") for s in seen} == set(fuzz.SPMM_VARIANTS)
        assert {s["env"].get("SBLAS_STAGE_RANGE") for s in seen} == {None, "0", "1"}
        assert {s["env"].get("SBLAS_SPMM_MIN_LDBT") for s in seen} == {None, "64"}
        assert some(seen, lambda s: "SBLAS_SPMM_MAX_BT_BYTES" in s["env"] and s["n"] == 256)
        assert some(seen, lambda s: "SBLAS_SPMM_MAX_BT_BYTES" in s["env"] and s["n"] == 300)
        assert some(seen, lambda s: "SBLAS_SPMM_MAX_BT_BYTES" not in s["env"] and s["n"] >= 256)
    if op == "spmm":
        # what the host rule launches for the call's sizes, staged width and switches (spmm_rule.cpp)
        for kernel in ("tiled", "mfma", "four_rows", "merge", "dpp_groups", "narrow", "rows8", "skip"):
            assert some(seen, lambda s: kernel in s["rule"]), kernel
        assert set().union(*(s["ldbt"] for s in seen)) == {8, 16, 32, 64, 128, 256, 384}
        assert some(seen, lambda s: s["chunks"] == 2) and some(seen, lambda s: s["chunks"] >= 3)
        # spmm_split_classify at the tool's split_min and piece: no row, a row, a row of several pieces
        assert some(seen, lambda s: s["split_rows"] == 0) and some(seen, lambda s: s["split_rows"] > 0)
        assert some(seen, lambda s: s["most_pieces"] > 2)
    if op == "spmv":
        # spmv_plan_classify: every kind of item, in a case that goes through the plan
        planned = [s for s in seen if s["entry"] == "plan"]
        kinds = set().union(*(s["kinds"] for s in planned))
        assert kinds >= {S.SPMV_ITEM_LPR, S.SPMV_ITEM_STREAM4096, S.SPMV_ITEM_STREAM6144, S.SPMV_ITEM_SEG, S.SPMV_ITEM_SPLIT}, kinds
        assert kinds & {S.SPMV_ITEM_LDS_S2, S.SPMV_ITEM_LDS_S3, S.SPMV_ITEM_LDS_S4, S.SPMV_ITEM_LDS_S7}, kinds
        assert some(planned, lambda s: s["split_pieces"] > 2)
        # the planted row below, at and above SPMV_SPLIT_MIN and the two stream tiers: its length is the block's longest
        for limit, value in fuzz.limits_of(op).items():
            for rel, L in (("below", value - 1), ("at", value), ("above", value + 1)):
                assert some(seen, lambda s: s["planted"] == (limit, rel) and s["longest"] == L), (limit, rel)


def test_spmm(fuzz, cuda):
    seen = run(fuzz, "spmm", cuda)
    census_host(fuzz, "spmm", seen)
    # the library's own counters.  panel_census() around the call:
    # ("fallback" too: the shuffled rows of the damage and the unsorted half of the planted rows reach panels the
    #  LDS-tiled kernel owns, which it then recomputes in the order the rows are stored in)
    for kind in ("windowed", "direct", "mfma", "fallback"):
        assert some(seen, lambda s: s["panels"][kind] > 0), kind
    assert some(seen, lambda s: s["panels"]["windowed"] > 0 and s["panels"]["direct"] > 0)      # both in one call
    # SpmmPlan.info() of the call's structure, width and switches
    for kind in ("windowed", "direct", "mfma", "merge", "four_rows"):
        assert some(seen, lambda s: s["plan"][kind]), kind
    assert some(seen, lambda s: s["plan"]["active"] and s["plan"]["stage_range"])
    assert some(seen, lambda s: s["plan"]["active"] and not s["plan"]["stage_range"])
    assert some(seen, lambda s: not s["plan"]["active"])
    # split_info() of the split plan: none, some, a row of several pieces -- and a call through such a plan
    assert some(seen, lambda s: s["split"]["split_rows"] == 0) and some(seen, lambda s: s["split"]["split_rows"] > 0)
    assert some(seen, lambda s: s["split"]["pieces"] > 2 * s["split"]["split_rows"] > 0)
    assert some(seen, lambda s: s["entry"] == "split_plan" and s["split"]["split_rows"] > 0 and "skip" in s["rule"])


def test_spmm_typed(fuzz, cuda):
    seen = run(fuzz, "spmm_typed", cuda)
    census_host(fuzz, "spmm_typed", seen)


def test_spmv(fuzz, cuda):
    seen = run(fuzz, "spmv", cuda)
    census_host(fuzz, "spmv", seen)
    planned = [s["plan"] for s in seen if s["entry"] == "plan"]
    for kind in ("lanes", "stream4096", "stream6144", "segmented", "lds", "split_rows"):
        assert some(planned, lambda info: info[kind] > 0), kind
    assert some(planned, lambda info: info["split_pieces"] > 2 * info["split_rows"] > 0)
    assert some(planned, lambda info: not info["active"]) and some(planned, lambda info: info["active"])
