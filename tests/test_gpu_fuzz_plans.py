"""A bounded run of tools/fuzz_plans.py inside the GPU suite: the transpose, COO assembly, SpGEMM, SDDMM, softmax, fused
attention, the triangular solves, ILU(0), the colouring with P A P^T, and the whole pipeline from triplets to a
preconditioner's action, each on random structures against the reference and at the bar of its own GPU test file (the
tool's docstring has the details; a failing case prints its parameters and the command line that replays it).

Every test ends with a census of what its cases exercised, so that the loop cannot pass by never reaching the hard
paths: every family, damage kind and degenerate shape, the planted row below, at and above each limit, and -- from the
plans' info() -- both kinds of launch, the long-row tier, the general path and several chunks, a split row, a non-zero
workspace.  tests/test_fuzz_plans_host.py holds the same seed's generators to the host half of it without a GPU."""
import importlib.util
import os

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SEED = 5
CASES = 60
PIPELINE_CASES = 8
MAX_ROWS = 1500
# Lowered for the operations whose test took longer than test_gpu_fuzz.py's own on the same MI355X at max_rows = 1500;
# the case count and the planted row stay.  Softmax and attention still take longer than it after that (about 4.9 s and
# 3.0 s for its 2.0 s): their time goes to the planted row itself, 4095 to 8195 entries that softmax_numerics and
# attention_numerics judge in Decimal and Fraction arithmetic in the 48 cases that have one, and neither a smaller matrix
# nor anything else short of judging fewer of its entries, or fewer cases, shortens that.
LOWERED = dict(transpose=600, spgemm=250, softmax=250, attention=250, ilu0=250)


def max_rows(op):
    return LOWERED.get(op, MAX_ROWS)


def load():
    spec = importlib.util.spec_from_file_location("fuzz_plans", os.path.join(ROOT, "tools", "fuzz_plans.py"))
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    return fuzz


@pytest.fixture(scope="module")
def fuzz(sblas):
    return load()


def run(fuzz, op, cuda, cases=CASES):
    """what every case exercised; the first mismatch fails the test with the case's parameters and its replay"""
    seen = []
    for case in range(cases):
        try:
            seen.append(fuzz.run_case(op, case, SEED, cuda, max_rows(op)))
        except AssertionError as e:
            pytest.fail("%s\nreplay: python tools/fuzz_plans.py --op %s --seed %d --max-rows %d --only %d" % (e, op, SEED, max_rows(op), case))
    return seen


def census(fuzz, seen, limits=()):
    """the host half: every family, damage kind and degenerate shape, and the planted row around every limit"""
    assert {s["family"] for s in seen if s["degenerate"] is None} == set(fuzz.FAMILIES)
    assert all(s["family"] is None for s in seen if s["degenerate"])       # a degenerate shape uses no family
    assert {s["damage"] for s in seen} == set(fuzz.DAMAGE)
    assert {s["degenerate"] for s in seen} == set(fuzz.DEGENERATE) | {None}
    planted = {s["planted"] for s in seen}
    assert None in planted                                                   # and a matrix without one
    for name in limits:
        for rel in fuzz.RELATIONS:
            assert (name, rel) in planted, (name, rel)


def some(seen, cond):
    return any(cond(s) for s in seen)


def test_transpose(fuzz, cuda):
    seen = run(fuzz, "transpose", cuda)
    census(fuzz, seen, ("spmv_split", "spmm_split"))
    assert some(seen, lambda s: s["split_rows"] > 0) and some(seen, lambda s: s["split_rows"] == 0)


def test_coo(fuzz, cuda):
    seen = run(fuzz, "coo", cuda)
    census(fuzz, seen, ("run",))
    assert some(seen, lambda s: s["triplets"] == 0) and some(seen, lambda s: s["longest_run"] > fuzz.COO_RUN)


def test_spgemm(fuzz, cuda):
    seen = run(fuzz, "spgemm", cuda)
    census(fuzz, seen, ("acc_cap", "s_max"))
    assert some(seen, lambda s: s["rows_row"] > 0) and some(seen, lambda s: s["rows_general"] > 0)
    assert some(seen, lambda s: s["chunks"] > 1)


def test_sddmm(fuzz, cuda):
    seen = run(fuzz, "sddmm", cuda)
    census(fuzz, seen)
    assert {s["k"] for s in seen} == {1, 3, 16, 17, 64, 130}
    assert some(seen, lambda s: s["block"]) and some(seen, lambda s: s["nonfinite"])
    assert some(seen, lambda s: s["beta"]) and some(seen, lambda s: not s["beta"])


def test_softmax(fuzz, cuda):
    seen = run(fuzz, "softmax", cuda)
    census(fuzz, seen, ("workspace",))
    assert some(seen, lambda s: s["workspace"] > 0) and some(seen, lambda s: s["workspace"] == 0)
    assert some(seen, lambda s: s["nonfinite"])


def test_attention(fuzz, cuda):
    seen = run(fuzz, "attention", cuda)
    census(fuzz, seen, ("workspace",))
    assert some(seen, lambda s: s["workspace"] > 0) and some(seen, lambda s: s["workspace"] == 0)
    assert {s["d"] for s in seen} == {1, 7, 64, 128} == {s["dv"] for s in seen}


def test_sptrsv(fuzz, cuda):
    seen = run(fuzz, "sptrsv", cuda)
    census(fuzz, seen, ("g4_max", "g16_max"))
    assert some(seen, lambda s: s["wide"] > 0 and s["chain"] > 0)
    assert {(s["lower"], s["unit"]) for s in seen} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {s["nrhs"] for s in seen} == {0, 1, 2, 5, 33}


def test_ilu0(fuzz, cuda):
    seen = run(fuzz, "ilu0", cuda)
    census(fuzz, seen, ("g4_max", "g16_max", "lds_max"))
    assert some(seen, lambda s: s["wide"] > 0 and s["chain"] > 0)
    assert some(seen, lambda s: s["long_rows"] > 0)


def test_colour_and_permute(fuzz, cuda):
    seen = run(fuzz, "color", cuda)
    census(fuzz, seen, ("g4_max", "g16_max", "window"))
    assert some(seen, lambda s: s["colors"] > fuzz.S.color_limits()["window"])


def test_pipeline_from_triplets_to_the_preconditioner(fuzz, cuda):
    seen = run(fuzz, "pipeline", cuda, PIPELINE_CASES)
    assert {s["family"] for s in seen} == {"grid5", "near_diagonal"}
    assert some(seen, lambda s: s["wide"] > 0) and some(seen, lambda s: s["chain"] > 0)
