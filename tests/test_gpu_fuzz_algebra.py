"""A bounded run of tools/fuzz_algebra.py inside the GPU suite: masked SpGEMM, masked SpGEMM on SpGEMM's own pattern, CSR
addition, and the gradients of SpgemmOperator and csr_add in one graph, each on random structures against the library's
scalar references bit for bit (the tool's docstring has the details; a failing case prints its parameters and the command
line that replays it).

Every test ends with a census of what its cases exercised, so that the loop cannot pass by never reaching the hard
paths: every family, damage kind and degenerate shape, the planted row below, at, above and far above each limit, both
paths of every plan, a planted X row that begins inside a wave under both kinds of straddling wave, both arms of the
sorted kernel's walk and their tie, an exact fill of the last workgroup, one and two blocks of GEAM's scan, an empty run
that ends on a workgroup edge in both operands, the gradient plans with an X row beyond the LDS limit on either side.
tests/test_fuzz_algebra_host.py holds the same seed's generators to the host half of it without a GPU.

SEED = 5 met every item of all four censuses: no other seed was tried."""
import importlib.util
import os

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SEED = 5
CASES = 60
MAX_ROWS = 1500
# Lowered where a test takes longer than test_gpu_fuzz_plans.py's slowest on the same MI355X in the same run; the case count
# and the planted rows stay.  Measured in one run of the whole suite at max_rows = 1500: test_mspgemm 3.98 s,
# test_masked_spgemm_gives_spgemm_bits 3.41 s, test_grad 1.26 s, test_geam 0.31 s (in a run of this file), against 4.95 s
# for test_gpu_fuzz_plans.py::test_softmax: nothing is lowered.  test_mspgemm took 7.4 s while its Fraction judge added the
# products of a case term by term; the sample (200 entries, the planted row's first) was kept and the sums are now formed
# over one common denominator (fuzz_algebra.exact_sums).
LOWERED = dict()


def max_rows(op):
    return LOWERED.get(op, MAX_ROWS)


def load():
    spec = importlib.util.spec_from_file_location("fuzz_algebra", os.path.join(ROOT, "tools", "fuzz_algebra.py"))
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
            pytest.fail("%s\nreplay: python tools/fuzz_algebra.py --op %s --seed %d --max-rows %d --only %d" % (e, op, SEED, max_rows(op), case))
    return seen


def some(seen, cond):
    return any(cond(s) for s in seen)


def census(fuzz, seen, limits=()):
    """the host half: every family, damage kind and degenerate shape, and the planted row around every limit"""
    assert {s["family"] for s in seen if s["degenerate"] is None} == set(fuzz.FAMILIES)
    assert all(s["family"] is None for s in seen if s["degenerate"])
    assert {s["damage"] for s in seen} == set(fuzz.DAMAGE)
    assert {s["degenerate"] for s in seen} == set(fuzz.DEGENERATE) | {None}
    planted = {s["planted"] for s in seen}
    assert None in planted
    for name in limits:
        for rel in fuzz.RELATIONS:
            assert (name, rel) in planted, (name, rel)


def census_mspgemm_host(fuzz, seen):
    """what of test_mspgemm's census the host can tell"""
    census(fuzz, seen, ("lds_row",))
    assert {(s["x_ascending"], s["y_ascending"]) for s in seen} == {(a, b) for a in (False, True) for b in (False, True)}
    assert some(seen, lambda s: s["forced"])
    assert {s["regime"] for s in seen} == set(fuzz.REGIMES)
    assert some(seen, lambda s: s["staged_rows"] > 0) and some(seen, lambda s: s["unstaged_long_rows"] > 0)
    sorted_ = [s for s in seen if s["forced"]]                               # the cases whose auto plan takes the sorted kernel
    assert some(sorted_, lambda s: s["straddled_waves"] > 0)
    assert some(sorted_, lambda s: s["staged_then_long"] > 0) and some(sorted_, lambda s: s["long_then_staged"] > 0)
    assert {s["planted"][1] for s in sorted_ if s["planted"]} == set(fuzz.RELATIONS)
    assert some(sorted_, lambda s: s["mask_dups"]) and some(sorted_, lambda s: s["mask_unsorted"])
    assert some(seen, lambda s: s["workgroups"] > 1) and some(sorted_, lambda s: s["exact_fill"])
    assert {1, 7, 64, fuzz.S.mspgemm_limits()["lds_row"] + 40} <= {s["k"] for s in seen}


def census_mspgemm_walks(seen):
    sorted_ = [s for s in seen if s["forced"]]
    for key in ("walk_x", "walk_y", "walk_tie", "nopair_entries"):
        assert some(sorted_, lambda s: s[key] > 0), key
    assert some(seen, lambda s: s["judged_classes"] > 0)


def census_geam_host(fuzz, seen):
    census(fuzz, seen, ("scan", "wg"))
    assert {(s["a_ascending"], s["b_ascending"]) for s in seen} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {s["relation"] for s in seen} == set(fuzz.GEAM_RELATIONS)
    assert {s["regime"] for s in seen} == set(fuzz.REGIMES)
    sorted_ = [s for s in seen if s["a_ascending"] and s["b_ascending"]]
    blocks = {min(s["scan_blocks"], 3) for s in sorted_}
    assert blocks == {1, 2, 3}, blocks
    assert {s["planted"] for s in sorted_ if s["planted"]} >= {("scan", rel) for rel in fuzz.RELATIONS}
    assert some(sorted_, lambda s: s["empty_run_on_edge"])
    assert some(seen, lambda s: s["matched"] == 0 and s["nnz_b"] > 0) and some(seen, lambda s: 0 < s["matched"] < s["nnz_b"])
    assert some(sorted_, lambda s: s["matched"] == s["nnz_b"] == s["nnz_a"] > 0)
    assert some(seen, lambda s: s["scalars_zero"]) and some(seen, lambda s: not s["scalars_zero"])
    assert {"alike", "b_empty"} <= {s["nnz_ratio"] for s in seen} and {"a_16x", "b_16x"} & {s["nnz_ratio"] for s in seen}


def census_grad_host(fuzz, seen):
    census(fuzz, seen, ("lds_row",))
    assert {s["general"] for s in seen} == {False, True}
    assert some(seen, lambda s: s["no_pairs"]) and some(seen, lambda s: not s["no_pairs"])
    assert some(seen, lambda s: s["dup_a"]) and some(seen, lambda s: s["dup_b"])
    assert {s["need"] for s in seen} == set(fuzz.GRAD_NEED)
    assert some(seen, lambda s: s["long_x_a"]) and some(seen, lambda s: s["long_x_b"])
    assert {s["with_add"] for s in seen} == {False, True}
    assert {s["side"] for s in seen} == {"c_row", "a_column", None}


def test_mspgemm(fuzz, cuda):
    seen = run(fuzz, "mspgemm", cuda)
    census_mspgemm_host(fuzz, seen)
    census_mspgemm_walks(seen)
    assert {s["path"] for s in seen} == {"sorted", "general"}
    assert all((s["path"] == "sorted") == s["forced"] for s in seen)


def test_masked_spgemm_gives_spgemm_bits(fuzz, cuda):
    seen = run(fuzz, "mspgemm_spgemm", cuda)
    census(fuzz, seen, ("acc_cap", "s_max"))
    assert some(seen, lambda s: s["rows_row"] > 0) and some(seen, lambda s: s["rows_general"] > 0)
    assert some(seen, lambda s: s["chunks"] > 1)
    assert some(seen, lambda s: s["masked_paths"] == {"sorted", "general"}) and some(seen, lambda s: s["masked_paths"] == {"general"})


def test_geam(fuzz, cuda):
    seen = run(fuzz, "geam", cuda)
    census_geam_host(fuzz, seen)
    assert {s["path"] for s in seen} == {"sorted", "general"}
    assert some(seen, lambda s: s["scatter"])


def test_grad(fuzz, cuda):
    seen = run(fuzz, "grad", cuda)
    census_grad_host(fuzz, seen)
    for key in ("grad_a_path", "grad_b_path"):
        assert {s[key] for s in seen} == {"sorted", "general", None}, key
    assert some(seen, lambda s: s["long_x_a"] and s["grad_a_path"] == "sorted") and some(seen, lambda s: s["long_x_b"] and s["grad_b_path"] == "sorted")
    assert some(seen, lambda s: s["dense"])
