"""ILU(0) without a GPU: the structure check (sblas_ilu0_check) against the restatement in tests/ilu0_numerics.py, every
refusal with its row and the order of the checks, the limits against csrc/ilu0.h, and the numpy references on exact data
and against their own error bound."""
import os
import re

import numpy as np
import pytest

import ilu0_numerics as IN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def accepted(S, n, rp, ci):
    want, bad = IN.check(n, rp, ci)
    assert bad is None
    got = S.ilu0_check(n, rp, ci)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(np.asarray(ci)[got], np.arange(n))
    return got


def refused(S, rp, ci):
    n = len(rp) - 1
    _, want = IN.check(n, rp, ci)
    with pytest.raises(S.SblasError) as e:
        S.ilu0_check(n, rp, ci)
    assert e.value.bad_row == want and "row %d" % want in str(e.value)
    return e.value.bad_row


def test_check_accepts_sorted_rows_with_a_diagonal(sblas, ash85):
    n = ash85["m"]
    rp, ci = IN.full_sorted(n, ash85["rowptr"], ash85["colidx"])
    accepted(sblas, n, rp, ci)
    accepted(sblas, 144, *IN.grid5(12))
    d = accepted(sblas, 500, *IN.csr_of_rows([[i] for i in range(500)]))
    assert np.array_equal(d, np.arange(500))
    assert len(accepted(sblas, 0, np.zeros(1, np.int32), np.zeros(0, np.int32))) == 0
    assert accepted(sblas, 1, np.array([0, 1], np.int32), np.array([0], np.int32)).tolist() == [0]
    rp, ci, first = IN.arrow_band([1, 4, 5, 33, 70])
    accepted(sblas, len(rp) - 1, rp, ci)


def test_every_refusal_names_its_row(sblas):
    rows = [[0, 1], [0, 1, 3], [1, 2], [0, 3, 4], [2, 4]]
    rp, ci = IN.csr_of_rows(rows)
    sblas.ilu0_check(5, rp, ci)                                             # sound as it stands
    assert refused(sblas, *IN.csr_of_rows([[0, 1], [0, 3, 1], [1, 2], [0, 3, 4], [2, 4]])) == 1   # unsorted
    assert refused(sblas, *IN.csr_of_rows([[0, 1], [0, 1, 3], [1, 2, 2], [0, 3, 4], [2, 4]])) == 2   # a doubled entry
    assert refused(sblas, *IN.csr_of_rows([[0, 1], [0, 1, 3], [1, 2], [0, 3, 3, 4], [2, 4]])) == 3   # a doubled diagonal
    assert refused(sblas, *IN.csr_of_rows([[0, 1], [0, 1, 3], [1, 2], [0, 4], [2, 4]])) == 3   # a missing diagonal
    assert refused(sblas, *IN.csr_of_rows([[0, 1], [0, 1, 3], [1, 2], [0, 3, 4], []])) == 4   # an empty row
    c = ci.copy()
    c[rp[3] + 2] = 5                                                        # row 3: a column == n
    assert refused(sblas, rp, c) == 3
    c = ci.copy()
    c[rp[1]] = -1                                                           # row 1: a negative column
    assert refused(sblas, rp, c) == 1
    r = rp.copy()
    r[3] = 4                                                                # row 2 ends before it starts
    assert refused(sblas, r, ci) == 2
    r = rp.copy()
    r[0] = 1
    assert refused(sblas, r, ci) == 0
    with pytest.raises(sblas.SblasError):
        sblas.ilu0_check(4, rp, ci)                                         # rowptr of another length


def test_the_order_of_the_checks_when_two_rows_are_bad(sblas):
    rows = [[0, 1], [0, 1, 3], [1, 2], [0, 3, 4], [2, 4]]
    rp, ci = IN.csr_of_rows(rows)
    # an unsorted row 1 and a column out of range in row 3: the ranges of every row come first
    rp2, ci2 = IN.csr_of_rows([[0, 1], [1, 0, 3], [1, 2], [0, 3, 9], [2, 4]])
    assert refused(sblas, rp2, ci2) == 3
    # ... and rowptr before either: row 4 ends before it starts
    r = rp2.copy()
    r[5] = r[4] - 1
    assert refused(sblas, r, ci2) == 4
    # row by row after that: a missing diagonal in row 1 is met before an unsorted row 2, and the other way round
    assert refused(sblas, *IN.csr_of_rows([[0, 1], [0, 3], [2, 1], [0, 3, 4], [2, 4]])) == 1
    assert refused(sblas, *IN.csr_of_rows([[0, 1], [1, 0], [1, 3], [0, 3, 4], [2, 4]])) == 1
    # within one row the outcome is the same whichever fault is met first
    assert refused(sblas, *IN.csr_of_rows([[0], [1], [3, 1], [3], [4]])) == 2


def header_constants():
    """NAME = value of every integer constexpr in sptrsv.h and ilu0.h, names resolved"""
    text = "".join(open(os.path.join(ROOT, "s-blas_amd", "csrc", f)).read() for f in ("sptrsv.h", "ilu0.h"))
    env = {}
    for name, expr in re.findall(r"constexpr\s+(?:int64_t|int)\s+(\w+)\s*=\s*([^;]+);", text):
        env[name] = int(eval(expr, {"__builtins__": {}}, dict(env)))
    return env


def test_limits_are_the_header_s_constants(sblas):
    lim, h = sblas.ilu0_limits(), header_constants()
    assert lim == dict(chain_rows=h["ILU0_CHAIN_ROWS"], chain_threads=h["ILU0_CHAIN_THREADS"], g4_max=h["SPTRSV_G4_MAX"],
                       g16_max=h["SPTRSV_G16_MAX"], lds_max=h["ILU0_LDS_MAX"], wide_threads=h["ILU0_WIDE_THREADS"])
    assert lim["chain_rows"] == sblas.sptrsv_limits()["chain_rows"] == 32   # the solves' default, until a sweep says otherwise
    assert lim["lds_max"] == 64 * h["ILU0_LDS_PER_LANE"] and lim["g16_max"] <= 16 * h["ILU0_LDS_PER_LANE"]
    assert lim["chain_threads"] % 64 == 0 and lim["wide_threads"] % 64 == 0
    assert lim["chain_threads"] * h["ILU0_LDS_PER_LANE"] * 12 <= 160 * 1024  # the chain workgroup's LDS fits a CU


# ---- the numpy references ----------------------------------------------------------------------------------------------
def test_reference_recovers_l0_and_u0_where_no_fill_arises():
    rng = np.random.default_rng(1)
    rp, ci, val, lu0 = IN.exact_bidiagonal_product(rng, 300)
    assert np.array_equal(IN.ilu0_ref(300, rp, ci, val), lu0)
    assert IN.residual_ratio(300, rp, ci, val, lu0) == 0.0


def residual_inputs():
    rng = np.random.default_rng(2)
    return [("grid 12", 144) + IN.grid5(12), ("random 150", 150) + IN.random_near_diagonal(rng, 150, 12, 150),
            ("band 120", 120) + IN.band(120, 20)]


@pytest.mark.parametrize("case", range(3))
def test_reference_meets_the_residual_bound_and_a_perturbed_factor_does_not(case):
    name, n, rp, ci = residual_inputs()[case]
    rng = np.random.default_rng(10 + case)
    val = IN.dominant_values(rng, n, rp, ci)
    lu = IN.ilu0_ref(n, rp, ci, val)
    ratio = IN.residual_ratio(n, rp, ci, val, lu)
    print("%s: residual / bound at most %.3g" % (name, ratio))
    assert 0.0 < ratio <= 1.0
    bad = lu.copy()
    bad[len(bad) // 2] *= 1 + 1e-12
    assert IN.residual_ratio(n, rp, ci, val, bad) > 1.0
