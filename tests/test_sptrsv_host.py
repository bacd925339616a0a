"""The triangular solve without a GPU: the plan's host rule (sblas_sptrsv_levels, sblas_sptrsv_schedule,
sblas_hip_sptrsv_limits) against the restatement in tests/sptrsv_numerics.py, the refusals with their bad rows, and the
numpy references against each other on exact data."""
import numpy as np
import pytest

import sptrsv_numerics as TN

WIDE, CHAIN = 0, 1


def check_levels(S, n, rp, ci, lower, unit=False):
    lv, nl = S.sptrsv_levels(n, rp, ci, lower=lower, unit_diag=unit)
    want, want_nl = TN.levels(n, rp, ci, lower)
    assert nl == want_nl
    assert np.array_equal(lv, want)
    return lv, nl


@pytest.mark.parametrize("lower", [True, False])
def test_levels_of_ash85(sblas, ash85, lower):
    n = ash85["m"]
    rp, ci = TN.triangle_of(n, ash85["rowptr"], ash85["colidx"], lower)
    lv, nl = check_levels(sblas, n, rp, ci, lower)
    assert nl > 1 and len(lv) == 85


def test_levels_of_the_grid_are_its_antidiagonals(sblas):
    side = 48
    for lower in (True, False):
        rp, ci = TN.grid5(side, lower)
        lv, nl = check_levels(sblas, side * side, rp, ci, lower)
        assert nl == 2 * side - 1 == 95
        assert TN.level_widths(lv, nl).tolist() == list(range(1, side + 1)) + list(range(side - 1, 0, -1))


def test_levels_of_a_bidiagonal_chain_a_diagonal_and_an_arrow(sblas):
    rp, ci = TN.bidiagonal(3000)
    lv, nl = check_levels(sblas, 3000, rp, ci, True)
    assert nl == 3000 and np.array_equal(lv, np.arange(3000))
    lv, nl = check_levels(sblas, 3000, rp, ci, False)                       # as an upper triangle: the diagonal alone
    assert nl == 1
    rp, ci = TN.diagonal(500)
    assert check_levels(sblas, 500, rp, ci, True)[1] == 1
    rp, ci = TN.arrow(200)
    lv, nl = check_levels(sblas, 200, rp, ci, True)
    assert nl == 3 and TN.level_widths(lv, nl).tolist() == [1, 198, 1]      # row 0; the rows that name it; the last row


def test_levels_of_unsorted_rows_with_duplicates_and_both_triangles(sblas):
    rng = np.random.default_rng(3)
    rp, ci = TN.messy(rng, 300)
    for lower in (True, False):
        check_levels(sblas, 300, rp, ci, lower)


def test_levels_under_a_unit_diagonal_with_and_without_stored_diagonals(sblas):
    rng = np.random.default_rng(4)
    rp, ci = TN.messy(rng, 120)
    lv_with, nl = check_levels(sblas, 120, rp, ci, True, unit=True)
    keep = ~TN.on_diagonal(rp, ci)                                          # the same matrix without its diagonals
    rp2 = np.zeros(121, np.int32)
    rp2[1:] = np.cumsum(np.bincount(np.repeat(np.arange(120), np.diff(rp))[keep], minlength=120))
    lv_without, nl2 = check_levels(sblas, 120, rp2, ci[keep], True, unit=True)
    assert nl == nl2 and np.array_equal(lv_with, lv_without)
    with pytest.raises(sblas.SblasError) as e:                              # and without unit, the first row lacks one
        sblas.sptrsv_levels(120, rp2, ci[keep])
    assert e.value.bad_row == 0


def test_trivial_sizes(sblas):
    lv, nl = sblas.sptrsv_levels(0, np.zeros(1, np.int32), np.zeros(0, np.int32))
    assert nl == 0 and len(lv) == 0
    lv, nl = sblas.sptrsv_levels(1, np.array([0, 1], np.int32), np.array([0], np.int32))
    assert nl == 1 and lv.tolist() == [0]
    lv, nl = sblas.sptrsv_levels(1, np.array([0, 0], np.int32), np.zeros(0, np.int32), unit_diag=True)
    assert nl == 1
    kind, first = sblas.sptrsv_schedule([])
    assert len(kind) == 0 and first.tolist() == [0]
    kind, first = sblas.sptrsv_schedule([1])
    assert kind.tolist() == [CHAIN] and first.tolist() == [0, 1]


def test_refusals_report_the_first_bad_row(sblas):
    rows = [[0], [0, 1], [1, 2], [3, 0], [4]]
    rp, ci = TN.csr_of_rows(rows)

    def refused(rp, ci, **kw):
        with pytest.raises(sblas.SblasError) as e:
            sblas.sptrsv_levels(len(rp) - 1, rp, ci, **kw)
        assert "row %d" % e.value.bad_row in str(e.value)
        return e.value.bad_row

    sblas.sptrsv_levels(5, rp, ci)                                          # sound as it stands
    r2, c2 = TN.csr_of_rows([[0], [0, 1], [1], [3, 0], [0]])                # missing diagonals in rows 2 and 4
    assert refused(r2, c2) == 2
    sblas.sptrsv_levels(5, r2, c2, unit_diag=True)                          # which a unit diagonal does not need
    r3, c3 = TN.csr_of_rows([[0], [1, 0, 1], [2], [3, 3], [4]])             # duplicated diagonals in rows 1 and 3
    assert refused(r3, c3) == 1
    c4 = ci.copy()
    c4[5] = 5                                                               # row 3: a column == n
    assert refused(rp, c4) == 3
    assert refused(rp, c4, unit_diag=True) == 3
    c5 = ci.copy()
    c5[1] = -1                                                              # row 1: a negative column
    assert refused(rp, c5) == 1
    r6 = rp.copy()
    r6[3] = 2                                                               # row 2 ends before it starts
    assert refused(r6, ci) == 2
    r7 = rp.copy()
    r7[0] = 1
    assert refused(r7, ci) == 0


def covered(kind, first, n_levels):
    assert len(first) == len(kind) + 1
    assert first[0] == 0 and first[-1] == n_levels
    assert np.all(np.diff(first) >= 1)                                      # in order, every level once, no empty launch


@pytest.mark.parametrize("chain_rows", [1, 7, 8, 9, 0, 10 ** 9])
def test_schedule_in_every_mode(sblas, chain_rows):
    default = sblas.sptrsv_limits()["chain_rows"]
    cr = chain_rows or default
    rng = np.random.default_rng(chain_rows % 97)
    shapes = [list(range(1, 49)) + list(range(47, 0, -1)), [1] * 50, [8, 8, 9, 9, 7, 8, 9, 1, 20, 8],
              list(rng.integers(1, 18, 200)), [default - 1, default, default + 1, default, default + 1, default + 2, 1], [5]]
    for widths in shapes:
        L = len(widths)
        kind, first = sblas.sptrsv_schedule(widths, "per_level", chain_rows)
        covered(kind, first, L)
        assert len(kind) == L and not kind.any()
        kind, first = sblas.sptrsv_schedule(widths, "chain", chain_rows)
        covered(kind, first, L)
        assert kind.tolist() == [CHAIN]
        kind, first = sblas.sptrsv_schedule(widths, "auto", chain_rows)
        covered(kind, first, L)
        for q in range(len(kind)):
            ws = widths[first[q]:first[q + 1]]
            if kind[q] == CHAIN:
                assert max(ws) <= cr                                        # no chain launch holds a level above chain_rows
                assert q == 0 or kind[q - 1] == WIDE                        # no two chain launches are adjacent
            else:
                assert len(ws) == 1 and ws[0] > cr                          # a wide launch is one level above chain_rows


def test_schedule_refuses_bad_arguments(sblas):
    with pytest.raises(sblas.SblasError):
        sblas.sptrsv_schedule([3, -1, 2])
    with pytest.raises(sblas.SblasError):
        sblas.sptrsv_schedule([3], "fastest")
    with pytest.raises(sblas.SblasError):
        sblas.sptrsv_schedule([3], "auto", -1)


def test_limits(sblas):
    lim = sblas.sptrsv_limits()
    assert 1 <= lim["chain_rows"] and lim["chain_threads"] % 64 == 0 and 64 <= lim["chain_threads"] <= 1024
    assert 1 <= lim["g4_max"] < lim["g16_max"]


# ---- the numpy references against each other --------------------------------------------------------------------------
@pytest.mark.parametrize("lower,unit", [(True, False), (False, False), (True, True), (False, True)])
def test_reference_returns_the_exact_grid_solution_and_a_zero_residual(lower, unit):
    rng = np.random.default_rng(11)
    rp, ci = TN.messy(rng, 150)
    g = TN.grid_problem(rng, 150, rp, ci, lower, unit)
    x = TN.reference(150, rp, ci, g.val, g.b, lower, unit, g.alpha)
    assert np.array_equal(x, g.x)
    res, bnd = TN.residual_bound(150, rp, ci, g.val, g.b, g.x, lower, unit, g.alpha)
    assert not res.any() and np.all(bnd > 0)
    g2 = TN.grid_problem(rng, 150, rp, ci, lower, unit, nrhs=5)
    assert np.array_equal(TN.reference(150, rp, ci, g2.val, g2.b, lower, unit, g2.alpha), g2.x)


def test_reference_meets_its_own_residual_bound_and_a_perturbed_one_does_not():
    rng = np.random.default_rng(12)
    rp, ci = TN.random_lower(rng, 400)
    val = TN.dominant_values(rng, 400, rp, ci)
    b = rng.standard_normal(400)
    x = TN.reference(400, rp, ci, val, b, alpha=1.5)
    TN.check_residual(400, rp, ci, val, b, x, alpha=1.5, what="reference")
    bad = x.copy()
    bad[200] *= 1 + 1e-12
    with pytest.raises(AssertionError):
        TN.check_residual(400, rp, ci, val, b, bad, alpha=1.5, what="perturbed")
