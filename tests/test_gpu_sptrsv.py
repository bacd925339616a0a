"""Sparse triangular solves on the GPU (SptrsvPlan, sptrsv) against tests/sptrsv_numerics.py.

Every case runs under six schedules -- auto, per_level, chain, and auto with chain_rows = 1, one below the widest level
and the widest level itself -- which must agree bit for bit with one another (the results contract: x[i]'s bits do not
depend on the level structure, the kernel, the mode or chain_rows), and each must satisfy residual_bound(), which
carries no measured margin.  On the diagonally dominant cases (|t_ii| >= 1 + sum |t_ij|) the solution also agrees with
the double-double substitution within 1e-10 of the largest |x| (the project's fp64 parity bar; the values are
log-uniform over eight binades, so the reference neither overflows nor underflows).  Every threshold (the default
chain_rows, the boundaries of the lane-group width G(p)) is read from sptrsv_limits()."""
import ctypes as C

import numpy as np
import pytest

import amg_numerics as AN
import numerics as NM
import sptrsv_numerics as TN

pytestmark = pytest.mark.gpu

INVALID = 1
PARITY = 1e-10


@pytest.fixture(scope="module")
def env(sblas, cuda):
    import torch
    return sblas, torch, cuda


def up(torch, cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def schedules(widest):
    return [("auto", dict()), ("per_level", dict(mode="per_level")), ("chain", dict(mode="chain")),
            ("auto/1", dict(chain_rows=1)), ("auto/widest-1", dict(chain_rows=max(widest - 1, 1))),
            ("auto/widest", dict(chain_rows=max(widest, 1)))]


def solve_all(env, name, n, rp, ci, val, b, lower=True, unit=False, alpha=1.0):
    """x as numpy, after every schedule has given the same bits; also -> {schedule: info}"""
    S, torch, cuda = env
    lv, nl = TN.levels(n, rp, ci, lower)
    widest = int(TN.level_widths(lv, nl).max()) if n else 0
    drp, dci, dval, db = up(torch, cuda, rp, ci, val, b)
    first, infos = None, {}
    for label, kw in schedules(widest):
        plan = S.SptrsvPlan(n, drp, dci, lower=lower, unit_diag=unit, **kw)
        info = plan.info()
        x = torch.full_like(db, -7.0)
        out = plan.solve(dval, db, x=x, alpha=alpha)
        torch.cuda.synchronize()
        assert out is x
        got = x.cpu().numpy()
        assert info["levels"] == nl and info["widest_level"] == widest, (name, label, info)
        assert info["launches"] == info["wide_launches"] + info["chain_launches"]
        if label == "per_level":
            assert info["wide_launches"] == nl and info["chain_launches"] == 0
        if label == "chain":
            assert info["wide_launches"] == 0 and info["chain_launches"] == (1 if n else 0)
        if label == "auto/widest" and n:
            assert info["wide_launches"] == 0 and info["chain_launches"] == 1   # nothing is above the widest level
        if label == "auto/widest-1" and widest > 1:
            assert info["wide_launches"] >= 1
        perm, lp = plan.levels()
        if label == "auto" and n:
            want = np.lexsort((np.arange(n), lv))                           # by (level, row)
            assert np.array_equal(perm.cpu().numpy(), want), name
            assert np.array_equal(lp.cpu().numpy(), np.concatenate([[0], np.cumsum(TN.level_widths(lv, nl))])), name
        plan.destroy()
        infos[label] = info
        if first is None:
            first = got
        else:
            same = TN.bits(got) == TN.bits(first)
            assert same.all(), "%s: %s differs from auto in %d of %d entries, first at %s: %r vs %r" % (
                name, label, (~same).sum(), same.size, np.argwhere(~same)[0].tolist(), got[~same][0], first[~same][0])
    return first, infos


def run_case(env, name, n, rp, ci, lower=True, unit=False, alpha=1.0, seed=0, parity=True):
    """dominant values on the pattern: all schedules, the residual bound, the reference"""
    rng = np.random.default_rng(seed)
    val = TN.dominant_values(rng, n, rp, ci, lower, unit)
    b = NM.log_uniform(rng, n, 8)
    x, infos = solve_all(env, name, n, rp, ci, val, b, lower, unit, alpha)
    TN.check_residual(n, rp, ci, val, b, x, lower, unit, alpha, what=name)
    if parity:
        ref = TN.reference(n, rp, ci, val, b, lower, unit, alpha)
        err = np.abs(x - ref).max() / np.abs(ref).max()
        print("%s: max|x - ref| / max|ref| = %.3g" % (name, err))
        assert err <= PARITY, (name, err)
    return x, infos, val, b


# ---------------------------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lower", [True, False])
def test_ash85(env, ash85, lower):
    n = ash85["m"]
    rp, ci = TN.triangle_of(n, ash85["rowptr"], ash85["colidx"], lower)
    run_case(env, "ash85 %s" % ("lower" if lower else "upper"), n, rp, ci, lower, alpha=-1.25, seed=1)


@pytest.mark.parametrize("lower", [True, False])
def test_grid_48(env, lower):
    side = 48
    rp, ci = TN.grid5(side, lower)
    x, infos, _, _ = run_case(env, "grid48 %s" % ("lower" if lower else "upper"), side * side, rp, ci, lower, seed=2)
    assert infos["auto"]["levels"] == 95
    for w in (1, 7, 24, 47):                                                # chain -> wide -> chain around every threshold
        S, torch, cuda = env
        plan = S.SptrsvPlan(side * side, *up(torch, cuda, rp, ci), lower=lower, chain_rows=w)
        info = plan.info()
        plan.destroy()
        assert info["chain_launches"] == 2 and info["wide_launches"] == 95 - 2 * w, (w, info)


def test_bidiagonal_chain_of_3000_rows(env):
    rp, ci = TN.bidiagonal(3000)
    x, infos, _, _ = run_case(env, "bidiagonal", 3000, rp, ci, seed=3)
    assert infos["auto"]["levels"] == 3000 and infos["auto"]["launches"] == 1


def test_diagonal_matrix(env):
    rp, ci = TN.diagonal(5000)
    x, infos, val, b = run_case(env, "diagonal", 5000, rp, ci, alpha=0.75, seed=4)
    assert infos["auto"]["levels"] == 1
    assert np.array_equal(x, (0.75 * b) / val)                              # nothing to sum: the last expression alone


def test_arrow_with_a_row_of_19999_entries(env):
    n = 20000
    rp, ci = TN.arrow(n)
    x, infos, _, _ = run_case(env, "arrow", n, rp, ci, seed=5)
    assert infos["auto"]["levels"] == 3 and infos["auto"]["longest_row"] == n
    rp2, ci2 = TN.csr_of_rows([[0]] + [[0, i] for i in range(1, n)])       # the dense first column alone: two levels
    x, infos, _, _ = run_case(env, "first column", n, rp2, ci2, seed=6)
    assert infos["auto"]["levels"] == 2 and infos["auto"]["widest_level"] == n - 1


def test_random_lower_4000(env):
    rng = np.random.default_rng(7)
    rp, ci = TN.random_lower(rng, 4000)
    lv, nl = TN.levels(4000, rp, ci)
    w = TN.level_widths(lv, nl)
    print("random lower: %d levels, widths %d .. %d" % (nl, w.min(), w.max()))
    assert nl == 42 and w.min() == 1 and w.max() == 370
    x, infos, _, _ = run_case(env, "random lower", 4000, rp, ci, seed=7)
    cr = sblas_default_chain_rows(env)
    assert infos["auto"]["wide_launches"] == int((w > cr).sum())
    assert infos["auto/1"]["wide_launches"] == int((w > 1).sum()) and infos["auto/1"]["chain_launches"] >= 1


def sblas_default_chain_rows(env):
    return env[0].sptrsv_limits()["chain_rows"]


def test_levels_around_the_default_chain_rows(env):
    cr = sblas_default_chain_rows(env)
    widths = [cr - 1, cr, cr + 1, cr - 1, cr + 1, cr + 1, cr]
    rp, ci = TN.staircase(widths)
    x, infos, _, _ = run_case(env, "staircase", sum(widths), rp, ci, seed=8)
    a = infos["auto"]
    assert a["levels"] == 7 and a["wide_launches"] == 3 and a["chain_launches"] == 3, a


def test_rows_around_every_group_width_boundary(env):
    lim = env[0].sptrsv_limits()
    g4, g16 = lim["g4_max"], lim["g16_max"]
    lengths = sorted({1, 2, g4 - 1, g4, g4 + 1, g4 + 2, 15, 16, 17, g16 - 1, g16, g16 + 1, g16 + 2, 63, 64, 65, 66, 127, 128, 129, 130, 200})
    rp, ci = TN.row_lengths_case(lengths)
    n = len(rp) - 1
    run_case(env, "group widths", n, rp, ci, seed=9)
    # the same rows as an upper triangle of the reversed matrix, unsorted
    rng = np.random.default_rng(10)
    rows = [list(rng.permutation(n - 1 - ci[rp[i]:rp[i + 1]])) for i in range(n - 1, -1, -1)]
    rp2, ci2 = TN.csr_of_rows(rows)
    run_case(env, "group widths, upper", n, rp2, ci2, lower=False, seed=11)


@pytest.mark.parametrize("lower,unit", [(True, False), (False, False), (True, True), (False, True)])
def test_bits_against_the_lane_order_restatement(env, lower, unit):
    """SpSV's bits against the host restatement of its contract (TN.solve_lane_order), not against another schedule: 80
    unsorted rows with entries in both triangles whose stored lengths are both sides of each G(p) boundary and 70 (two
    rounds per lane of a whole wave).  Every ignored entry is NaN -- the other triangle and, under unit, the stored
    diagonal -- so one that is multiplied by zero instead of skipped shows; alpha is not 1.  Equality of bits: no
    tolerance."""
    S, torch, cuda = env
    lim = S.sptrsv_limits()
    g4, g16 = lim["g4_max"], lim["g16_max"]
    lengths = [1, g4, g4 + 1, g16, g16 + 1, 70]
    assert (g4, g16) == (AN.G4_MAX, AN.G16_MAX) and 64 < lengths[-1] <= 80
    n, alpha = 80, 0.3
    rng = np.random.default_rng(41 + 2 * lower + unit)
    rows = []
    for i in range(n):
        others = rng.choice(np.delete(np.arange(n), i), lengths[i % len(lengths)] - 1, replace=False)
        rows.append(list(rng.permutation(np.concatenate([others, [i]]))))   # stored order: the triangles interleaved
    rp, ci = TN.csr_of_rows(rows)
    val = TN.dominant_values(rng, n, rp, ci, lower, unit)
    ignored = TN.selected(rp, ci, not lower)
    assert ignored.any() and TN.selected(rp, ci, lower).any()
    val[ignored] = np.nan
    if unit:
        val[TN.on_diagonal(rp, ci)] = np.nan                                # ignored too: the diagonal is 1
    b = NM.log_uniform(rng, n, 8)
    want = TN.solve_lane_order(n, rp, ci, val, b, lower, unit, alpha)
    assert np.isfinite(want).all()
    drp, dci, dval, db = up(torch, cuda, rp, ci, val, b)
    for mode, chain_rows in (("per_level", 0), ("chain", 0), ("auto", 8)):    # some twenty levels, up to some twenty rows wide
        plan = S.SptrsvPlan(n, drp, dci, lower=lower, unit_diag=unit, mode=mode, chain_rows=chain_rows)
        info = plan.info()
        assert mode != "auto" or (info["wide_launches"] >= 1 and info["chain_launches"] >= 1), info
        got = plan.solve(dval, db, alpha=alpha).cpu().numpy()
        plan.destroy()
        same = TN.bits(got) == TN.bits(want)
        assert same.all(), "%s: %d of %d entries differ from the restatement, first at row %d (stored length %d): %r vs %r" % (
            mode, (~same).sum(), n, np.argmax(~same), rp[np.argmax(~same) + 1] - rp[np.argmax(~same)], got[np.argmax(~same)], want[np.argmax(~same)])


def test_unsorted_rows_with_duplicates(env):
    rng = np.random.default_rng(12)
    rp, ci = TN.messy(rng, 700)
    run_case(env, "messy lower", 700, rp, ci, True, seed=13)
    run_case(env, "messy upper", 700, rp, ci, False, seed=14)


def test_a_full_matrix_as_lower_and_as_upper(env, ash85):
    n = ash85["m"]
    rp0, ci0 = np.asarray(ash85["rowptr"], np.int64), np.asarray(ash85["colidx"], np.int64)
    rows = [sorted(set(ci0[rp0[i]:rp0[i + 1]].tolist()) | {i}) for i in range(n)]  # both triangles and a diagonal
    rp, ci = TN.csr_of_rows(rows)
    assert TN.selected(rp, ci, True).any() and TN.selected(rp, ci, False).any()
    run_case(env, "full as lower", n, rp, ci, True, seed=15)
    run_case(env, "full as upper", n, rp, ci, False, seed=16)


def test_a_combined_unit_l_and_u_factor_by_two_plans(env):
    """L (unit lower, its diagonal not stored) and U (upper, with the diagonal) in one CSR, as ILU(0) leaves them:
    y = L^-1 b then x = U^-1 y, on the same arrays."""
    S, torch, cuda = env
    rng = np.random.default_rng(17)
    side = 20
    n = side * side
    lo, up_ = TN.grid5(side, True), TN.grid5(side, False)
    rows = [[c for c in lo[1][lo[0][i]:lo[0][i + 1]] if c != i] + list(up_[1][up_[0][i]:up_[0][i + 1]]) for i in range(n)]
    rp, ci = TN.csr_of_rows(rows)
    val = TN.dominant_values(rng, n, rp, ci, lower=False)                   # U dominant, its diagonal set
    sel_l = TN.selected(rp, ci, True)
    val[sel_l] = NM.log_uniform(rng, int(sel_l.sum()), 4, center=-3)        # L's multipliers: small
    b = NM.log_uniform(rng, n, 8)
    y, _ = solve_all(env, "LU: L", n, rp, ci, val, b, lower=True, unit=True)
    TN.check_residual(n, rp, ci, val, b, y, True, True, what="LU: L")
    x, _ = solve_all(env, "LU: U", n, rp, ci, val, y, lower=False, unit=False)
    TN.check_residual(n, rp, ci, val, y, x, False, False, what="LU: U")
    yr = TN.reference(n, rp, ci, val, b, True, True)
    xr = TN.reference(n, rp, ci, val, yr, False, False)
    assert np.abs(y - yr).max() <= PARITY * np.abs(yr).max()
    assert np.abs(x - xr).max() <= PARITY * np.abs(xr).max()


def test_n_0_and_n_1(env):
    S, torch, cuda = env
    x, infos = solve_all(env, "n = 0", 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0), np.zeros(0))
    assert x.size == 0 and infos["auto"]["launches"] == 0
    x, _ = solve_all(env, "n = 1", 1, np.array([0, 1], np.int32), np.array([0], np.int32), np.array([4.0]), np.array([3.0]), alpha=2.0)
    assert x.tolist() == [1.5]
    x, _ = solve_all(env, "n = 1 unit", 1, np.array([0, 0], np.int32), np.zeros(0, np.int32), np.zeros(0), np.array([3.0]), unit=True)
    assert x.tolist() == [3.0]
    X = S.SptrsvPlan(0, *up(torch, cuda, np.zeros(1, np.int32), np.zeros(0, np.int32))).solve(
        torch.zeros(0, dtype=torch.float64, device=cuda), torch.zeros((0, 3), dtype=torch.float64, device=cuda))
    assert tuple(X.shape) == (0, 3)


def test_an_empty_block_of_right_hand_sides_with_numpys_strides(env):
    """found by tools/fuzz_plans.py (ilu0, a matrix without rows): a 0 x 3 array from numpy reaches torch with the strides
    (0, 0), contiguous as torch sees it; solve() read stride(1) != 1 as "not row-major" and refused it"""
    S, torch, cuda = env
    plan = S.SptrsvPlan(0, *up(torch, cuda, np.zeros(1, np.int32), np.zeros(0, np.int32)))
    val = torch.zeros(0, dtype=torch.float64, device=cuda)
    B = torch.zeros(0, dtype=torch.float64, device=cuda).as_strided((0, 3), (0, 0))
    assert B.is_contiguous() and B.stride() == (0, 0)
    X = plan.solve(val, B)
    assert tuple(X.shape) == (0, 3)
    assert plan.solve(val, B, x=B) is B
    plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# exact grid
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lower,unit", [(True, False), (False, False), (True, True), (False, True)])
def test_exact_grid_returns_x_itself(env, lower, unit):
    rng = np.random.default_rng(20)
    lim = env[0].sptrsv_limits()
    base_rp, base_ci = TN.row_lengths_case([2, lim["g4_max"] + 1, lim["g16_max"], lim["g16_max"] + 1, 65, 130, 300])
    n0 = len(base_rp) - 1
    mrp, mci = TN.messy(rng, n0)                                             # both triangles, duplicates, unsorted
    rows = [list(base_ci[base_rp[i]:base_rp[i + 1]]) + [c for c in mci[mrp[i]:mrp[i + 1]] if c != i] for i in range(n0)]
    if not lower:
        rows = [[n0 - 1 - c for c in r] for r in rows[::-1]]
    rp, ci = TN.csr_of_rows(rows)
    g = TN.grid_problem(rng, n0, rp, ci, lower, unit)
    x, _ = solve_all(env, "exact grid", n0, rp, ci, g.val, g.b, lower, unit, g.alpha)
    assert np.array_equal(x, g.x)
    S, torch, cuda = env
    g2 = TN.grid_problem(rng, n0, rp, ci, lower, unit, nrhs=5)              # and through the SpSM kernels
    drp, dci, dval, dB = up(torch, cuda, rp, ci, g2.val, g2.b)
    for kw in (dict(), dict(mode="per_level"), dict(mode="chain")):
        X = S.SptrsvPlan(n0, drp, dci, lower=lower, unit_diag=unit, **kw).solve(dval, dB, alpha=g2.alpha)
        assert np.array_equal(X.cpu().numpy(), g2.x), kw


# ---------------------------------------------------------------------------------------------------------------------
# SpSM
# ---------------------------------------------------------------------------------------------------------------------
def test_spsm_columns_do_not_depend_on_nrhs_mode_or_padding(env):
    S, torch, cuda = env
    rng = np.random.default_rng(21)
    n = 1500
    rp, ci = TN.random_lower(rng, n)
    val = TN.dominant_values(rng, n, rp, ci)
    widest = int(TN.level_widths(*TN.levels(n, rp, ci)).max())
    B = NM.log_uniform(rng, (n, 130), 8)
    drp, dci, dval = up(torch, cuda, rp, ci, val)
    alpha = 1.75
    plans = {label: S.SptrsvPlan(n, drp, dci, **kw) for label, kw in schedules(widest)[:4]}
    full = None
    for nrhs in (130, 1, 3, 64, 65):
        for label, plan in plans.items():
            for pad_b, pad_x in ((3, 5), (0, 0)):
                if (pad_b, pad_x) == (0, 0) and label != "auto":
                    continue
                Bbuf = torch.full((n, nrhs + pad_b), np.nan, dtype=torch.float64, device=cuda)
                Bbuf[:, :nrhs] = torch.from_numpy(B[:, :nrhs]).to(cuda)
                Xbuf = torch.full((n, nrhs + pad_x), -7.0, dtype=torch.float64, device=cuda)
                out = plan.solve(dval, Bbuf[:, :nrhs], x=Xbuf[:, :nrhs], alpha=alpha)
                torch.cuda.synchronize()
                assert out.data_ptr() == Xbuf.data_ptr()
                got = Xbuf.cpu().numpy()
                assert np.all(got[:, nrhs:] == -7.0), "the padding of X was written"
                if full is None:
                    full = got[:, :nrhs].copy()
                    TN.check_residual(n, rp, ci, val, B, full, alpha=alpha, what="SpSM 130")
                    ref = TN.reference(n, rp, ci, val, B, alpha=alpha)
                    assert np.abs(full - ref).max() <= PARITY * np.abs(ref).max()
                assert np.array_equal(TN.bits(got[:, :nrhs]), TN.bits(full[:, :nrhs])), (nrhs, label, pad_b)
    # nrhs = 0 is a no-op
    empty = plans["auto"].solve(dval, torch.empty((n, 0), dtype=torch.float64, device=cuda))
    assert tuple(empty.shape) == (n, 0)
    for plan in plans.values():
        plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# the plan's behaviour
# ---------------------------------------------------------------------------------------------------------------------
def small_case(seed=30, n=900):
    rng = np.random.default_rng(seed)
    rp, ci = TN.random_lower(rng, n)
    return rng, n, rp, ci, TN.dominant_values(rng, n, rp, ci), NM.log_uniform(rng, n, 8)


def test_in_place_equals_out_of_place(env):
    S, torch, cuda = env
    rng, n, rp, ci, val, b = small_case()
    drp, dci, dval, db = up(torch, cuda, rp, ci, val, b)
    B = NM.log_uniform(rng, (n, 7), 8)
    for kw in (dict(), dict(mode="per_level"), dict(mode="chain")):
        plan = S.SptrsvPlan(n, drp, dci, **kw)
        x = plan.solve(dval, db, alpha=0.5)
        xb = db.clone()
        assert plan.solve(dval, xb, x=xb, alpha=0.5) is xb
        assert torch.equal(xb.view(torch.int64), x.view(torch.int64))
        dB = torch.from_numpy(B).to(cuda)
        X = plan.solve(dval, dB)
        XB = dB.clone()
        plan.solve(dval, XB, x=XB)
        assert torch.equal(XB.view(torch.int64), X.view(torch.int64))
        plan.destroy()


def test_new_values_on_the_same_plan_and_the_one_shot(env):
    S, torch, cuda = env
    rng, n, rp, ci, val, b = small_case(31)
    drp, dci, dval, db = up(torch, cuda, rp, ci, val, b)
    plan = S.SptrsvPlan(n, drp, dci)
    first = plan.solve(dval, db).cpu().numpy()
    val2 = TN.dominant_values(rng, n, rp, ci)
    second = plan.solve(torch.from_numpy(val2).to(cuda), db).cpu().numpy()
    again = plan.solve(dval, db).cpu().numpy()
    plan.destroy()
    assert np.array_equal(TN.bits(first), TN.bits(again)) and not np.array_equal(first, second)
    TN.check_residual(n, rp, ci, val2, b, second, what="new values")
    one = S.sptrsv((n, drp, dci, dval), db).cpu().numpy()
    assert np.array_equal(TN.bits(one), TN.bits(first))
    # the one shot on an upper triangle and several right-hand sides: the matrix turned upside down
    up_rp, up_ci = TN.csr_of_rows([list(n - 1 - ci[rp[i]:rp[i + 1]]) for i in range(n - 1, -1, -1)])
    up_val = TN.dominant_values(rng, n, up_rp, up_ci, lower=False)
    B = NM.log_uniform(rng, (n, 3), 8)
    X = S.sptrsv((n,) + tuple(up(torch, cuda, up_rp, up_ci, up_val)), torch.from_numpy(B).to(cuda), lower=False, alpha=2.0)
    TN.check_residual(n, up_rp, up_ci, up_val, B, X.cpu().numpy(), lower=False, alpha=2.0, what="one shot, upper")


def test_solve_replays_in_a_graph_after_val_and_b_are_overwritten(env):
    S, torch, cuda = env
    rng, n, rp, ci, val, b = small_case(32, n=1200)
    drp, dci, dval, db = up(torch, cuda, rp, ci, val, b)
    plan = S.SptrsvPlan(n, drp, dci, chain_rows=32)                         # both kinds of launch in the graph
    assert plan.info()["wide_launches"] >= 1 and plan.info()["chain_launches"] >= 2
    x = torch.empty(n, dtype=torch.float64, device=cuda)
    dB = torch.from_numpy(NM.log_uniform(rng, (n, 5), 8)).to(cuda)
    X = torch.empty_like(dB)
    plan.solve(dval, db, x=x)                                               # warm: the code objects are loaded
    plan.solve(dval, dB, x=X)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            plan.solve(dval, db, x=x, alpha=1.5)
            plan.solve(dval, dB, x=X, alpha=1.5)
    for _ in range(2):
        dval.copy_(torch.from_numpy(TN.dominant_values(rng, n, rp, ci)))
        db.copy_(torch.from_numpy(NM.log_uniform(rng, n, 8)))
        dB.copy_(torch.from_numpy(NM.log_uniform(rng, (n, 5), 8)))
        x.fill_(-7.0), X.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        rx, rX = x.clone(), X.clone()
        ex, eX = plan.solve(dval, db, alpha=1.5), plan.solve(dval, dB, alpha=1.5)
        torch.cuda.synchronize()
        assert torch.equal(rx.view(torch.int64), ex.view(torch.int64))
        assert torch.equal(rX.view(torch.int64), eX.view(torch.int64))
        TN.check_residual(n, rp, ci, dval.cpu().numpy(), db.cpu().numpy(), rx.cpu().numpy(), alpha=1.5, what="replay")
    plan.destroy()


def test_transposed_solve_through_the_transpose_plan(env):
    S, torch, cuda = env
    rng, n, rp, ci, val, b = small_case(33)
    # dominant by columns too: scale every column's off-diagonals below the diagonal's margin
    dg = TN.on_diagonal(rp, ci)
    val[~dg] *= 2.0 ** -8
    drp, dci, dval, db = up(torch, cuda, rp, ci, val, b)
    tp = S.TransposePlan(n, n, drp, dci, dval)
    colptr, rowidx, valT = tp.csc()                                         # T^T as CSR: an upper triangle
    plan = S.SptrsvPlan(n, colptr, rowidx, lower=False)
    x = plan.solve(valT, db, alpha=-2.0).cpu().numpy()
    plan.destroy(), tp.destroy()
    cp, ri, perm = NM.csc_of(n, n, rp, ci)
    TN.check_residual(n, cp, ri, val[perm], b, x, lower=False, alpha=-2.0, what="transposed")
    ref = TN.reference(n, cp, ri, val[perm], b, lower=False, alpha=-2.0)
    assert np.abs(x - ref).max() <= PARITY * np.abs(ref).max()
    # and it is the transposed system that was solved: T^T x = alpha b, checked through T's own rows
    dense = np.zeros((n, n))
    np.add.at(dense, (NM.row_of_entries(rp), ci), val)
    assert np.abs(dense.T @ x + 2.0 * b).max() <= 1e-9 * np.abs(b).max()


def test_a_zero_pivot_spreads_inf_and_nan_to_its_dependants_only(env):
    S, torch, cuda = env
    rng, n, rp, ci, val, b = small_case(34)
    def reached_from(r):
        reach = np.zeros(n, bool)
        reach[r] = True
        for i in range(r + 1, n):                                           # rows ascend: one pass closes the set
            c = ci[rp[i]:rp[i + 1]]
            reach[i] = reach[c[c < i]].any()
        return reach

    for r in range(n // 4, n):                                              # a pivot with some dependants, and many rows without
        reach = reached_from(r)
        if reach.sum() > 20:
            break
    assert reach.sum() > 20 and (~reach).sum() > n // 4
    clean, _ = solve_all(env, "before the zero", n, rp, ci, val, b)
    val0 = val.copy()
    val0[rp[r]:rp[r + 1]][ci[rp[r]:rp[r + 1]] == r] = 0.0
    assert val0[rp[r + 1] - 1] == 0.0                                       # random_lower stores the diagonal last
    x, _ = solve_all_nonfinite(env, n, rp, ci, val0, b)
    assert not np.isfinite(x[reach]).any()
    assert np.array_equal(TN.bits(x[~reach]), TN.bits(clean[~reach]))


def solve_all_nonfinite(env, n, rp, ci, val, b):
    """solve_all, with NaNs compared as NaNs (which NaN a sum holds is the adder's choice)"""
    S, torch, cuda = env
    widest = int(TN.level_widths(*TN.levels(n, rp, ci)).max())
    drp, dci, dval, db = up(torch, cuda, rp, ci, val, b)
    first = None
    for label, kw in schedules(widest):
        plan = S.SptrsvPlan(n, drp, dci, **kw)
        got = plan.solve(dval, db).cpu().numpy()                            # no error code: the solve returns
        plan.destroy()
        if first is None:
            first = got
        nan = np.isnan(first)
        assert np.array_equal(np.isnan(got), nan), label
        assert np.array_equal(TN.bits(got[~nan]), TN.bits(first[~nan])), label
    return first, None


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_create_refuses_a_bad_structure_and_names_the_row(env):
    S, torch, cuda = env
    rp, ci = TN.csr_of_rows([[0], [0, 1], [1], [3, 0], [0]])               # rows 2 and 4 lack a diagonal
    drp, dci = up(torch, cuda, rp, ci)
    with pytest.raises(S.SblasError) as e:
        S.SptrsvPlan(5, drp, dci)
    assert e.value.bad_row == 2 and "row 2" in str(e.value) and "code %d" % INVALID in str(e.value)
    S.SptrsvPlan(5, drp, dci, unit_diag=True).destroy()
    rp, ci = TN.csr_of_rows([[0], [1, 0, 1], [2]])
    with pytest.raises(S.SblasError) as e:
        S.SptrsvPlan(3, *up(torch, cuda, rp, ci))
    assert e.value.bad_row == 1
    rp, ci = TN.csr_of_rows([[0], [1], [2, 3]])
    with pytest.raises(S.SblasError) as e:
        S.SptrsvPlan(3, *up(torch, cuda, rp, ci), unit_diag=True)
    assert e.value.bad_row == 2
    with pytest.raises(S.SblasError) as e:
        S.SptrsvPlan(3, *up(torch, cuda, np.array([0, 2, 1, 3], np.int32), np.array([0, 1, 2], np.int32)))
    assert e.value.bad_row == 1
    with pytest.raises(S.SblasError) as e:                                  # rowptr ends short of nnz
        S.SptrsvPlan(3, *up(torch, cuda, np.array([0, 1, 2, 3], np.int32), np.array([0, 1, 2, 2], np.int32)))
    assert e.value.bad_row == 2
    with pytest.raises(S.SblasError):
        S.SptrsvPlan(3, *up(torch, cuda, np.array([0, 1, 2, 3], np.int32), np.array([0, 1, 2], np.int32)), mode="fastest")


def test_calls_are_refused_before_anything_is_launched(env):
    S, torch, cuda = env
    rng, n, rp, ci, val, b = small_case(35, n=300)
    drp, dci, dval, db = up(torch, cuda, rp, ci, val, b)
    plan = S.SptrsvPlan(n, drp, dci)
    x = torch.full((n,), -7.0, dtype=torch.float64, device=cuda)
    L = S.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    other_rp, other_ci = drp.clone(), dci.clone()                            # the same structure at other addresses
    for prp, pci in ((other_rp, dci), (drp, other_ci)):
        rc = L.sblas_hip_sptrsv_f64_i32_planned(plan.handle, stream, prp.data_ptr(), pci.data_ptr(), dval.data_ptr(), 1.0,
                                                db.data_ptr(), x.data_ptr())
        assert rc == INVALID
        rc = L.sblas_hip_sptrsm_f64_i32_planned(plan.handle, stream, prp.data_ptr(), pci.data_ptr(), dval.data_ptr(), 1, 1.0,
                                                db.data_ptr(), 1, x.data_ptr(), 1)
        assert rc == INVALID
    rc = L.sblas_hip_sptrsm_f64_i32_planned(plan.handle, stream, drp.data_ptr(), dci.data_ptr(), dval.data_ptr(), 4, 1.0,
                                            db.data_ptr(), 3, x.data_ptr(), 4)  # ldb below nrhs
    assert rc == INVALID
    assert L.sblas_hip_sptrsv_f64_i32_planned(None, stream, drp.data_ptr(), dci.data_ptr(), dval.data_ptr(), 1.0, db.data_ptr(),
                                              x.data_ptr()) == INVALID
    bad = [lambda: plan.solve(dval.cpu(), db), lambda: plan.solve(dval, db.cpu()), lambda: plan.solve(dval, db, x=x.cpu()),
           lambda: plan.solve(dval.float(), db), lambda: plan.solve(dval, db.float()),
           lambda: plan.solve(dval[:-1], db), lambda: plan.solve(dval, db[:-1]), lambda: plan.solve(dval, db, x=x[:-1]),
           lambda: plan.solve(dval, db[::2]),
           lambda: plan.solve(dval, torch.zeros((4, n), dtype=torch.float64, device=cuda).t()),   # column-major
           lambda: S.SptrsvPlan(n, drp.cpu(), dci), lambda: S.SptrsvPlan(n, drp, dci.cpu()),
           lambda: S.SptrsvPlan(n, drp.long(), dci), lambda: S.SptrsvPlan(n, drp, dci.long()),
           lambda: S.SptrsvPlan(n + 1, drp, dci), lambda: S.SptrsvPlan(n, drp, dci[:-1])]
    for k, call in enumerate(bad):
        with pytest.raises(S.SblasError):
            call()
            pytest.fail("call %d was accepted" % k)
    torch.cuda.synchronize()
    assert bool((x == -7.0).all())                                          # nothing ran
    plan.destroy()
