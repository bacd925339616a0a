"""SpGEMM on the GPU (SpgemmPlan, spgemm) against the numpy restatement of the contract in tests/spgemm_numerics.py.
Every case runs three ways -- AUTO, GENERAL, and GENERAL with a chunk cap of 257 products so that several chunks occur
at small sizes -- and all three must give the reference's rowptr and colidx exactly and its values bit for bit
(spgemm_numerics.same_bits: equal bits; where the reference holds a NaN, a NaN).  Every boundary (S_max, the LDS
accumulator capacity, the narrow group's shares of both) is read from spgemm_limits().  Then the device cross-check
through coo_to_csr(dup="sum"), contract (I), the plan's behaviour and the refusals."""
import ctypes as C

import numpy as np
import pytest

import numerics as NM
import spgemm_numerics as GN

pytestmark = pytest.mark.gpu

INVALID = 1
SMALL_CAP = 257
MODES = (("auto", dict()), ("general", dict(general=True)), ("chunks", dict(general=True, chunk_cap=SMALL_CAP)))
_ref = {}


@pytest.fixture(scope="module")
def env(sblas, cuda):
    import torch
    return sblas, torch, cuda


def up(torch, cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def csr_of_rows(rows, cols_unused=None):
    """(rowptr, colidx, val) from a list of (columns, values) or of column lists (values then count 1, 2, ...)"""
    rp, ci, v = [0], [], []
    for r in rows:
        c, w = r if isinstance(r, tuple) else (r, None)
        c = list(c)
        ci += c
        v += list(w) if w is not None else [1.0 + 0.25 * ((len(v) + j) % 7) for j in range(len(c))]
        rp.append(len(ci))
    return np.array(rp, np.int32), np.array(ci, np.int32), np.array(v, np.float64)


def run_case(env, name, m, k, n, A, B, modes=MODES):
    """all modes against the reference; -> {mode: (info, rowptr, colidx, val)} as numpy"""
    S, torch, cuda = env
    if name not in _ref:
        _ref[name] = GN.reference(m, n, A[0], A[1], A[2], B[0], B[1], B[2])
    rpc, cic, vc = _ref[name]
    dA, dB = up(torch, cuda, *A), up(torch, cuda, *B)
    out = {}
    for mode, kw in modes:
        plan = S.SpgemmPlan(m, k, n, dA[0], dA[1], dB[0], dB[1], **kw)
        info = plan.info()
        rp, ci = plan.csr()
        val = plan.multiply(dA[2], dB[2])
        torch.cuda.synchronize()
        got = (info, rp.cpu().numpy().copy(), ci.cpu().numpy().copy(), val.cpu().numpy().copy())
        plan.destroy()
        assert info["nnz_c"] == len(cic), (name, mode)
        assert np.array_equal(got[1], rpc), (name, mode, "rowptr")
        assert np.array_equal(got[2], cic), (name, mode, "colidx")
        if not GN.same_bits(got[3], vc):
            bad = np.flatnonzero(GN.bits(got[3]) != GN.bits(vc))
            pytest.fail("%s / %s: %d of %d values differ from the reference, first at %d: %r vs %r"
                        % (name, mode, len(bad), len(vc), bad[0], got[3][bad[0]], vc[bad[0]]))
        assert info["rows_row"] + info["rows_general"] <= m
        if mode != "auto":
            assert info["rows_row"] == 0, (name, mode)
        out[mode] = got
    for mode in out:                                                        # and hence each other: here on plain bits
        assert np.array_equal(GN.bits(out[mode][3]), GN.bits(out[modes[0][0]][3])), (name, mode)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------------------------
def test_ash85_times_its_transpose(env, ash85):
    S, torch, cuda = env
    m, n = ash85["m"], ash85["n"]
    A = (ash85["rowptr"].astype(np.int32), ash85["colidx"].astype(np.int32), ash85["val"].astype(np.float64))
    dA = up(torch, cuda, *A)
    colptr, rowidx, valT, _ = S.csr_transpose(m, n, dA[0], dA[1], dA[2])
    torch.cuda.synchronize()
    B = (colptr.cpu().numpy(), rowidx.cpu().numpy(), valT.cpu().numpy())
    out = run_case(env, "ash85_aat", m, n, m, A, B)
    info, rp, ci, _ = out["auto"]
    assert info["b_ascending"] and info["rows_general"] == 0
    pat = GN.pattern_dense(m, m, rp, ci)
    assert np.array_equal(pat, pat.T)


def test_random_rectangular(env):
    rng = np.random.default_rng(101)
    m, k, n = 700, 450, 1900
    A = GN.random_csr(rng, m, k, 6, sort=False)
    B = GN.random_csr(rng, k, n, 9)
    out = run_case(env, "rect", m, k, n, A, B)
    assert out["chunks"][0]["chunks"] > 10


def test_empty_rows_on_both_sides(env):
    rng = np.random.default_rng(102)
    m, k, n = 300, 200, 500
    A = list(GN.random_csr(rng, m, k, 5, sort=False, empty_every=3))
    B = GN.random_csr(rng, k, n, 7, empty_every=2)                           # rows 0, 2, 4, ... of B are empty
    rp, ci, v = A
    for i in (1, 4, 7):                                                      # rows of A that name empty B rows only
        ci[rp[i]:rp[i + 1]] = 2 * (ci[rp[i]:rp[i + 1]] // 2)
    out = run_case(env, "empties", m, k, n, (rp, ci, v), B)
    rpc = out["auto"][1]
    assert rp[2] > rp[1] and rpc[2] == rpc[1]                                # work to look at, and an empty C row


@pytest.mark.parametrize("name", ["m0", "nnz_a0", "nnz_b0", "n1", "k0"])
def test_degenerate_shapes(env, name):
    rng = np.random.default_rng(103)
    z = lambda rows: (np.zeros(rows + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64))
    if name == "m0":
        m, k, n, A, B = 0, 9, 11, z(0), GN.random_csr(rng, 9, 11, 3)
    elif name == "nnz_a0":
        m, k, n, A, B = 13, 9, 11, z(13), GN.random_csr(rng, 9, 11, 3)
    elif name == "nnz_b0":
        m, k, n, A, B = 13, 9, 11, GN.random_csr(rng, 13, 9, 3), z(9)
    elif name == "k0":
        m, k, n, A, B = 5, 0, 7, z(5), z(0)
    else:
        m, k, n = 40, 30, 1
        A, B = GN.random_csr(rng, m, k, 4, sort=False), GN.random_csr(rng, k, 1, 1)
    run_case(env, name, m, k, n, A, B)


def test_every_product_of_a_row_on_one_column(env):
    A = csr_of_rows([(list(range(300)), [(-1.0) ** j * (1.0 + j / 7.0) for j in range(300)]), [0, 1]])
    B = csr_of_rows([[0]] * 300)
    out = run_case(env, "one_column", 2, 300, 3, A, B)
    assert out["auto"][0]["nnz_c"] == 2 and out["chunks"][0]["max_row_products"] == 300 > SMALL_CAP


def test_b_row_lengths_at_the_lane_chunk_edges_in_both_lane_groups(env):
    S = env[0]
    rng = np.random.default_rng(104)
    lens = [0, 1, 63, 64, 65, 129, 15, 16, 17, 33]
    n = 700
    B = csr_of_rows([np.sort(rng.choice(n, L, replace=False)) for L in lens])
    B = (B[0], B[1], rng.random(len(B[1])) * 2 - 1)
    rowsA = [[j] for j in range(len(lens))]                                   # one B row each
    rowsA += [list(range(len(lens))), list(range(len(lens)))[::-1], [5, 5, 3, 5]]
    rowsA += [[1, 6, 7, 0], [6, 1], [7, 7, 1], [1, 0, 1], [8, 1, 1, 1]] * 3      # short on average: the 16-lane form
    A = csr_of_rows(rowsA)
    widths = set()
    for i in range(len(rowsA)):
        prod = sum(lens[j] for j in rowsA[i])
        if prod:
            widths.add(S.spgemm_group_width(prod, len(rowsA[i]), n))
    assert widths == {16, 64}                                                # both forms are in this case
    run_case(env, "b_lengths", len(rowsA), len(lens), n, A, B)


def test_bitmap_word_edges_with_an_unaligned_first_column(env):
    B = csr_of_rows([[5], [5 + 31, 5 + 32, 5 + 63, 5 + 64], [7, 31, 32, 63, 64], [33, 64, 65, 95, 96, 97]])
    A = csr_of_rows([[0, 1], [1, 0], [2], [2, 0], [3, 2, 1, 0], [1], [0, 3]])
    run_case(env, "word_edges", 7, 4, 130, A, B)


# ---------------------------------------------------------------------------------------------------------------------
# capacity edges
# ---------------------------------------------------------------------------------------------------------------------
def test_span_of_exactly_s_max_and_one_more(env):
    S = env[0]
    for tag, s_max in (("wide", S.spgemm_limits()["s_max"]), ("narrow", S.spgemm_limits()["s_max"] // 4)):
        B = csr_of_rows([[3], [3 + s_max - 1], [3 + s_max], [4, 9, 3 + s_max - 2]])
        A = csr_of_rows([[0, 1, 3, 0], [0, 2, 3], [1, 2]])                    # spans s_max, s_max + 1, 2
        out = run_case(env, "span_" + tag, 3, 4, 3 + s_max + 1, A, B)
        info = out["auto"][0]
        if tag == "wide":
            assert info["rows_row"] == 2 and info["rows_general"] == 1       # the second row is too wide for the bitmap
        else:
            assert info["rows_row"] == 3 and info["rows_general"] == 0
            assert S.spgemm_group_width(4, 4, s_max) == 16 and S.spgemm_group_width(3, 3, s_max + 1) == 64


def test_c_rows_at_the_accumulator_capacity_and_beyond(env):
    S = env[0]
    cap = S.spgemm_limits()["acc_cap"]
    nb = cap // 64
    # wide: disjoint 64-entry B rows (mean 64: the 64-lane form), each named twice so that every entry is added to
    Bw = [[r * 64 + j for j in range(64)] for r in range(nb + 1)] + [[(nb + 1) * 64]]
    twice = lambda rows: rows + rows[::-1]
    Aw = [twice(list(range(nb))), twice(list(range(nb))) + [nb + 1], twice(list(range(nb + 1)))]   # cap, cap + 1, cap + 64
    out = run_case(env, "acc_wide", 3, nb + 2, (nb + 2) * 64, csr_of_rows(Aw), csr_of_rows(Bw))
    assert np.diff(out["auto"][1]).tolist() == [cap, cap + 1, cap + 64] and out["auto"][0]["rows_general"] == 0
    # narrow: 16-entry rows, a quarter of the capacity to a group
    ncap = cap // 4
    nn = ncap // 16
    Bn = [[r * 16 + j for j in range(16)] for r in range(nn + 1)] + [[(nn + 1) * 16]]
    An = [twice(list(range(nn))), twice(list(range(nn))) + [nn + 1], twice(list(range(nn + 1))), [0, 1], [nn + 1]]
    for row in An:
        assert S.spgemm_group_width(sum(len(Bn[j]) for j in row), len(row), (nn + 2) * 16) == 16
    out = run_case(env, "acc_narrow", 5, nn + 2, (nn + 2) * 16, csr_of_rows(An), csr_of_rows(Bn))
    assert np.diff(out["auto"][1]).tolist() == [ncap, ncap + 1, ncap + 16, 32, 1]


# ---------------------------------------------------------------------------------------------------------------------
# A and B as stored
# ---------------------------------------------------------------------------------------------------------------------
def test_unsorted_a_with_duplicates_stays_on_the_row_path(env):
    rng = np.random.default_rng(105)
    m, k, n = 400, 120, 900
    rp, ci, v = GN.random_csr(rng, m, k, 8, sort=False)
    ci[1::5] = ci[0:-1:5][:len(ci[1::5])]                                    # duplicates inside and across rows' ends
    B = GN.random_csr(rng, k, n, 12)
    out = run_case(env, "a_dups", m, k, n, (rp, ci, v), B)
    info = out["auto"][0]
    assert info["b_ascending"] and info["rows_general"] == 0 and info["rows_row"] > 0


@pytest.mark.parametrize("defect", ["unsorted_row", "duplicate_entry"])
def test_b_that_is_not_strictly_ascending_goes_general(env, defect):
    rng = np.random.default_rng(106)
    m, k, n = 150, 90, 400
    A = GN.random_csr(rng, m, k, 6, sort=False)
    rp, ci, v = GN.random_csr(rng, k, n, 10)
    row = int(np.flatnonzero(np.diff(rp) >= 3)[0])
    if defect == "unsorted_row":
        ci[rp[row]], ci[rp[row] + 2] = ci[rp[row] + 2], ci[rp[row]]
    else:
        ci[rp[row] + 1] = ci[rp[row]]
    out = run_case(env, "b_" + defect, m, k, n, A, (rp, ci, v))
    info = out["auto"][0]
    assert not info["b_ascending"] and info["rows_row"] == 0 and info["rows_general"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------------------------------------------------
def test_special_values_land_where_the_contract_puts_them(env):
    inf, nan = np.inf, np.nan
    tiny = 2.0 ** -1060
    B = csr_of_rows([([0, 2, 5], [1.0, -0.0, 3.0]),                          # 0
                     ([2, 5], [0.0, -3.0]),                                  # 1
                     ([1, 5, 6], [inf, 0.0, -inf]),                          # 2
                     ([1, 6], [2.0, nan]),                                   # 3
                     ([3, 4], [2.0 ** -30, tiny])])                          # 4
    A = csr_of_rows([([0], [1.0]),                                           # -0.0 alone stays -0.0
                     ([0, 1], [1.0, 1.0]),                                   # 3 + -3: a stored +0.0; -0.0 + 0.0 = +0.0
                     ([0, 0], [1.0, -1.0]),                                  # every entry cancels: structure unchanged
                     ([2, 0], [1.0, 5.0]),                                   # inf, inf * nothing; 0 * 1 + 15
                     ([2, 2], [1.0, -1.0]),                                  # inf - inf = nan, 0 - 0, -inf + inf = nan
                     ([2], [0.0]),                                           # inf * 0 = nan
                     ([3, 2], [1.0, 1.0]),                                   # nan + -inf stays nan; 2 + inf = inf
                     ([4, 4], [2.0 ** -1040, 2.0 ** -12]),                   # denormal products and sums; an underflow to 0
                     ([4], [-(2.0 ** -14)])])
    out = run_case(env, "special", 9, 5, 7, A, B)
    rp, ci, val = out["auto"][1:]
    row = lambda i: val[rp[i]:rp[i + 1]]
    assert np.signbit(row(0)[1]) and row(0)[1] == 0.0
    assert row(1).tolist()[1:] == [0.0, 0.0] and not np.signbit(row(1)[1:]).any()
    assert (row(2) == 0.0).all() and rp[3] - rp[2] == 3
    assert np.isnan(row(4)[0]) and np.isnan(row(4)[2]) and row(4)[1] == 0.0
    assert np.isnan(row(5)[0])
    assert row(6)[0] == inf and np.isnan(row(6)[2])
    assert 0.0 < abs(row(8)[1]) < 2.0 ** -1022                               # a denormal came through


# ---------------------------------------------------------------------------------------------------------------------
# contract (I)
# ---------------------------------------------------------------------------------------------------------------------
def test_a_rows_bits_do_not_depend_on_where_the_row_stands(env):
    rng = np.random.default_rng(107)
    kb, n = 12, 640
    Brows = [np.sort(rng.choice(n, L, replace=False)) for L in (70, 5, 0, 64, 130, 9, 33, 1, 65, 17, 2, 40)]
    Bvals = [(rng.random(len(r)) * 2 - 1) * 10.0 ** rng.integers(-8, 8, len(r)) for r in Brows]
    probe_cols = np.array([4, 0, 9, 4, 3, 7, 0, 2, 11], np.int32)             # unsorted, with duplicates
    probe_vals = (rng.random(len(probe_cols)) * 2 - 1) * 10.0 ** rng.integers(-8, 8, len(probe_cols))
    got = []
    for variant, (at, shift, m, k) in enumerate(((0, 0, 1, kb), (7, 3, 20, kb + 3), (18, 40, 19, kb + 50))):
        Arows = []
        for i in range(m):
            if i == at:
                Arows.append((list(probe_cols + shift), list(probe_vals)))
            else:
                L = int(rng.integers(0, 6))
                Arows.append((list(rng.integers(0, k, L)), list(rng.random(L))))
        # B's rows renumbered with A's columns; the rows around them are other rows
        Ball = [(np.sort(rng.choice(n, 7, replace=False)), rng.random(7)) for _ in range(k)]
        for j in range(kb):
            Ball[j + shift] = (Brows[j], Bvals[j])
        out = run_case(env, "indep%d" % variant, m, k, n, csr_of_rows(Arows), csr_of_rows(Ball))
        for mode in out:
            _, rp, ci, val = out[mode]
            got.append((ci[rp[at]:rp[at + 1]].copy(), GN.bits(val[rp[at]:rp[at + 1]]).copy()))
    for ci, vb in got[1:]:
        assert np.array_equal(ci, got[0][0]) and np.array_equal(vb, got[0][1])


# ---------------------------------------------------------------------------------------------------------------------
# the device cross-check
# ---------------------------------------------------------------------------------------------------------------------
def test_plan_equals_coo_to_csr_sum_of_the_expanded_triplets_on_the_device(env):
    S, torch, cuda = env
    rng = np.random.default_rng(108)
    m, k, n = 500, 300, 1200
    A = GN.random_csr(rng, m, k, 7, sort=False)
    B = GN.random_csr(rng, k, n, 11)
    row, col, val = GN.expand(m, A[0], A[1], A[2], B[0], B[1], B[2])         # products rounded once on the host: the same bits
    d = up(torch, cuda, row, col, val)
    rp, ci, v, _, _ = S.coo_to_csr(m, n, d[0], d[1], d[2], dup="sum")
    dA, dB = up(torch, cuda, *A), up(torch, cuda, *B)
    for kw in (dict(), dict(general=True, chunk_cap=SMALL_CAP)):
        plan = S.SpgemmPlan(m, k, n, dA[0], dA[1], dB[0], dB[1], **kw)
        prp, pci = plan.csr()
        pv = plan.multiply(dA[2], dB[2])
        torch.cuda.synchronize()
        assert torch.equal(prp, rp) and torch.equal(pci, ci)
        assert torch.equal(pv.view(torch.int64), v.view(torch.int64))
        plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# plan behaviour
# ---------------------------------------------------------------------------------------------------------------------
def mixed_case(S):
    """rows on the wide form, the narrow form and, through one over-wide row, the general path"""
    rng = np.random.default_rng(109)
    s_max = S.spgemm_limits()["s_max"]
    m, k, n = 260, 140, s_max + 64
    A = list(GN.random_csr(rng, m, k, 6, sort=False))
    rp, ci, v = GN.random_csr(rng, k, 800, 14)
    ci = ci.copy()
    ci[rp[3 + 1] - 1] = n - 1                                                # B's row 3 reaches the last column
    return m, k, n, tuple(A), (rp, ci, v)


def test_multiply_again_with_new_values_and_run_to_run(env):
    S, torch, cuda = env
    m, k, n, A, B = mixed_case(S)
    rng = np.random.default_rng(110)
    va2, vb2 = rng.random(len(A[2])) - 0.5, rng.random(len(B[2])) - 0.5
    dA, dB = up(torch, cuda, *A), up(torch, cuda, *B)
    dva2, dvb2 = up(torch, cuda, va2, vb2)
    plan = S.SpgemmPlan(m, k, n, dA[0], dA[1], dB[0], dB[1])
    info = plan.info()
    assert info["rows_general"] > 0 and info["rows_row"] > 0
    first = plan.multiply(dA[2], dB[2]).clone()
    second = plan.multiply(dva2, dvb2).clone()
    again = plan.multiply(dA[2], dB[2]).clone()
    fresh = S.SpgemmPlan(m, k, n, dA[0], dA[1], dB[0], dB[1])
    f1 = fresh.multiply(dA[2], dB[2]).clone()
    fresh2 = S.SpgemmPlan(m, k, n, dA[0], dA[1], dB[0], dB[1])
    f2 = fresh2.multiply(dva2, dvb2).clone()
    torch.cuda.synchronize()
    i64 = lambda t: t.view(torch.int64)
    assert torch.equal(i64(first), i64(f1)) and torch.equal(i64(second), i64(f2)) and torch.equal(i64(first), i64(again))
    assert GN.same_bits(second.cpu().numpy(), GN.reference(m, n, A[0], A[1], va2, B[0], B[1], vb2)[2])
    # the one-shot call owns its tensors
    rpc, cic, vc = S.spgemm((m, k) + tuple(dA), (k, n) + tuple(dB))
    prp, pci = plan.csr()
    assert torch.equal(rpc, prp) and torch.equal(cic, pci) and torch.equal(i64(vc), i64(first))
    assert rpc.data_ptr() != prp.data_ptr()
    for p in (plan, fresh, fresh2):
        p.destroy()


def test_numeric_replays_in_a_graph_with_changed_value_buffers(env):
    S, torch, cuda = env
    m, k, n, A, B = mixed_case(S)
    dA, dB = up(torch, cuda, *A), up(torch, cuda, *B)
    plan = S.SpgemmPlan(m, k, n, dA[0], dA[1], dB[0], dB[1], chunk_cap=SMALL_CAP)
    bufa, bufb = dA[2].clone(), dB[2].clone()
    out = torch.empty(plan.nnz_c, dtype=torch.float64, device=cuda)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            plan.multiply(bufa, bufb, out=out)
    rng = np.random.default_rng(111)
    for _ in range(2):
        na, nb = rng.random(len(A[2])) * 2 - 1, rng.random(len(B[2])) * 2 - 1
        bufa.copy_(torch.from_numpy(na)), bufb.copy_(torch.from_numpy(nb))
        out.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        replayed = out.clone()
        eager = plan.multiply(bufa, bufb)
        torch.cuda.synchronize()
        assert torch.equal(replayed.view(torch.int64), eager.view(torch.int64))
        assert GN.same_bits(replayed.cpu().numpy(), GN.reference(m, n, A[0], A[1], na, B[0], B[1], nb)[2])
    plan.destroy()


def test_csr_of_c_feeds_the_spmv_and_spmm_plans(env):
    S, torch, cuda = env
    rng = np.random.default_rng(112)
    m, k, n, N = 320, 210, 450, 8
    A = GN.random_csr(rng, m, k, 6)
    B = GN.random_csr(rng, k, n, 8)
    A = (A[0], A[1], rng.random(len(A[1])) + 0.5)
    B = (B[0], B[1], rng.random(len(B[1])) + 0.5)
    x = rng.random(n) + 0.5
    dA, dB = up(torch, cuda, *A), up(torch, cuda, *B)
    (dx,) = up(torch, cuda, x)
    plan = S.SpgemmPlan(m, k, n, dA[0], dA[1], dB[0], dB[1])
    rpc, cic = plan.csr()
    vc = plan.multiply(dA[2], dB[2])
    y = torch.zeros(m, dtype=torch.float64, device=cuda)
    sp = S.SpmvPlan(m, n, rpc, cic)
    sp(vc, dx, 1.0, 0.0, y)
    t = torch.zeros(k, dtype=torch.float64, device=cuda)
    y2 = torch.zeros(m, dtype=torch.float64, device=cuda)
    S.spmv(k, n, dB[0], dB[1], dB[2], dx, 1.0, 0.0, t)
    S.spmv(m, k, dA[0], dA[1], dA[2], t, 1.0, 0.0, y2)
    X = torch.from_numpy(np.ascontiguousarray(np.tile(x[:, None], (1, N)))).to(cuda)       # row-major n x N
    Y = torch.zeros((m, N), dtype=torch.float64, device=cuda)
    mp = S.SpmmPlan(m, n, rpc, cic, N)
    S.spmm_tensor((m, n, rpc, cic, vc), X, Y, 1.0, 0.0, plan=mp)
    torch.cuda.synchronize()
    # both routes sum the same positive terms a * b * x, each through at most la + lb + 2 roundings
    la, lb = int(np.diff(A[0]).max()), int(np.diff(B[0]).max())
    Bx = NM.row_sums(B[0], B[2] * x[B[1]])
    ABx = NM.row_sums(A[0], A[2] * Bx[A[1]])
    bound = 2.0 * NM.gamma(la + lb + 3, np.float64) * ABx
    err = np.abs(y.cpu().numpy() - y2.cpu().numpy())
    print("C x against A (B x): worst error / bound = %.3g" % float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    assert (np.abs(Y.cpu().numpy() - y2.cpu().numpy()[:, None]) <= bound[:, None]).all()
    sp.destroy(), mp.destroy(), plan.destroy()


def test_at_a_through_the_transpose_plan_has_a_symmetric_pattern(env):
    S, torch, cuda = env
    rng = np.random.default_rng(113)
    m, k = 310, 170
    A = GN.random_csr(rng, m, k, 5, sort=False)
    dA = up(torch, cuda, *A)
    tp = S.TransposePlan(m, k, dA[0], dA[1], dA[2])
    colptr, rowidx, valT = tp.csc()
    plan = S.SpgemmPlan(k, m, k, colptr, rowidx, dA[0], dA[1])                # A^T (k x m) times A (m x k): B = A is unsorted
    assert not plan.info()["b_ascending"]
    rp, ci = plan.csr()
    val = plan.multiply(valT, dA[2])
    torch.cuda.synchronize()
    rp, ci, val = rp.cpu().numpy(), ci.cpu().numpy(), val.cpu().numpy()
    pat = GN.pattern_dense(k, k, rp, ci)
    assert np.array_equal(pat, pat.T)
    At = (colptr.cpu().numpy(), rowidx.cpu().numpy(), valT.cpu().numpy())
    ref = GN.reference(k, k, At[0], At[1], At[2], A[0], A[1], A[2])
    assert np.array_equal(rp, ref[0]) and np.array_equal(ci, ref[1]) and GN.same_bits(val, ref[2])
    # and with both factors ascending, on the row path: (A^T) times (A^T)^T
    back = S.TransposePlan(k, m, colptr, rowidx, valT)
    bcp, bri, bv = back.csc()                                                # A again, rows ascending
    plan2 = S.SpgemmPlan(k, m, k, colptr, rowidx, bcp, bri)
    assert plan2.info()["b_ascending"] and plan2.info()["rows_general"] == 0
    rp2, ci2 = plan2.csr()
    torch.cuda.synchronize()
    assert np.array_equal(rp2.cpu().numpy(), rp) and np.array_equal(ci2.cpu().numpy(), ci)
    for p in (plan, plan2, tp, back):
        p.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(env):
    S, torch, cuda = env
    L = S.lib()
    rng = np.random.default_rng(114)
    m, k, n = 20, 15, 30
    A = GN.random_csr(rng, m, k, 4, sort=False)
    B = GN.random_csr(rng, k, n, 5)

    def create(A, B, m=m, k=k, n=n, null=(), flags=0, cap=0, out=True):
        d = up(torch, cuda, A[0], A[1], B[0], B[1])
        ptrs = [None if j in null else t.data_ptr() for j, t in enumerate(d)]
        h = C.c_void_p()
        rc = L.sblas_hip_spgemm_plan_create(-1, None, m, k, n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], flags, cap, C.byref(h) if out else None)
        torch.cuda.synchronize()
        assert rc == 0 or not h.value                                        # no plan is made
        if rc == 0:
            L.sblas_hip_spgemm_plan_destroy(h)
        return rc

    assert create(A, B) == 0
    bad = A[1].copy()
    bad[3] = k                                                               # a column of A >= k
    assert create((A[0], bad, A[2]), B) == INVALID
    bad = A[1].copy()
    bad[5] = -1
    assert create((A[0], bad, A[2]), B) == INVALID
    bad = B[1].copy()
    bad[-1] = n                                                              # a column of B >= n
    assert create(A, (B[0], bad, B[2])) == INVALID
    for which, M in ((0, A), (1, B)):                                        # a decreasing rowptr; one that starts above 0
        down, late = M[0].copy(), M[0].copy()
        down[1] = down[2] + 1
        late[0] = 1
        for r in (down, late):
            pair = ((r, M[1], M[2]), B) if which == 0 else (A, (r, M[1], M[2]))
            assert create(*pair) == INVALID
    for null in ((0,), (1,), (2,), (3,)):
        assert create(A, B, null=null) == INVALID
    assert create(A, B, out=False) == INVALID
    assert create(A, B, m=-1) == INVALID and create(A, B, n=1 << 31) == INVALID
    assert create(A, B, flags=2) == INVALID and create(A, B, cap=-1) == INVALID
    # numeric: the argument path
    dA, dB = up(torch, cuda, *A), up(torch, cuda, *B)
    plan = S.SpgemmPlan(m, k, n, dA[0], dA[1], dB[0], dB[1])
    out = torch.empty(plan.nnz_c, dtype=torch.float64, device=cuda)
    num = L.sblas_hip_spgemm_plan_numeric
    assert num(None, None, dA[2].data_ptr(), dB[2].data_ptr(), out.data_ptr()) == INVALID
    assert num(plan.handle, None, None, dB[2].data_ptr(), out.data_ptr()) == INVALID
    assert num(plan.handle, None, dA[2].data_ptr(), None, out.data_ptr()) == INVALID
    assert num(plan.handle, None, dA[2].data_ptr(), dB[2].data_ptr(), None) == INVALID
    assert L.sblas_hip_spgemm_plan_info(None, (C.c_int64 * 12)()) == INVALID
    assert L.sblas_hip_spgemm_plan_csr(None, None, None) == INVALID
    if torch.cuda.device_count() > 1:                                        # the wrong current device
        with torch.cuda.device(1):
            assert num(plan.handle, None, dA[2].data_ptr(), dB[2].data_ptr(), out.data_ptr()) == INVALID
    with pytest.raises(S.SblasError):
        plan.multiply(dA[2][:-1], dB[2])
    with pytest.raises(S.SblasError):
        S.SpgemmPlan(m, k, n, dA[0].cpu(), dA[1], dB[0], dB[1])
    with pytest.raises(S.SblasError):
        S.spgemm((m, k) + tuple(dA), (k + 1, n) + tuple(dB))
    assert S.spgemm_check_nnz(1 << 31) == INVALID                            # create's nnz(C) check, on the host rule
    plan.destroy()
    torch.cuda.synchronize()
