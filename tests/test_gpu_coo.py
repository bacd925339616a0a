"""CSR from COO triplets on the GPU (sblas_hip_coo_to_csr_f64_i32, the assembly plan) against a numpy restatement of the
contract written here: numpy.lexsort for the order, searchsorted for rowptr and, for dup="sum", a loop over the position
inside a run (vectorised across runs, sequential within one).  Integer arrays are compared with array_equal, values as
uint64 views: every case is bit-exact.  Then the plan against the one-shot call, determinism and graph replay, the
existing plans on the converted CSR, torch's own coalesce as a cross-check, and the refusals."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID, HIP = 1, 2
KEEP, SUM = 0, 1
_cache = {}


@pytest.fixture(scope="module")
def env(sblas, oracle, cuda):
    import torch
    return sblas, oracle, torch, cuda


def upload(torch, cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def restate(rows, cols, r, c, v, dup):
    """(rowptr, colidx, val, perm, runptr) of the contract in include/sblas_hip.h, in numpy"""
    nnz = len(r)
    order = np.lexsort((c, r))                                   # by (row, col); stable, so equal pairs keep input order
    rs, cs, vs = r[order], c[order], v[order]
    if dup == "keep":
        rowptr = np.searchsorted(rs, np.arange(rows + 1), side="left")
        return rowptr.astype(np.int32), cs.astype(np.int32), vs, order.astype(np.int32), np.arange(nnz + 1, dtype=np.int32)
    head = np.ones(nnz, bool)
    head[1:] = (rs[1:] != rs[:-1]) | (cs[1:] != cs[:-1])
    start = np.flatnonzero(head)
    runptr = np.append(start, nnz)
    lens = np.diff(runptr)
    out = vs[start].copy()                                       # a run of one is copied
    with np.errstate(all="ignore"):                              # (Inf and NaN are values like any other here)
        for j in range(1, int(lens.max()) if len(lens) else 0):
            m = lens > j
            out[m] += vs[start[m] + j]                           # ((v1 + v2) + v3) + ...: one plain add per step
    rowptr = np.searchsorted(rs[start], np.arange(rows + 1), side="left")
    return rowptr.astype(np.int32), cs[start].astype(np.int32), out, order.astype(np.int32), runptr.astype(np.int32)


def triplets_of(rows, rp, ci, v, rng):
    """the triplets of a CSR, shuffled"""
    r = np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp.astype(np.int64)))
    p = rng.permutation(len(ci))
    return r[p], ci[p].astype(np.int32), v[p]


def random_triplets(rows, cols, nnz, rng, empty_every=0):
    r = rng.integers(0, rows, nnz).astype(np.int32)
    if empty_every:
        r -= (r % empty_every == 0) & (r > 0)                    # every empty_every-th row holds nothing
    return r, rng.integers(0, cols, nnz).astype(np.int32), rng.random(nnz) * 2 - 1


def case(name):
    """(rows, cols, row, col, val) as numpy arrays"""
    if name in _cache:
        return _cache[name]
    from sblas_amd import synth
    rng = np.random.default_rng(sum(map(ord, name)))   # a seed of its own per case
    e32, e64 = np.zeros(0, np.int32), np.zeros(0)
    if name == "ash85":                    # the loader's CSR (symmetric file, expanded), shuffled
        import oracle_py
        from conftest import ASH85
        m, n, nnz, sym, rp, ci, v = oracle_py.read_mtx(ASH85)
        out = (m, n) + triplets_of(m, rp, ci, v, rng)
    elif name == "random_empty":           # duplicates by chance, every 7th row empty
        out = (3000, 2000) + random_triplets(3000, 2000, 40000, rng, empty_every=7)
    elif name == "heavy_duplicates":       # 3000 pairs, each listed 1 .. 30 times
        rows, cols = 300, 40
        br, bc = np.divmod(rng.choice(rows * cols, 3000, replace=False), cols)
        k = rng.integers(1, 31, 3000)
        r, c = np.repeat(br, k).astype(np.int32), np.repeat(bc, k).astype(np.int32)
        p = rng.permutation(len(r))
        out = (rows, cols, r[p], c[p], (rng.random(len(r)) * 2 - 1) * 10.0 ** rng.integers(-8, 8, len(r)))
    elif name == "tall":
        out = (200000, 50) + random_triplets(200000, 50, 1000000, rng)
    elif name == "wide":
        out = (50, 300000) + random_triplets(50, 300000, 20000, rng)
    elif name == "one_row":                # no row pass
        out = (1, 5000) + random_triplets(1, 5000, 20000, rng)
    elif name == "one_col":                # no column pass
        out = (5000, 1) + random_triplets(5000, 1, 20000, rng, empty_every=4)
    elif name == "one_by_one":             # no pass at all: one run of 5000 (longer than the sum kernel's LDS chunk)
        out = (1, 1, np.zeros(5000, np.int32), np.zeros(5000, np.int32), rng.random(5000) * 2 - 1)
    elif name == "cols_2_26":              # four column passes
        out = (500, 1 << 26) + random_triplets(500, 1 << 26, 4000, rng)
    elif name == "rows_2_26":              # four row passes
        out = (1 << 26, 500) + random_triplets(1 << 26, 500, 4000, rng)
    elif name == "powerlaw":               # a 10^6-entry row
        rp, ci, v = synth.powerlaw(1000000, avg=3, max_len=10 ** 6)
        out = (1000000, 1000000) + triplets_of(1000000, rp, ci, v, rng)
    elif name == "nd24k_small":
        rows, (rp, ci, v) = synth.nd24k_like(scale=0.05)
        out = (rows, rows) + triplets_of(rows, rp, ci, v, rng)
    elif name in ("sorted", "reversed"):   # already in (row, col) order / in the opposite order, duplicates included
        rows, cols, r, c, v = case("random_empty")
        o = np.lexsort((c, r))
        o = o if name == "sorted" else o[::-1]
        out = (rows, cols, np.ascontiguousarray(r[o]), np.ascontiguousarray(c[o]), np.ascontiguousarray(v[o]))
    elif name == "no_nnz":
        out = (40, 30, e32, e32, e64)
    elif name == "no_rows":
        out = (0, 30, e32, e32, e64)
    elif name == "no_cols":
        out = (40, 0, e32, e32, e64)
    elif name == "no_rows_no_cols":
        out = (0, 0, e32, e32, e64)
    elif name == "special_values":
        # (row, col) -> the run in input order.  Inf + -Inf is left out: IEEE 754 leaves the sign of a generated NaN open
        # (x86 sets it, gfx950 clears it), so its bits belong to no contract; every NaN here is an input NaN.
        inf, nan = float("inf"), float("nan")
        runs = {(0, 0): [-0.0], (0, 1): [-0.0, -0.0], (0, 2): [0.0, -0.0], (0, 3): [-0.0, 0.0],
                (1, 0): [1.5, -1.5], (1, 1): [1e16, 1.0, -1e16], (1, 2): [1.0, 1e16, -1e16], (1, 3): [0.1, 0.2, 0.3, -0.6],
                (2, 0): [inf], (2, 1): [inf, 1.0], (2, 2): [-inf, -inf], (2, 3): [1e308, 1e308],
                (3, 0): [nan], (3, 1): [1.0, nan], (3, 2): [nan, 2.0, 3.0], (3, 3): [5e-324, 5e-324],
                (5, 1): [2.0 ** -1074, -(2.0 ** -1074)], (5, 4): [3.0, -1.0, -2.0]}
        r = np.array([i for (i, j), vals in runs.items() for _ in vals], np.int32)
        c = np.array([j for (i, j), vals in runs.items() for _ in vals], np.int32)
        p = rng.permutation(len(r))          # the runs interleaved; each run's values keep the order listed above
        r, c, v = r[p], c[p], np.zeros(len(r))
        for (i, j), vals in runs.items():
            v[np.flatnonzero((r == i) & (c == j))] = vals
        out = (6, 5, r, c, v)
    else:
        raise KeyError(name)
    _cache[name] = out
    return out


# (rows_2_26 moves a 256 MiB rowptr; every other case is a few MB)
CASES = ["ash85", "random_empty", "heavy_duplicates", "tall", "wide", "one_row", "one_col", "one_by_one", "cols_2_26",
         "rows_2_26", "powerlaw", "nd24k_small", "sorted", "reversed", "no_nnz", "no_rows", "no_cols", "no_rows_no_cols",
         "special_values"]


def check_against(want, got, name, with_val=True):
    rowptr, colidx, val, perm, runptr = [None if t is None else t.cpu().numpy() for t in got]
    assert np.array_equal(rowptr, want[0]), name
    assert np.array_equal(colidx, want[1]), name
    assert np.array_equal(perm, want[3]), name
    assert np.array_equal(runptr, want[4]), name
    if with_val:
        assert val.dtype == np.float64 and np.array_equal(bits(val), bits(want[2])), name
    else:
        assert val is None


@pytest.mark.parametrize("dup", ["keep", "sum"])
@pytest.mark.parametrize("name", CASES)
def test_conversion_is_the_restatement(env, name, dup):
    S, O, torch, cuda = env
    rows, cols, r, c, v = case(name)
    want = restate(rows, cols, r, c, v, dup)
    r_d, c_d, v_d = upload(torch, cuda, r, c, v)
    check_against(want, S.coo_to_csr(rows, cols, r_d, c_d, v_d, dup=dup), name)
    check_against(want, S.coo_to_csr(rows, cols, r_d, c_d, None, dup=dup), name, with_val=False)   # structure only


def test_special_values_keep_their_meaning(env):
    """what the bit comparison above implies, spelled out: the structure never depends on the values"""
    S, O, torch, cuda = env
    rows, cols, r, c, v = case("special_values")
    r_d, c_d, v_d = upload(torch, cuda, r, c, v)
    rp, ci, val, pm, ru = [t.cpu().numpy() for t in S.coo_to_csr(rows, cols, r_d, c_d, v_d, dup="sum")]
    at = lambda i, j: val[rp[i] + list(ci[rp[i]:rp[i + 1]]).index(j)]
    assert len(ci) == 18 and list(np.diff(rp)) == [4, 4, 4, 4, 0, 2]
    assert np.signbit(at(0, 0)) and at(0, 0) == 0                  # a run of one is copied: -0.0 stays
    assert np.signbit(at(0, 1)) and not np.signbit(at(0, 2)) and not np.signbit(at(0, 3))
    assert at(1, 0) == 0.0 and at(5, 1) == 0.0 and at(5, 4) == 0.0   # cancelled: a stored zero
    assert at(1, 1) == 0.0 and at(1, 2) == 0.0                     # (1e16 + 1) - 1e16 and (1 + 1e16) - 1e16, left to right
    assert at(1, 3) == ((0.1 + 0.2) + 0.3) + -0.6
    assert at(2, 0) == np.inf and at(2, 1) == np.inf and at(2, 2) == -np.inf and at(2, 3) == np.inf
    assert np.isnan(at(3, 0)) and np.isnan(at(3, 1)) and np.isnan(at(3, 2))
    assert at(3, 3) == 1e-323                                      # subnormals are not flushed


@pytest.mark.parametrize("dup", ["keep", "sum"])
@pytest.mark.parametrize("name", ["ash85", "random_empty", "heavy_duplicates", "one_by_one", "powerlaw", "no_nnz", "no_rows_no_cols"])
def test_plan_agrees_with_the_one_shot_call(env, name, dup):
    S, O, torch, cuda = env
    rows, cols, r, c, v = case(name)
    nnz = len(r)
    r_d, c_d, v_d = upload(torch, cuda, r, c, v)
    rowptr, colidx, val, perm, runptr = S.coo_to_csr(rows, cols, r_d, c_d, v_d, dup=dup)
    plan = S.CooPlan(rows, cols, r_d, c_d, dup=dup)
    p_rowptr, p_colidx, p_perm, p_runptr = plan.csr()
    for a, b in ((rowptr, p_rowptr), (colidx, p_colidx), (perm, p_perm), (runptr, p_runptr)):
        assert torch.equal(a, b), name
    assert np.array_equal(np.sort(perm.cpu().numpy()), np.arange(nnz)), name          # a permutation
    ru = runptr.cpu().numpy().astype(np.int64)
    assert ru[0] == 0 and ru[-1] == nnz and (np.diff(ru) > 0).all(), name             # strictly increasing, ends at nnz
    got = plan.assemble(v_d)
    assert np.array_equal(bits(got.cpu().numpy()), bits(val.cpu().numpy())), name
    info = plan.info()
    bitlen = lambda n: int(n - 1).bit_length() if n > 1 else 0
    passes = (bitlen(cols) + 7) // 8 + (bitlen(rows) + 7) // 8 if nnz else 0
    want = dict(rows=rows, cols=cols, nnz=nnz, csr_nnz=len(colidx), longest_run=int(np.diff(ru).max()) if nnz else 0,
                passes=passes, dup=dup)
    assert {k: info[k] for k in want} == want, (name, info)
    assert info["bytes"] >= 4 * (rows + 1) + 12 * nnz
    plan.destroy()


def test_keep_and_sum_agree_without_duplicates(env):
    S, O, torch, cuda = env
    for name in ("ash85", "nd24k_small"):
        rows, cols, r, c, v = case(name)
        r_d, c_d, v_d = upload(torch, cuda, r, c, v)
        keep = S.coo_to_csr(rows, cols, r_d, c_d, v_d, dup="keep")
        summed = S.coo_to_csr(rows, cols, r_d, c_d, v_d, dup="sum")
        assert len(summed[1]) == len(r), name                                          # no duplicates in these inputs
        for a, b in zip(keep, summed):
            assert torch.equal(a, b), name


def test_conversion_is_deterministic_and_assemble_replays_in_a_graph(env):
    S, O, torch, cuda = env
    rows, cols, r, c, v = case("heavy_duplicates")
    r_d, c_d, v_d = upload(torch, cuda, r, c, v)
    for dup in ("keep", "sum"):
        a = S.coo_to_csr(rows, cols, r_d, c_d, v_d, dup=dup)
        b = S.coo_to_csr(rows, cols, r_d, c_d, v_d, dup=dup)
        for x, y in zip(a, b):
            assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
        plan = S.CooPlan(rows, cols, r_d, c_d, dup=dup)
        buf = v_d.clone()
        out = torch.empty(plan.csr_nnz, dtype=torch.float64, device=cuda)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                plan.assemble(buf, out=out)
        rng = np.random.default_rng(5)
        for _ in range(3):                                        # new values in the same buffer, the same graph
            nv = (rng.random(len(v)) * 2 - 1) * 10.0 ** rng.integers(-6, 6, len(v))
            buf.copy_(torch.from_numpy(nv))
            out.fill_(-7.0)
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(bits(out.cpu().numpy()), bits(restate(rows, cols, r, c, nv, dup)[2])), dup
        plan.destroy()


def test_existing_plans_run_on_the_converted_csr(env):
    """SpmvPlan, spmm and TransposePlan on the plan's CSR against the same calls on the numpy-built CSR: the arrays are the
    same, so the bits must be; and the summed CSR's SpMV against the oracle on the restatement's CSR."""
    S, O, torch, cuda = env
    N = 16
    for name in ("random_empty", "nd24k_small"):
        rows, cols, r, c, v = case(name)
        nnz = len(r)
        r_d, c_d, v_d = upload(torch, cuda, r, c, v)
        rng = np.random.default_rng(11)
        x, B = rng.random(cols), rng.random(cols * N)
        x_d, B_d = upload(torch, cuda, x, B)
        plan = S.CooPlan(rows, cols, r_d, c_d, dup="keep")
        rowptr, colidx, _, _ = plan.csr()
        val = plan.assemble(v_d)
        want = restate(rows, cols, r, c, v, "keep")
        h_rowptr, h_colidx, h_val = upload(torch, cuda, want[0], want[1], want[2])

        def products(rp, ci, vv):
            y = torch.ones(rows, dtype=torch.float64, device=cuda)
            sp = S.SpmvPlan(rows, cols, rp, ci)
            sp(vv, x_d, 2.0, 0.5, y)
            Cm = torch.ones(rows * N, dtype=torch.float64, device=cuda)
            ws = torch.empty(S.spmm_workspace_bytes(rows, cols, nnz, N) // 8 + 1, dtype=torch.float64, device=cuda)
            S.spmm(rows, cols, rp, ci, vv, B_d, cols, N, 2.0, 0.5, Cm, rows, ws)
            tp = S.TransposePlan(rows, cols, rp, ci, vv)
            yt = torch.ones(cols, dtype=torch.float64, device=cuda)
            tp.spmv(torch.ones(rows, dtype=torch.float64, device=cuda), 1.0, 0.0, yt)
            torch.cuda.synchronize()
            res = (y, Cm, yt) + tp.csc()
            sp.destroy(), tp.destroy()
            return res

        for a, b in zip(products(rowptr, colidx, val), products(h_rowptr, h_colidx, h_val)):
            assert torch.equal(a, b), name
        plan.destroy()
        # dup="sum": SpMV of the summed CSR against the oracle on the restatement's CSR
        s_rowptr, s_colidx, s_val, _, _ = S.coo_to_csr(rows, cols, r_d, c_d, v_d, dup="sum")
        ws_ = restate(rows, cols, r, c, v, "sum")
        y = torch.ones(rows, dtype=torch.float64, device=cuda)
        S.spmv(rows, cols, s_rowptr, s_colidx, s_val, x_d, 2.0, 0.5, y)
        ref = O.spmv(rows, ws_[0], ws_[1], ws_[2], x, np.ones(rows), 2.0, 0.5)
        got = y.cpu().numpy()
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print("%s: SpMV of the summed CSR, max error relative to max|y| = %.3g" % (name, err))
        assert err <= 1e-10, name


def test_torch_coalesce_cross_check(env):
    """coo_from_torch + coo_to_csr(dup="sum") against t.coalesce().to_sparse_csr().  The indices must be equal.  torch adds
    a run in an order of its own, so the values agree only within the bound of a reordered sum of len_max terms:
    |difference| <= len_max * 2^-53 * sum|v| per entry (each of the two sums is within (len - 1) * 2^-53 * sum|v| of the
    exact one, to first order; len_max counts both and the second-order terms)."""
    S, O, torch, cuda = env
    rows, cols, r, c, v = case("heavy_duplicates")
    idx = torch.from_numpy(np.stack([r, c]).astype(np.int64)).to(cuda)
    t = torch.sparse_coo_tensor(idx, torch.from_numpy(v).to(cuda), (rows, cols))
    assert not t.is_coalesced()
    rows_, cols_, r_d, c_d, v_d = S.coo_from_torch(t)
    assert (rows_, cols_) == (rows, cols) and r_d.is_cuda
    rowptr, colidx, val, perm, runptr = S.coo_to_csr(rows, cols, r_d, c_d, v_d, dup="sum")
    ref = t.coalesce().to_sparse_csr()
    assert np.array_equal(rowptr.cpu().numpy(), ref.crow_indices().cpu().numpy())
    assert np.array_equal(colidx.cpu().numpy(), ref.col_indices().cpu().numpy())
    ru = runptr.cpu().numpy().astype(np.int64)
    absum = np.add.reduceat(np.abs(v[perm.cpu().numpy()]), ru[:-1])
    bound = int(np.diff(ru).max()) * 2.0 ** -53 * absum
    diff = np.abs(val.cpu().numpy() - ref.values().cpu().numpy())
    print("torch cross-check: largest difference / bound = %.3g" % (diff / bound).max())
    assert (diff <= bound).all()


def test_refusals(env):
    S, O, torch, cuda = env
    rows, cols, r, c, v = case("ash85")
    nnz = len(r)
    L = S.lib()
    bad_row, bad_col = r.copy(), c.copy()
    bad_row[17] = rows                                   # one row index equal to rows
    bad_col[nnz - 3] = -1                                # one negative column
    r_d, c_d, v_d, br_d, bc_d = upload(torch, cuda, r, c, v, bad_row, bad_col)
    # the validator finds the bad index by reading it; no sort kernel runs on these triplets
    for rr, cc in ((br_d, c_d), (r_d, bc_d)):
        for dup in ("keep", "sum"):
            with pytest.raises(S.SblasError, match="invalid argument"):
                S.CooPlan(rows, cols, rr, cc, dup=dup)
        h = C.c_void_p()
        assert L.sblas_hip_coo_plan_create(-1, None, rows, cols, nnz, rr.data_ptr(), cc.data_ptr(), SUM, C.byref(h)) == INVALID
        assert not h.value
    import os
    os.environ["SBLAS_VALIDATE"] = "1"
    S.reload_env()
    try:
        for rr, cc in ((br_d, c_d), (r_d, bc_d)):
            with pytest.raises(S.SblasError, match="invalid argument"):
                S.coo_to_csr(rows, cols, rr, cc, v_d, dup="sum")
        check_against(restate(rows, cols, r, c, v, "sum"), S.coo_to_csr(rows, cols, r_d, c_d, v_d, dup="sum"), "validated")
    finally:
        del os.environ["SBLAS_VALIDATE"]
        S.reload_env()
    # a device index behind the last one: no plan is made there
    h = C.c_void_p()
    rc = L.sblas_hip_coo_plan_create(torch.cuda.device_count(), None, rows, cols, nnz, r_d.data_ptr(), c_d.data_ptr(), KEEP,
                                     C.byref(h))
    assert rc == HIP and not h.value
    plan = S.CooPlan(rows, cols, r_d, c_d, dup="sum")
    out = torch.empty(plan.csr_nnz, dtype=torch.float64, device=cuda)
    assert L.sblas_hip_coo_plan_assemble(plan.handle, None, None, out.data_ptr()) == INVALID
    assert L.sblas_hip_coo_plan_assemble(plan.handle, None, v_d.data_ptr(), None) == INVALID
    # assemble runs on the calling thread's current device and refuses a plan of another one; a box with one GPU has no
    # second device to stand on, so this branch runs where there are two
    if torch.cuda.device_count() > 1:
        with torch.cuda.device(1):
            assert L.sblas_hip_coo_plan_assemble(plan.handle, None, v_d.data_ptr(), out.data_ptr()) == INVALID
    with pytest.raises(S.SblasError):
        plan.assemble(v_d[:-1])
    with pytest.raises(S.SblasError):
        plan.assemble(v_d, out=out[:-1])
    assert L.sblas_hip_coo_plan_assemble(plan.handle, None, v_d.data_ptr(), out.data_ptr()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(restate(rows, cols, r, c, v, "sum")[2]))
    plan.destroy()
