"""Transposed products on the GPU: the device CSR -> CSC transpose against numpy's stable argsort (every radix pass count,
empty rows / columns / matrices, duplicates, a 10^6-entry row and column), determinism and graph capture, and the
transpose plan's A^T x / A^T B against the oracle and bit for bit against the existing plans on the host-built CSC."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COL, ROW = 0, 1
INVALID = 1
_cache = {}


@pytest.fixture(scope="module")
def env(sblas, oracle, cuda):
    import torch
    return sblas, oracle, torch, cuda


def upload(torch, cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def host_csc(rows, cols, rp, ci, v):
    """(colptr, rowidx, valT, perm): column c in CSR order, the stable argsort of the column indices"""
    perm = np.argsort(ci, kind="stable").astype(np.int32)
    row_of = np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp.astype(np.int64)))
    colptr = np.zeros(cols + 1, np.int64)
    np.cumsum(np.bincount(ci, minlength=cols), out=colptr[1:])
    return colptr.astype(np.int32), row_of[perm], v[perm], perm


def host_transpose_csr(rows, cols, rp, ci, v):
    """A^T as (rows', cols', rowptr, colidx, val)"""
    cp, ri, vt, _ = host_csc(rows, cols, rp, ci, v)
    return cols, rows, cp, ri, vt


def matrix(name):
    if name in _cache:
        return _cache[name]
    from sblas_amd import synth
    if name == "ash85":
        import oracle_py
        from conftest import ASH85
        m, n, nnz, sym, rp, ci, v = oracle_py.read_mtx(ASH85)
        out = (m, n, rp, ci, v)
    elif name == "random_empty":          # unsorted rows, duplicates, every 7th row empty
        out = (3000, 2000) + synth.random_csr(3000, 2000, 12, empty_every=7)
    elif name == "random_sorted":
        out = (3000, 2000) + synth.random_csr(3000, 2000, 12, sorted_rows=True, empty_every=5)
    elif name == "duplicates":            # every row lists a few columns several times
        rows, cols = 500, 64
        rng = np.random.default_rng(3)
        base = rng.integers(0, cols, (rows, 6)).astype(np.int32)
        ci = np.repeat(base, 3, axis=1).reshape(-1)
        rp = np.arange(0, 18 * rows + 1, 18, dtype=np.int32)
        out = (rows, cols, rp, ci, rng.random(len(ci)) * 2 - 1)
    elif name == "tall":                  # rows >> cols
        out = (200000, 50) + synth.random_csr(200000, 50, 5)
    elif name == "wide":                  # cols >> rows
        out = (50, 300000) + synth.random_csr(50, 300000, 400)
    elif name == "one_col":
        out = (1000, 1) + synth.random_csr(1000, 1, 3, empty_every=4)
    elif name == "four_passes":           # cols = 2^26: four 8-bit passes
        out = (500, 1 << 26) + synth.random_csr(500, 1 << 26, 8)
    elif name == "powerlaw":              # a 10^6-entry row
        out = (1000000, 1000000) + synth.powerlaw(1000000, avg=3, max_len=10 ** 6)
    elif name == "powerlaw_t":            # its host transpose: a 10^6-entry column, so a long row of A^T
        out = host_transpose_csr(*matrix("powerlaw"))
    elif name == "powerlaw40_t":          # the same with 40 nonzeros a row: its long row of A^T is split by the SpMM plan
        rp, ci, v = synth.powerlaw(1000000, avg=40, max_len=10 ** 6)
        out = host_transpose_csr(1000000, 1000000, rp, ci, v)
    elif name == "nd24k_small":
        rows, (rp, ci, v) = synth.nd24k_like(scale=0.05)
        out = (rows, rows, rp, ci, v)
    elif name == "no_nnz":
        out = (40, 30, np.zeros(41, np.int32), np.zeros(0, np.int32), np.zeros(0))
    elif name == "no_rows":
        out = (0, 30, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    elif name == "no_cols":
        out = (40, 0, np.zeros(41, np.int32), np.zeros(0, np.int32), np.zeros(0))
    _cache[name] = out
    return out


CASES = ["ash85", "random_empty", "random_sorted", "duplicates", "tall", "wide", "one_col", "four_passes", "powerlaw",
         "powerlaw_t", "nd24k_small", "no_nnz", "no_rows", "no_cols"]


@pytest.mark.parametrize("name", CASES)
def test_transpose_is_the_stable_argsort(env, name):
    S, O, torch, cuda = env
    rows, cols, rp, ci, v = matrix(name)
    want = host_csc(rows, cols, rp, ci, v)
    rp_d, ci_d, v_d = upload(torch, cuda, rp, ci, v)
    for val, with_perm in ((v_d, True), (None, True), (v_d, False)):
        cp, ri, vt, pm = S.csr_transpose(rows, cols, rp_d, ci_d, val, with_perm=with_perm)
        torch.cuda.synchronize()
        assert np.array_equal(cp.cpu().numpy(), want[0]), name
        assert np.array_equal(ri.cpu().numpy(), want[1]), name
        if val is not None:
            assert np.array_equal(vt.cpu().numpy(), want[2]), name        # a gather: bit for bit
        else:
            assert vt is None
        if with_perm:
            assert np.array_equal(pm.cpu().numpy(), want[3]), name
        else:
            assert pm is None


def test_transpose_is_deterministic_and_replays_in_a_graph(env):
    S, O, torch, cuda = env
    rows, cols, rp, ci, v = matrix("random_empty")
    rp_d, ci_d, v_d = upload(torch, cuda, rp, ci, v)
    a = S.csr_transpose(rows, cols, rp_d, ci_d, v_d)
    b = S.csr_transpose(rows, cols, rp_d, ci_d, v_d)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            out = S.csr_transpose(rows, cols, rp_d, ci_d, v_d)
    for t in out:
        t.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(a, out):
        assert torch.equal(x, y)


def _oracle_spmv(O, rows, rp, ci, v, x, y, alpha, beta):
    return O.spmv(rows, np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32), np.ascontiguousarray(v),
                  x.copy(), y.copy(), alpha, beta)


@pytest.mark.parametrize("name", ["ash85", "random_empty", "wide", "nd24k_small", "powerlaw_t", "no_nnz", "no_rows"])
def test_transposed_spmv(env, name):
    S, O, torch, cuda = env
    rows, cols, rp, ci, v = matrix(name)
    cp, ri, vt, _ = host_csc(rows, cols, rp, ci, v)
    rp_d, ci_d, v_d, cp_d, ri_d, vt_d = upload(torch, cuda, rp, ci, v, cp, ri, vt)
    plan = S.TransposePlan(rows, cols, rp_d, ci_d, v_d)
    ref_plan = S.SpmvPlan(cols, rows, cp_d, ri_d)
    rng = np.random.default_rng(11)
    x = rng.random(rows) * 2 - 1
    y0 = rng.random(cols) * 2 - 1
    x_d, = upload(torch, cuda, x)
    for alpha, beta in ((1.0, 0.0), (2.5, -0.75), (-1.0, 1.0)):
        y_d, yr_d = upload(torch, cuda, y0, y0)
        plan.spmv(x_d, alpha, beta, y_d)
        ref_plan(vt_d, x_d, alpha, beta, yr_d)
        got = y_d.cpu().numpy()
        assert np.array_equal(got, yr_d.cpu().numpy()), (name, alpha, beta)   # the SpMV plan's bits
        if cols:
            ref = _oracle_spmv(O, cols, cp, ri, vt, x, y0, alpha, beta)
            assert np.abs(got - ref).max() <= 1e-10 * max(np.abs(ref).max(), 1.0), (name, alpha, beta)
    info = plan.info()
    assert info["nnz"] == len(ci) and not info["spmm_plan"]
    if name == "powerlaw_t":                  # its 10^6-entry column is a split row of A^T
        assert info["spmv_split_rows"] >= 1
    if cols:
        assert info["bytes"] >= (cols + 1) * 4 + 16 * len(ci)
        c2 = plan.csc()
        assert np.array_equal(c2[0].cpu().numpy(), cp) and np.array_equal(c2[1].cpu().numpy(), ri)
        assert np.array_equal(c2[2].cpu().numpy(), vt)
    plan.destroy()


def _dense(B, order):
    """flat storage and leading dimension of a (r x n) numpy matrix in `order`"""
    r, n = B.shape
    return (np.ascontiguousarray(B.T).ravel(), max(r, 1)) if order == COL else (np.ascontiguousarray(B).ravel(), max(n, 1))


def _undense(flat, r, n, order):
    return flat.reshape(n, r).T if order == COL else flat.reshape(r, n)


@pytest.mark.parametrize("name", ["ash85", "random_empty", "nd24k_small"])
def test_transposed_spmm(env, name):
    S, O, torch, cuda = env
    rows, cols, rp, ci, v = matrix(name)
    cp, ri, vt, _ = host_csc(rows, cols, rp, ci, v)
    nnz = len(ci)
    rp_d, ci_d, v_d, cp_d, ri_d, vt_d = upload(torch, cuda, rp, ci, v, cp, ri, vt)
    width = 64
    plan = S.TransposePlan(rows, cols, rp_d, ci_d, v_d, n=width)
    assert plan.info()["spmm_plan"] and plan.info()["n"] == width
    ref_plan = S.SpmmPlan(cols, rows, cp_d, ri_d, width)
    rng = np.random.default_rng(5)
    for N in (1, 8, 16, 32, 64, 128, 256):
        ws = torch.empty(S.spmm_workspace_bytes(cols, rows, nnz, N) // 8 + 1, dtype=torch.float64, device=cuda)
        Bm = rng.random((rows, N)) * 2 - 1
        C0 = rng.random((cols, N)) * 2 - 1
        alpha, beta = (1.5, -0.5) if N % 16 else (1.0, 0.0)
        ref = _undense(O.spmm(cols, rows, N, cp, ri, vt, _dense(Bm, COL)[0], _dense(C0, COL)[0].copy(), alpha, beta),
                       cols, N, COL)
        for ob in (COL, ROW):
            for oc in (COL, ROW):
                Bf, ldb = _dense(Bm, ob)
                Cf, ldc = _dense(C0, oc)
                B_d, C_d, Cr_d = upload(torch, cuda, Bf, Cf, Cf)
                plan.spmm_ordered(B_d, ldb, ob, N, alpha, beta, C_d, ldc, oc, ws)
                if N == width:
                    ref_plan.spmm_ordered(vt_d, B_d, ldb, ob, N, alpha, beta, Cr_d, ldc, oc, ws)
                else:
                    S.spmm_ordered(cols, rows, cp_d, ri_d, vt_d, B_d, ldb, ob, N, alpha, beta, Cr_d, ldc, oc, ws)
                got = C_d.cpu().numpy()
                assert np.array_equal(got, Cr_d.cpu().numpy()), (name, N, ob, oc)
                g = _undense(got, cols, N, oc)
                assert np.abs(g - ref).max() <= 1e-10 * max(np.abs(ref).max(), 1.0), (name, N, ob, oc)
    # 2-D tensors: the layout from the strides
    Bt = torch.from_numpy(rng.random((rows, 48))).to(cuda)
    Ct = torch.zeros(48, cols, dtype=torch.float64, device=cuda).t()          # column-major view
    plan.spmm_tensor(Bt, Ct, 1.0, 0.0)
    Cf = torch.zeros(cols * 48, dtype=torch.float64, device=cuda)
    ws = torch.empty(S.spmm_workspace_bytes(cols, rows, nnz, 48) // 8 + 1, dtype=torch.float64, device=cuda)
    plan.spmm_ordered(Bt.reshape(-1), 48, ROW, 48, 1.0, 0.0, Cf, cols, COL, ws)
    assert torch.equal(Ct.t().reshape(-1), Cf)
    plan.destroy()


def test_split_plan_gives_the_split_spmm_plan_bits(env):
    S, O, torch, cuda = env
    rows, cols, rp, ci, v = matrix("powerlaw40_t")     # one column of 10^6 entries: a long row of A^T
    cp, ri, vt, _ = host_csc(rows, cols, rp, ci, v)
    nnz = len(ci)
    rp_d, ci_d, v_d, cp_d, ri_d, vt_d = upload(torch, cuda, rp, ci, v, cp, ri, vt)
    N = 64
    plan = S.TransposePlan(rows, cols, rp_d, ci_d, v_d, n=N, split=True)
    ref_plan = S.SpmmPlan(cols, rows, cp_d, ri_d, N, split=True)
    assert plan.info()["spmm_split_rows"] == ref_plan.split_info()["split_rows"] >= 1
    ws = torch.empty(S.spmm_workspace_bytes(cols, rows, nnz, N) // 8 + 1, dtype=torch.float64, device=cuda)
    B_d = torch.rand(rows * N, dtype=torch.float64, device=cuda)
    for ob, oc in ((COL, COL), (ROW, ROW)):
        ldb = rows if ob == COL else N
        ldc = cols if oc == COL else N
        C_d = torch.zeros(cols * N, dtype=torch.float64, device=cuda)
        Cr_d = torch.zeros(cols * N, dtype=torch.float64, device=cuda)
        plan.spmm_ordered(B_d, ldb, ob, N, 1.0, 0.0, C_d, ldc, oc, ws)
        ref_plan.spmm_ordered(vt_d, B_d, ldb, ob, N, 1.0, 0.0, Cr_d, ldc, oc, ws)
        assert torch.equal(C_d, Cr_d), (ob, oc)
    plan.destroy()
    ref_plan.destroy()


def test_update_values_and_graph_replay(env):
    S, O, torch, cuda = env
    rows, cols, rp, ci, v = matrix("random_empty")
    nnz = len(ci)
    rp_d, ci_d, v_d = upload(torch, cuda, rp, ci, v)
    N = 32
    plan = S.TransposePlan(rows, cols, rp_d, ci_d, v_d, n=N)
    rng = np.random.default_rng(9)
    x_d, = upload(torch, cuda, rng.random(rows))
    B_d, = upload(torch, cuda, rng.random(rows * N))
    ws = torch.empty(S.spmm_workspace_bytes(cols, rows, nnz, N) // 8 + 1, dtype=torch.float64, device=cuda)

    def products(p):
        y = torch.zeros(cols, dtype=torch.float64, device=cuda)
        Cm = torch.zeros(cols * N, dtype=torch.float64, device=cuda)
        p.spmv(x_d, 1.0, 0.0, y)
        p.spmm_ordered(B_d, rows, COL, N, 1.0, 0.0, Cm, cols, COL, ws)
        return y, Cm

    new_val, = upload(torch, cuda, rng.random(nnz) * 2 - 1)
    plan.update_values(new_val)
    fresh = S.TransposePlan(rows, cols, rp_d, ci_d, new_val, n=N)
    for a, b in zip(products(plan), products(fresh)):
        assert torch.equal(a, b)
    # update_values + spmv + spmm in one graph, replayed after val changes in place
    y = torch.zeros(cols, dtype=torch.float64, device=cuda)
    Cm = torch.zeros(cols * N, dtype=torch.float64, device=cuda)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            plan.update_values(v_d)
            plan.spmv(x_d, 1.0, 0.0, y)
            plan.spmm_ordered(B_d, rows, COL, N, 1.0, 0.0, Cm, cols, COL, ws)
    newer = rng.random(nnz) * 2 - 1
    v_d.copy_(torch.from_numpy(newer))
    g.replay()
    torch.cuda.synchronize()
    fresh2 = S.TransposePlan(rows, cols, rp_d, ci_d, v_d, n=N)
    y2, C2 = products(fresh2)
    assert torch.equal(y, y2) and torch.equal(Cm, C2)
    for p in (plan, fresh, fresh2):
        p.destroy()


def test_refusals(env):
    S, O, torch, cuda = env
    rows, cols, rp, ci, v = matrix("ash85")
    bad = ci.copy()
    bad[17] = cols                                     # one column index out of range
    rp_d, ci_d, v_d, bad_d = upload(torch, cuda, rp, ci, v, bad)
    with pytest.raises(S.SblasError, match="invalid argument"):
        S.TransposePlan(rows, cols, rp_d, bad_d, v_d, n=8)
    L = S.lib()
    h = C.c_void_p()
    rc = L.sblas_hip_transpose_plan_create(-1, None, rows, cols, len(ci), rp_d.data_ptr(), bad_d.data_ptr(), v_d.data_ptr(),
                                           0, 0, C.byref(h))
    assert rc == INVALID and not h.value
    plan = S.TransposePlan(rows, cols, rp_d, ci_d, v_d, n=8)
    x = torch.ones(rows, dtype=torch.float64, device=cuda)
    y = torch.zeros(cols, dtype=torch.float64, device=cuda)
    other = torch.cuda.current_device() + 1            # another device than the plan's: refused before it is touched
    assert L.sblas_hip_spmv_csr_t_f64_i32_planned(plan.handle, other, None, x.data_ptr(), 1.0, 0.0, y.data_ptr()) == INVALID
    with pytest.raises(S.SblasError):
        plan.spmv(x[:rows - 1], 1.0, 0.0, y)           # x shorter than A's rows
    ws = torch.empty(S.spmm_workspace_bytes(cols, rows, len(ci), 8) // 8 + 1, dtype=torch.float64, device=cuda)
    B = torch.ones(rows * 8, dtype=torch.float64, device=cuda)
    Cm = torch.zeros(cols * 8, dtype=torch.float64, device=cuda)
    f = L.sblas_hip_spmm_csr_t_f64_i32_planned
    call = lambda ldb, ob, ldc, oc, wsb=ws.numel() * 8, dev=-1: f(plan.handle, dev, None, B.data_ptr(), ldb, ob, 8, 1.0, 0.0,
                                                                  Cm.data_ptr(), ldc, oc, ws.data_ptr(), wsb)
    assert call(rows, COL, cols, COL) == 0
    assert call(rows - 1, COL, cols, COL) == INVALID   # B is rows x n
    assert call(rows, COL, cols - 1, COL) == INVALID   # C is cols x n
    assert call(7, ROW, cols, COL) == INVALID
    assert call(rows, COL, 7, ROW) == INVALID
    assert call(rows, COL, cols, COL, dev=other) == INVALID
    assert call(rows, COL, cols, COL, wsb=S.spmm_workspace_bytes(cols, rows, len(ci), 8) - 1) == 3
    with pytest.raises(S.SblasError):
        plan.update_values(v_d[:-1])
    plan.destroy()
