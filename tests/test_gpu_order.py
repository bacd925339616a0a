"""Row-major B and C (sblas_hip_spmm_csr_ordered & co.).  Every case is checked twice: against the oracle (column-major,
transposed in numpy) at 1e-10 relative, and bit for bit against the (COL, COL) call on the same inputs, transposed --
the summation order does not depend on the layout, so neither may a single bit of the result."""
import numpy as np
import pytest

from test_gpu_parity import SPMM_VARIANTS, Dev, _env_switch, close

pytestmark = pytest.mark.gpu

COL, ROW = 0, 1
PAIRS = [(ROW, ROW), (ROW, COL), (COL, ROW)]
WIDTHS = [1, 5, 8, 16, 32, 64, 100, 128, 256]
SENTINEL = -7.25e300


@pytest.fixture(scope="module")
def env(sblas, oracle, cuda):
    import torch
    return sblas, oracle, torch, cuda


@pytest.fixture
def variant_env():
    yield from _env_switch("SBLAS_SPMM_VARIANT")


@pytest.fixture
def chunk_env():
    yield from _env_switch("SBLAS_SPMM_MAX_BT_BYTES")


@pytest.fixture
def range_env():
    yield from _env_switch("SBLAS_STAGE_RANGE")


_SHAPES = {}


def shapes():
    if _SHAPES:
        return _SHAPES
    from sblas_amd import synth
    from test_gpu_plan import _shapes
    _SHAPES.update(_shapes(synth))
    _SHAPES["powerlaw"] = (synth.powerlaw(3000, avg=4.0, max_len=6000, cols=7000), 7000)   # one row of 6000 entries
    _SHAPES["short"] = (synth.banded(4000, 4, 30), 4000)                                     # short rows throughout
    return _SHAPES


def pack(X, order, ld, dtype=np.float64):
    """logical (r x c) array -> flat buffer in `order` at leading dimension `ld`, padding = SENTINEL"""
    r, c = X.shape
    if order == COL:
        buf = np.full(ld * c, SENTINEL, dtype)
        buf.reshape(c, ld)[:, :r] = X.T
    else:
        buf = np.full(r * ld, SENTINEL, dtype)
        buf.reshape(r, ld)[:, :c] = X
    return buf


def unpack(buf, order, ld, r, c):
    """-> (logical r x c array, padding mask of the buffer)"""
    pad = np.ones(buf.shape, bool)
    if order == COL:
        X = buf.reshape(c, ld)[:, :r].T.copy()
        pad.reshape(c, ld)[:, :r] = False
    else:
        X = buf.reshape(r, ld)[:, :c].copy()
        pad.reshape(r, ld)[:, :c] = False
    return X, pad


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


class Case:
    """one matrix on the device plus the calls of the tests below"""

    def __init__(self, env, rp, ci, v, cols):
        self.sblas, self.oracle, self.torch, self.dev = env
        self.A = Dev(self.torch, self.dev, rp, ci, v, cols)
        self.rows, self.cols, self.nnz = self.A.rows, cols, len(ci)

    def ws(self, n):
        nb = self.sblas.spmm_workspace_bytes(self.rows, self.cols, self.nnz, n)
        return self.torch.empty(max(nb, 8) // 8, dtype=self.torch.float64, device=self.dev)

    def call(self, Bl, Cl, n, alpha, beta, ob, oc, pad_b=0, pad_c=0, plan=None, ws=None):
        """-> (logical result, padding of C untouched)"""
        torch, S = self.torch, self.sblas
        ldb = (self.cols if ob == COL else n) + pad_b
        ldc = (self.rows if oc == COL else n) + pad_c
        bbuf, cbuf = pack(Bl, ob, ldb), pack(Cl, oc, ldc)
        B = torch.from_numpy(bbuf).to(self.dev)
        C = torch.from_numpy(cbuf).to(self.dev)
        ws = self.ws(n) if ws is None else ws
        if plan is None:
            S.spmm_ordered(self.rows, self.cols, self.A.rowptr, self.A.colidx, self.A.val, B, ldb, ob, n, alpha, beta, C, ldc, oc, ws)
        else:
            plan.spmm_ordered(self.A.val, B, ldb, ob, n, alpha, beta, C, ldc, oc, ws)
        torch.cuda.synchronize()
        out = C.cpu().numpy()
        X, pad = unpack(out, oc, ldc, self.rows, n)
        return X, same_bits(out[pad], cbuf[pad])

    def ref(self, Bl, Cl, n, alpha, beta):
        Cp = np.ascontiguousarray(Cl.T).reshape(-1).copy()
        Bp = np.ascontiguousarray(Bl.T).reshape(-1)
        self.oracle.spmm(self.rows, self.cols, n, *self.A.h, Bp, Cp, alpha, beta)
        return Cp.reshape(n, self.rows).T

    def check_pairs(self, n, alpha=1.5, beta=-0.5, pairs=PAIRS, seed=0, oracle=True, **kw):
        rng = np.random.default_rng(seed + n)
        Bl, Cl = rng.standard_normal((self.cols, n)), rng.standard_normal((self.rows, n))
        base, ok = self.call(Bl, Cl, n, alpha, beta, COL, COL, **{k: v for k, v in kw.items() if k in ("plan", "ws")})
        assert ok
        if oracle:
            assert close(base, self.ref(Bl, Cl, n, alpha, beta)), (n, np.abs(base - self.ref(Bl, Cl, n, alpha, beta)).max())
        for ob, oc in pairs:
            got, ok = self.call(Bl, Cl, n, alpha, beta, ob, oc, **kw)
            assert ok, ("padding of C changed", ob, oc)
            assert same_bits(got, base), (ob, oc, n, np.abs(got - base).max())
        return base


@pytest.mark.parametrize("n", WIDTHS)
@pytest.mark.parametrize("shape", ["banded", "sparse", "mixed", "grid", "blocks", "powerlaw", "short"])
def test_every_shape_and_width_matches_the_transposed_column_major_bits(env, shape, n):
    (rp, ci, v), cols = shapes()[shape]
    Case(env, rp, ci, v, cols).check_pairs(n)


@pytest.mark.parametrize("n", [5, 64, 100])
def test_padding_stays_untouched_and_beta_zero_ignores_nan(env, n):
    (rp, ci, v), cols = shapes()["mixed"]
    c = Case(env, rp, ci, v, cols)
    c.check_pairs(n, pad_b=3, pad_c=5)
    rng = np.random.default_rng(n)
    Bl = rng.standard_normal((cols, n))
    Cn = np.full((c.rows, n), np.nan)
    base, _ = c.call(Bl, Cn, n, 2.0, 0.0, COL, COL)
    assert not np.isnan(base).any()
    for ob, oc in PAIRS:
        got, ok = c.call(Bl, Cn, n, 2.0, 0.0, ob, oc, pad_b=2, pad_c=7)
        assert ok and same_bits(got, base), (ob, oc)


@pytest.mark.parametrize("n", [8, 32, 64, 128])
@pytest.mark.parametrize("variant", SPMM_VARIANTS)
def test_every_kernel_selection(env, variant_env, variant, n):
    variant_env(variant)
    for i, shape in enumerate(("mixed", "grid", "blocks", "short")):
        (rp, ci, v), cols = shapes()[shape]
        Case(env, rp, ci, v, cols).check_pairs(n, seed=31 * i)


@pytest.mark.parametrize("n", [64, 200, 300])
def test_column_chunks_and_range_staging(env, chunk_env, range_env, n):
    from sblas_amd import synth
    K = 700
    rp, ci, v = synth.banded(K, 30, 60)
    for limit in (8 * 701 * 128, 8 * 701 * 64, 8 * 701 * 40):
        chunk_env(str(limit))
        Case(env, rp, ci, v, K).check_pairs(n)
    chunk_env(str(0xffffffff))
    # a re-based row block (method 2) with range staging, C offset to the block's first row inside a taller C
    sub = (rp[200:451] - rp[200]).astype(np.int32)
    c = Case(env, sub, ci[rp[200]:rp[450]], v[rp[200]:rp[450]], K)
    for rs in ("1", "0"):
        range_env(rs)
        for limit in (0xffffffff, 8 * 701 * 64):
            chunk_env(str(limit))
            c.check_pairs(n)
            # the same through an offset C: rows 200..449 of a 700-row C
            rng = np.random.default_rng(n)
            Bl, Cfull = rng.standard_normal((K, n)), rng.standard_normal((K, n))
            S, torch = c.sblas, c.torch
            outs = {}
            for ob, oc in [(COL, COL)] + PAIRS:
                ldb, ldc = (K if ob == COL else n), (K if oc == COL else n)
                B = torch.from_numpy(pack(Bl, ob, ldb)).to(c.dev)
                C = torch.from_numpy(pack(Cfull, oc, ldc)).to(c.dev)
                off = 200 if oc == COL else 200 * ldc
                S.spmm_ordered(c.rows, K, c.A.rowptr, c.A.colidx, c.A.val, B, ldb, ob, n, 1.5, -1.0, C, ldc, oc, c.ws(n),
                               c_offset=off)
                torch.cuda.synchronize()
                outs[(ob, oc)] = unpack(C.cpu().numpy(), oc, ldc, K, n)[0]
            want = Cfull.copy()
            want[200:450] = c.ref(Bl, Cfull[200:450], n, 1.5, -1.0)
            assert close(outs[(COL, COL)], want)
            for k in PAIRS:
                assert same_bits(outs[k], outs[(COL, COL)]), k


def test_mfma_panels_and_nonfinite_b(env, variant_env):
    (rp, ci, v), cols = shapes()["blocks"]
    c = Case(env, rp, ci, v, cols)
    n = 128
    rng = np.random.default_rng(1)
    Bl, Cl = rng.standard_normal((cols, n)), rng.standard_normal((c.rows, n))
    Bl[int(ci[len(ci) // 2]), 3] = np.inf
    base, _ = c.call(Bl, Cl, n, 1.0, 1.0, COL, COL)
    for ob, oc in PAIRS:
        got, ok = c.call(Bl, Cl, n, 1.0, 1.0, ob, oc)
        assert ok and same_bits(got, base), (ob, oc)
    c.sblas.panel_census()
    c.check_pairs(n)
    census = c.sblas.panel_census()
    assert census["mfma"] > 0, census
    variant_env("mfma")
    c.check_pairs(64)


def test_plans_serve_every_order(env):
    for shape, n in (("mixed", 64), ("blocks", 128), ("grid", 256), ("banded", 16), ("powerlaw", 8)):
        (rp, ci, v), cols = shapes()[shape]
        c = Case(env, rp, ci, v, cols)
        plan = c.sblas.SpmmPlan(c.rows, cols, c.A.rowptr, c.A.colidx, n)
        try:
            ws = c.ws(n)
            base = c.check_pairs(n, ws=ws)
            planned = c.check_pairs(n, plan=plan, ws=ws)            # planned (COL, COL) and every pair through one plan
            assert same_bits(base, planned), shape
            for ob, oc in PAIRS * 2:                                  # alternating orders on the same plan
                rng = np.random.default_rng(n)
                Bl, Cl = rng.standard_normal((cols, n)), rng.standard_normal((c.rows, n))
                got, ok = c.call(Bl, Cl, n, 1.5, -0.5, ob, oc, plan=plan, ws=ws)
                assert ok and same_bits(got, base), (shape, ob, oc)
        finally:
            plan.destroy()


def test_planned_row_major_call_replays_in_a_graph(env):
    (rp, ci, v), cols = shapes()["mixed"]
    c = Case(env, rp, ci, v, cols)
    S, torch, dev = c.sblas, c.torch, c.dev
    n = 64
    rng = np.random.default_rng(3)
    Bl, Cl = rng.standard_normal((cols, n)), rng.standard_normal((c.rows, n))
    want, _ = c.call(Bl, Cl, n, 1.0, 0.0, COL, COL)
    plan = S.SpmmPlan(c.rows, cols, c.A.rowptr, c.A.colidx, n)
    B = torch.from_numpy(np.ascontiguousarray(Bl)).to(dev)
    C = torch.zeros(c.rows, n, dtype=torch.float64, device=dev)
    ws = c.ws(n)
    plan.spmm_ordered(c.A.val, B, n, ROW, n, 1.0, 0.0, C, n, ROW, ws)        # (outside the capture first)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.spmm_ordered(c.A.val, B, n, ROW, n, 1.0, 0.0, C, n, ROW, ws)
    C.fill_(np.nan)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(C.cpu().numpy(), want)
    del g
    plan.destroy()


@pytest.mark.parametrize("types", [("f32", "i32"), ("f64", "i64"), ("f32", "i64")])
@pytest.mark.parametrize("n", [5, 64, 100])
def test_typed_pairs(env, types, n):
    sblas, oracle, torch, dev = env
    from sblas_amd import synth
    vt = {"f32": np.float32, "f64": np.float64}[types[0]]
    it = {"i32": np.int32, "i64": np.int64}[types[1]]
    M, K = 400, 350
    rp, ci, v = synth.random_csr(M, K, 10, seed=n, long_row=(100, 300))
    rp, ci, v = rp.astype(it), ci.astype(it), v.astype(vt)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    drp, dci, dv = up(rp), up(ci), up(v)
    rng = np.random.default_rng(n)
    Bl, Cl = rng.standard_normal((K, n)).astype(vt), rng.standard_normal((M, n)).astype(vt)
    ws = torch.empty(max(sblas.spmm_typed_workspace_bytes(dv.dtype, drp.dtype, M, K, len(ci), n), 1), dtype=torch.uint8, device=dev)
    outs = {}
    for ob, oc in [(COL, COL)] + PAIRS:
        ldb, ldc = (K if ob == COL else n) + 1, (M if oc == COL else n) + 2
        cbuf = pack(Cl, oc, ldc, vt)
        B, C = up(pack(Bl, ob, ldb, vt)), up(cbuf)
        sblas.spmm_ordered(M, K, drp, dci, dv, B, ldb, ob, n, 0.5, 2.0, C, ldc, oc, ws)
        torch.cuda.synchronize()
        out = C.cpu().numpy()
        X, pad = unpack(out, oc, ldc, M, n)
        assert same_bits(out[pad], cbuf[pad])
        outs[(ob, oc)] = X
    ref = oracle.spmm_typed(M, K, n, rp, ci, v, np.ascontiguousarray(Bl.T).reshape(-1),
                            np.ascontiguousarray(Cl.T).reshape(-1).copy(), 0.5, 2.0).reshape(n, M).T
    tol = 1e-4 if vt == np.float32 else 1e-10
    assert np.allclose(outs[(COL, COL)], ref, rtol=tol, atol=tol * 1e-2)
    for k in PAIRS:
        assert same_bits(outs[k], outs[(COL, COL)]), k


def test_empty_cases(env):
    sblas, oracle, torch, dev = env
    from sblas_amd import synth
    rp, ci, v = synth.banded(300, 5, 10)
    c = Case(env, rp, ci, v, 300)
    # nnz = 0: C = beta * C only, padding untouched
    z = Case(env, np.zeros(301, np.int32), np.zeros(0, np.int32), np.zeros(0), 300)
    for beta in (0.5, 0.0, 1.0):
        z.check_pairs(40, beta=beta, pad_c=3, oracle=False)
        rng = np.random.default_rng(0)
        got, ok = z.call(rng.standard_normal((300, 40)), np.full((300, 40), 3.0), 40, 1.0, beta, ROW, ROW, pad_c=3)
        assert ok and (got == 3.0 * beta).all()
    # cols = 0 (no B at all)
    e = Case(env, np.zeros(51, np.int32), np.zeros(0, np.int32), np.zeros(0), 0)
    for ob, oc in PAIRS:
        Cl = np.full((50, 7), 2.0)
        ldc = (50 if oc == COL else 7) + 1
        cb = pack(Cl, oc, ldc)
        C = torch.from_numpy(cb).to(dev)
        sblas.spmm_ordered(50, 0, e.A.rowptr, e.A.colidx, e.A.val, None, 7, ob, 7, 1.0, 0.25, C, ldc, oc, None)
        torch.cuda.synchronize()
        X, pad = unpack(C.cpu().numpy(), oc, ldc, 50, 7)
        assert (X == 0.5).all() and same_bits(C.cpu().numpy()[pad], cb[pad])
    # rows = 0 and n = 0: nothing to do, nothing touched
    C = torch.full((10,), 9.0, dtype=torch.float64, device=dev)
    B = torch.ones(300 * 4, dtype=torch.float64, device=dev)
    r0 = torch.zeros(1, dtype=torch.int32, device=dev)
    sblas.spmm_ordered(0, 300, r0, c.A.colidx, c.A.val, B, 4, ROW, 4, 1.0, 0.0, C, 4, ROW, c.ws(4))
    sblas.spmm_ordered(300, 300, c.A.rowptr, c.A.colidx, c.A.val, B, 4, ROW, 0, 1.0, 0.0, C, 4, ROW, c.ws(4))
    torch.cuda.synchronize()
    assert (C.cpu().numpy() == 9.0).all()


def test_spmm_tensor_views_need_no_copy(env):
    sblas, oracle, torch, dev = env
    (rp, ci, v), cols = shapes()["mixed"]
    c = Case(env, rp, ci, v, cols)
    A = (c.rows, cols, c.A.rowptr, c.A.colidx, c.A.val)
    n = 48
    rng = np.random.default_rng(7)
    Bl, Cl = rng.standard_normal((cols, n)), rng.standard_normal((c.rows, n))
    want, _ = c.call(Bl, Cl, n, 1.25, 0.5, COL, COL)
    # contiguous (row-major) tensors
    B = torch.from_numpy(Bl.copy()).to(dev)
    C = torch.from_numpy(Cl.copy()).to(dev)
    sblas.spmm_tensor(A, B, C, 1.25, 0.5)
    torch.cuda.synchronize()
    assert same_bits(C.cpu().numpy(), want)
    # .t() views of column-major storage
    Bt = torch.from_numpy(np.ascontiguousarray(Bl.T)).to(dev).t()
    Ct = torch.from_numpy(np.ascontiguousarray(Cl.T)).to(dev).t()
    sblas.spmm_tensor(A, Bt, Ct, 1.25, 0.5)
    torch.cuda.synchronize()
    assert same_bits(Ct.cpu().numpy(), want)
    # column slices of wider tensors (the columns around them untouched)
    Bw = torch.from_numpy(np.hstack([np.full((cols, 3), 5.0), Bl, np.full((cols, 2), 5.0)])).to(dev)
    Cw0 = np.hstack([np.full((c.rows, 4), SENTINEL), Cl, np.full((c.rows, 1), SENTINEL)])
    Cw = torch.from_numpy(Cw0.copy()).to(dev)
    plan = sblas.SpmmPlan(c.rows, cols, c.A.rowptr, c.A.colidx, n)
    sblas.spmm_tensor(A, Bw[:, 3:3 + n], Cw[:, 4:4 + n], 1.25, 0.5, plan=plan)
    torch.cuda.synchronize()
    out = Cw.cpu().numpy()
    assert same_bits(out[:, 4:4 + n], want)
    assert same_bits(out[:, :4], Cw0[:, :4]) and same_bits(out[:, 4 + n:], Cw0[:, 4 + n:])
    plan.destroy()


@pytest.mark.parametrize("g", [2, 3])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_merge_rowblocks_on_folded_ranks(env, g, dt):
    sblas, oracle, torch, dev = env
    from sblas_amd import synth
    vt = {"f64": np.float64, "f32": np.float32}[dt]
    M, K, N = 500, 400, 37
    rp, ci, v = synth.random_csr(M, K, 9, seed=g, long_row=(50, 300))
    v = v.astype(vt)
    rng = np.random.default_rng(g)
    Cl = rng.standard_normal((M, N)).astype(vt)
    parts = [sblas.partition_nnz(rp, g, q) for q in range(g)]
    starts = [p["start_row"] for p in parts]
    nrows = [len(p["rowptr"]) - 1 for p in parts]
    blocks = [rng.standard_normal((m, N)).astype(vt) for m in nrows]
    comm = sblas.comm_get([0] * g)
    streams = [torch.cuda.Stream(device=dev) for _ in range(g)]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    res = {}
    for order in (COL, ROW):
        ldc = (M if order == COL else N) + 3
        part = [up(b.T.reshape(-1) if order == COL else b.reshape(-1)) for b in blocks]
        Cs = [up(pack(Cl, order, ldc, vt)) for _ in range(g)]
        torch.cuda.synchronize()
        sblas.merge_rowblocks_ordered(comm, order, M, N, starts, nrows, part, None, 1.5, -0.5, Cs, ldc, streams)
        torch.cuda.synchronize()
        res[order] = [unpack(C_.cpu().numpy(), order, ldc, M, N)[0] for C_ in Cs]
    want = -0.5 * Cl.astype(np.float64)
    acc = np.zeros((M, N))
    for q in range(g):
        acc[starts[q]:starts[q] + nrows[q]] += blocks[q]
    want += 1.5 * acc
    for q in range(g):
        assert same_bits(res[ROW][q], res[COL][q]), q
        assert np.allclose(res[COL][q], want, rtol=1e-5 if vt == np.float32 else 1e-12, atol=1e-5 if vt == np.float32 else 1e-12)
