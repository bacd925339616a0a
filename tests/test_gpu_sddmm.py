"""SDDMM on the GPU (sblas_hip_sddmm_csr_f64_i32 through sblas_amd.sddmm / sddmm_tensor) against arithmetic yardsticks:
exact grids with ==, the gamma(k + 2) bound against a double-double reference, and the contract that the bits of an
output are a function of its two operand rows, k, alpha, beta and the old value alone."""
import os

import numpy as np
import pytest

import sddmm_numerics as SN

pytestmark = pytest.mark.gpu

ROW, COL = 1, 0
ORDERS = [(ROW, ROW), (ROW, COL), (COL, ROW), (COL, COL)]
KS = [0, 1, 2, 3, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 128, 129, 256, 300]
AB = [(1.0, 0.0), (-2.0, 0.5), (0.5, 1.0)]

_cache = {}


def pattern(name):
    """(rows, cols, rowptr, colidx) as numpy arrays"""
    if name in _cache:
        return _cache[name]
    from sblas_amd import synth
    if name == "random":          # unsorted rows, duplicate columns, empty rows, one long row
        rows, cols = 3000, 2500
        rp, ci, _ = synth.random_csr(rows, cols, 6, empty_every=7, long_row=(11, 5000))
    elif name == "powerlaw":      # a row of 120 000 entries among rows of one to three
        rows = cols = 150000
        rp, ci, _ = synth.powerlaw(rows, max_len=120000)
    elif name == "banded":
        rows = cols = 20000
        rp, ci, _ = synth.banded(rows, 5, 40)
    elif name == "nd24k_slice":   # 500 rows of 399 entries
        full_rows, (rp, ci, _) = synth.nd24k_like(0.05)
        rows, cols = 500, full_rows
        rp = rp[:rows + 1].copy()
        ci = ci[:rp[-1]].copy()
    elif name == "ash85":
        import sblas_amd as S
        rows, cols, _, _, rp, ci, _ = S.read_mtx(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ash85.mtx"))
    elif name == "empty":
        rows, cols, rp, ci = 0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32)
    elif name == "empty_rows":
        rows, cols, rp, ci = 100, 50, np.zeros(101, np.int32), np.zeros(0, np.int32)
    elif name == "dups":          # every row: unsorted columns, each listed twice and one three times
        rows, cols = 400, 300
        rng = np.random.default_rng(5)
        parts, lens = [], []
        for r in range(rows):
            c = rng.choice(cols, size=int(rng.integers(0, 9)), replace=False)
            row = np.concatenate([c, c, c[:1]])
            rng.shuffle(row)
            parts.append(row)
            lens.append(len(row))
        rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        ci = np.concatenate(parts).astype(np.int32)
    else:
        raise KeyError(name)
    out = (int(rows), int(cols), np.asarray(rp, np.int32), np.asarray(ci, np.int32))
    _cache[name] = out
    return out


def dev_operand(torch, dev, M, order, pad=0, fill=0.0, offset=False, extra_row=False):
    """M (r x k numpy) as a device view in `order` with leading dimension minimum + pad; the padding (and one extra row
    behind the last when asked) holds `fill`.  offset: the view starts 8 bytes into its base (row-major only)."""
    r, k = M.shape
    Mt = torch.from_numpy(np.ascontiguousarray(M)).to(dev)
    if order == ROW:
        ld = k + pad + (1 if offset else 0)
        base = torch.full((r + (1 if extra_row else 0), max(ld, 1)), fill, dtype=torch.float64, device=dev)
        o = 1 if offset else 0
        view = base[:r, o:o + k]
    else:
        ld = r + pad + (1 if extra_row else 0)
        base = torch.full((max(k, 1), max(ld, 1)), fill, dtype=torch.float64, device=dev)
        view = base.t()[:r, :k]
    view.copy_(Mt)
    return view


def run(S, torch, dev, pat, X, Y, alpha, beta, old=None, orders=(ROW, ROW), **kw):
    rows, cols, rp, ci = pat
    R, Cx = torch.from_numpy(rp).to(dev), torch.from_numpy(ci).to(dev)
    Xd = dev_operand(torch, dev, X, orders[0], **kw)
    Yd = dev_operand(torch, dev, Y, orders[1], **kw)
    out = torch.from_numpy(np.ascontiguousarray(old)).to(dev) if old is not None else torch.full((len(ci),), float("nan"),
                                                                                                 dtype=torch.float64, device=dev)
    S.sddmm_tensor((rows, cols, R, Cx), Xd, Yd, out, alpha, beta)
    return out.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def general(pat, k, seed=0, binades=24):
    rows, cols, rp, ci = pat
    rng = np.random.default_rng(seed)
    return (SN.log_uniform(rng, (rows, k), binades), SN.log_uniform(rng, (cols, k), binades), SN.log_uniform(rng, len(ci), binades))


# ---- 1. exact grids ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_exact_grid_every_order_pair(sblas, cuda, k):
    import torch
    pat = pattern("random")
    rows, cols, rp, ci = pat
    for alpha, beta in AB:
        g = SN.grid_problem(rp, ci, rows, cols, k, alpha, beta, seed=k)
        for orders in ORDERS:
            got = run(sblas, torch, cuda, pat, g.X, g.Y, alpha, beta, g.old, orders)
            bad = np.flatnonzero(got != g.expected)
            assert len(bad) == 0, "k=%d alpha=%g beta=%g orders=%s: %d of %d entries differ, first %d: %r != %r" % (
                k, alpha, beta, orders, len(bad), len(ci), bad[0], got[bad[0]], g.expected[bad[0]])


@pytest.mark.parametrize("name", ["powerlaw", "banded", "nd24k_slice", "ash85", "dups", "empty", "empty_rows"])
@pytest.mark.parametrize("k", [1, 5, 64, 100])
def test_exact_grid_structures(sblas, cuda, name, k):
    import torch
    pat = pattern(name)
    rows, cols, rp, ci = pat
    g = SN.grid_problem(rp, ci, rows, cols, k, -2.0, 0.5, seed=3)
    for orders in ((ROW, ROW), (COL, COL)):
        got = run(sblas, torch, cuda, pat, g.X, g.Y, -2.0, 0.5, g.old, orders)
        assert got.shape == g.expected.shape and (got == g.expected).all(), "%s k=%d orders=%s" % (name, k, orders)


# ---- 2. general data within the bound ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ks", [("random", [1, 2, 3, 7, 17, 33, 64, 100, 129, 300]), ("powerlaw", [1, 64]),
                                     ("nd24k_slice", [16, 64, 256]), ("banded", [8, 65]), ("ash85", [5, 64])])
def test_general_data_within_the_bound(sblas, cuda, name, ks):
    import torch
    pat = pattern(name)
    _, _, rp, ci = pat
    for k in ks:
        X, Y, old = general(pat, k, seed=k)
        for alpha, beta in ((1.0, 0.0), (-1.75, 0.3)):
            got = run(sblas, torch, cuda, pat, X, Y, alpha, beta, old)
            ok, worst, where, over = SN.check_general(got, rp, ci, X, Y, old, alpha, beta)
            print("%s k=%d alpha=%g beta=%g: worst err/bound = %.3g" % (name, k, alpha, beta, worst))
            assert ok, "%s k=%d alpha=%g beta=%g: %d entries over the bound, worst %.3g at entry %s" % (
                name, k, alpha, beta, over, worst, where)


# ---- 3. the order is a function of k alone -------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 13, 16, 17, 33, 64, 100, 129, 257, 300])
def test_layouts_leading_dimensions_and_alignment_agree_bitwise(sblas, cuda, k):
    import torch
    pat = pattern("random")
    X, Y, old = general(pat, k, seed=100 + k)
    ref = bits(run(sblas, torch, cuda, pat, X, Y, -1.5, 0.75, old))
    for orders in ORDERS[1:]:
        assert (bits(run(sblas, torch, cuda, pat, X, Y, -1.5, 0.75, old, orders)) == ref).all(), orders
    for pad in (1, 3):
        for orders in ORDERS:
            assert (bits(run(sblas, torch, cuda, pat, X, Y, -1.5, 0.75, old, orders, pad=pad)) == ref).all(), (pad, orders)
    # the view T[:, 1:1 + k]: a base 8 bytes off a 16-byte boundary, even and odd leading dimensions
    for pad in (0, 1):
        assert (bits(run(sblas, torch, cuda, pat, X, Y, -1.5, 0.75, old, (ROW, ROW), pad=pad, offset=True)) == ref).all(), pad


@pytest.mark.parametrize("k", [1, 7, 64, 130])
def test_bits_follow_the_entry_not_its_place(sblas, cuda, k):
    import torch
    pat = pattern("random")
    rows, cols, rp, ci = pat
    X, Y, old = general(pat, k, seed=7 * k)
    alpha, beta = 1.25, -0.5
    ref = bits(run(sblas, torch, cuda, pat, X, Y, alpha, beta, old))
    rng = np.random.default_rng(k)
    # a random permutation of the entries inside every row permutes the output
    perm = np.arange(len(ci))
    for r in range(rows):
        rng.shuffle(perm[rp[r]:rp[r + 1]])
    got = bits(run(sblas, torch, cuda, (rows, cols, rp, ci[perm]), X, Y, alpha, beta, old[perm]))
    assert (got == ref[perm]).all()
    # the rows reordered (the lengths around an entry change): the same bits per (row, col, old)
    rperm = rng.permutation(rows)
    lens = np.diff(rp.astype(np.int64))[rperm]
    rp2 = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    src = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in rperm]) if len(ci) else np.zeros(0, np.int64)
    got = bits(run(sblas, torch, cuda, (rows, cols, rp2, ci[src]), X[rperm], Y, alpha, beta, old[src]))
    assert (got == ref[src]).all()
    # duplicates of one (row, col) with equal old values get equal bits
    dp = pattern("dups")
    Xd, Yd, _ = general(dp, k, seed=k + 1)
    got = bits(run(sblas, torch, cuda, dp, Xd, Yd, alpha, 0.0))
    key = SN.row_of_entries(dp[2]) * dp[1] + dp[3]
    order = np.argsort(key, kind="stable")
    same = key[order][1:] == key[order][:-1]
    assert same.sum() > 100 and (got[order][1:][same] == got[order][:-1][same]).all()


@pytest.mark.parametrize("name", ["random", "powerlaw"])
@pytest.mark.parametrize("k", [1, 64])
def test_rebased_row_blocks_give_the_bits_of_the_whole_call(sblas, cuda, name, k):
    import torch
    pat = pattern(name)
    rows, cols, rp, ci = pat
    X, Y, old = general(pat, k, seed=11)
    alpha, beta = -0.5, 2.0
    ref = bits(run(sblas, torch, cuda, pat, X, Y, alpha, beta, old))
    Xd = torch.from_numpy(X).to(cuda)
    Yd = torch.from_numpy(Y).to(cuda)
    Cd = torch.from_numpy(ci).to(cuda)
    out = torch.from_numpy(old.copy()).to(cuda)
    g = 3
    for i in range(g):
        part = sblas.partition_nnz(rp, g, i)
        start, nnz_i, first, reb = part["start_row"], part["nnz"], part["first_nnz"], part["rowptr"]
        R = torch.from_numpy(np.asarray(reb, np.int32)).to(cuda)
        nrows = len(reb) - 1
        sblas.sddmm(nrows, cols, R, Cd[first:first + nnz_i], Xd, k, ROW, Yd, k, ROW, k, alpha, beta, out[first:first + nnz_i],
                    x_offset=start * k)
    assert (bits(out.cpu().numpy()) == ref).all()


# ---- 4. tails ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 5, 13, 17, 33, 63, 65, 127, 129, 299])
def test_padding_and_the_row_behind_the_last_are_never_read_into_a_product(sblas, cuda, k):
    import torch
    pat = pattern("random")
    X, Y, old = general(pat, k, seed=k)
    for orders in ORDERS:
        ref = bits(run(sblas, torch, cuda, pat, X, Y, 1.0, 0.0, None, orders, pad=3, extra_row=True))
        for fill in (float("nan"), float("inf")):
            got = bits(run(sblas, torch, cuda, pat, X, Y, 1.0, 0.0, None, orders, pad=3, fill=fill, extra_row=True))
            assert (got == ref).all(), (orders, fill)
            assert np.isfinite(got.view(np.float64)).all()


# ---- 5. non-finite operands ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4, 33, 64, 200])
def test_ieee_classes_and_beta_zero(sblas, cuda, k):
    import torch
    pat = pattern("random")
    rows, cols, rp, ci = pat
    rng = np.random.default_rng(k)
    X = rng.uniform(-1, 1, (rows, k))
    Y = rng.uniform(-1, 1, (cols, k))
    old = rng.uniform(-1, 1, len(ci))
    specials = [np.nan, np.inf, -np.inf, 0.0]
    for M in (X, Y):
        idx = rng.integers(0, M.size, max(4, M.size // 300))
        M.flat[idx] = rng.choice(specials, len(idx))
    old[rng.integers(0, len(ci), len(ci) // 50)] = rng.choice(specials[:3], len(ci) // 50)
    for alpha, beta in ((1.0, 0.0), (-2.0, 0.5)):
        for orders in ((ROW, ROW), (COL, COL)):
            got = run(sblas, torch, cuda, pat, X, Y, alpha, beta, old, orders)
            want = SN.predict_class(rp, ci, X, Y, old, alpha, beta)
            have = SN.class_of(got)
            bad = np.flatnonzero(want != have)
            assert len(bad) == 0, "%d entries in the wrong class, first %d: want %d got %r" % (len(bad), bad[0], want[bad[0]], got[bad[0]])
    # beta == 0: out is not read
    Xf, Yf, _ = general(pat, k, seed=1)
    got = run(sblas, torch, cuda, pat, Xf, Yf, 1.0, 0.0, np.full(len(ci), np.nan))
    assert np.isfinite(got).all()


# ---- 6. determinism ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orders", [(ROW, ROW), (COL, ROW)])
def test_repeated_calls_and_graph_replay_give_the_same_bits(sblas, cuda, orders):
    import torch
    pat = pattern("random")
    rows, cols, rp, ci = pat
    k = 48
    X, Y, old = general(pat, k, seed=2)
    first = bits(run(sblas, torch, cuda, pat, X, Y, 0.5, 0.25, old, orders))
    for _ in range(4):
        assert (bits(run(sblas, torch, cuda, pat, X, Y, 0.5, 0.25, old, orders)) == first).all()
    R, Cx = torch.from_numpy(rp).to(cuda), torch.from_numpy(ci).to(cuda)
    A = (rows, cols, R, Cx)
    Xd = dev_operand(torch, cuda, X, orders[0])
    Yd = dev_operand(torch, cuda, Y, orders[1])
    out = torch.zeros(len(ci), dtype=torch.float64, device=cuda)
    need = sblas.sddmm_workspace_bytes(rows, cols, len(ci), k, orders[0], orders[1])
    ws = torch.empty((need + 7) // 8, dtype=torch.float64, device=cuda)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sblas.sddmm_tensor(A, Xd, Yd, out, 0.5, 0.0, workspace=ws)   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sblas.sddmm_tensor(A, Xd, Yd, out, 0.5, 0.0, workspace=ws)
    for step in range(3):
        Xn, Yn, _ = general(pat, k, seed=50 + step)
        Xd.copy_(torch.from_numpy(Xn).to(cuda))
        Yd.copy_(torch.from_numpy(Yn).to(cuda))
        graph.replay()
        torch.cuda.synchronize()
        replayed = bits(out.cpu().numpy())
        eager = bits(run(sblas, torch, cuda, pat, Xn, Yn, 0.5, 0.0, None, orders))
        assert (replayed == eager).all(), step


# ---- 7. SBLAS_VALIDATE ---------------------------------------------------------------------------------------------
def test_validate_refuses_a_column_outside_the_matrix_and_writes_nothing(sblas, cuda, monkeypatch):
    import torch
    rows, cols, rp, ci = pattern("random")
    bad = ci.copy()
    bad[len(bad) // 2] = cols
    R, Cx = torch.from_numpy(rp).to(cuda), torch.from_numpy(bad).to(cuda)
    X = torch.ones(rows, 8, dtype=torch.float64, device=cuda)
    Y = torch.ones(cols, 8, dtype=torch.float64, device=cuda)
    out = torch.full((len(ci),), -7.0, dtype=torch.float64, device=cuda)
    monkeypatch.setenv("SBLAS_VALIDATE", "1")
    sblas.reload_env()
    try:
        with pytest.raises(sblas.SblasError, match="code 1"):
            sblas.sddmm_tensor((rows, cols, R, Cx), X, Y, out, 1.0, 0.0)
        torch.cuda.synchronize()
        assert (out == -7.0).all()
        good = torch.from_numpy(ci).to(cuda)
        sblas.sddmm_tensor((rows, cols, R, good), X, Y, out, 1.0, 0.0)
        assert (out == 8.0).all()
    finally:
        monkeypatch.delenv("SBLAS_VALIDATE")
        sblas.reload_env()
