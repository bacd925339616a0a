"""Row-wise softmax on a CSR pattern on the GPU (sblas_hip_csr_softmax_f64_i32 and its backward through sblas_amd) and
CsrOperator.softmax / CsrOperator.sddmm: the error bounds of softmax_numerics against its Decimal references, the contract
that the bits of a row's outputs are a function of the row's values, its length and scale alone, the IEEE classes, and
autograd."""
import numpy as np
import pytest

import softmax_numerics as XN

pytestmark = pytest.mark.gpu

SCALES = (1.0, 0.125)            # 0.125 = 64 ** -0.5
LONG = 100000                    # the neighbours of the embedding tests
# lengths around every path and cell boundary: the 8-lane group, one cell (64), the register path (512), the rows kernel's
# limit and first supercell (4096), the second and third supercell
EDGES = [7, 8, 9, 63, 64, 65, 127, 128, 129, 511, 512, 513, 575, 576, 577, 4032, 4095, 4096, 4097, 4160, 8191, 8192, 8193,
         12287, 12288, 12289, 12353]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def rowptr_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def forward(S, torch, dev, rp, x, scale, inplace=False):
    R = torch.from_numpy(np.ascontiguousarray(rp, np.int32)).to(dev)
    X = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    out = X if inplace else torch.full_like(X, float("nan"))
    S.csr_softmax(R, X, out, scale)
    return out.cpu().numpy()


def backward(S, torch, dev, rp, p, dp, scale, inplace=False):
    R = torch.from_numpy(np.ascontiguousarray(rp, np.int32)).to(dev)
    P = torch.from_numpy(np.ascontiguousarray(p)).to(dev)
    DP = torch.from_numpy(np.ascontiguousarray(dp)).to(dev)
    dx = DP if inplace else torch.full_like(DP, float("nan"))
    S.csr_softmax_backward(R, P, DP, dx, scale)
    return dx.cpu().numpy()


def gradients(rp, seed):
    """p (a softmax of the pattern, from numpy) and dp of mixed sign"""
    rng = np.random.default_rng(seed)
    p = XN.numpy_forward(rp, XN.scores(rp, seed, spread=20.0), 1.0)
    return p, rng.uniform(-2.0, 2.0, len(p))


# ---- 1. within the bound -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "mixed", "ash85", "banded", "powerlaw", "nd24k_slice"])
def test_forward_within_the_bound(sblas, cuda, name):
    """Every entry of the sampled rows (all rows of the small inputs; XN.SAMPLE_ROWS = 24 rows drawn by seed plus the longest
    and a one-entry row of the large ones) within the relative bound, no entry excused; every such row sums to 1."""
    import torch
    rp = XN.pattern(name)
    rows = XN.sample_rows(rp)
    for scale in SCALES:
        x = XN.scores(rp, seed=3, scale=scale)
        got = forward(sblas, torch, cuda, rp, x, scale)
        res = XN.check_forward(got, rp, x, scale, rows)
        print("softmax %s scale=%g: %d entries, worst err/bound = %.3g, largest relative error = %.2f u, worst |row sum - 1| / "
              "bound = %.3g" % (name, scale, res["entries"], res["worst"], res["worst_u"], res["sum_worst"]))
        assert res["ok"], res
        lens = np.diff(rp.astype(np.int64))
        assert not np.isnan(got).any()
        one = np.flatnonzero(lens == 1)
        assert (got[rp[:-1][one]] == 1.0).all()                     # a one-entry row is exactly 1


def test_forward_underflow_within_the_absolute_bound(sblas, cuda):
    import torch
    rp, x = XN.wide_row()
    got = forward(sblas, torch, cuda, rp, x, 1.0)
    res = XN.check_forward(got, rp, x, 1.0, absolute=True)
    print("softmax spread 1500: worst err/bound = %.3g, worst |row sum - 1| / bound = %.3g, zeros %d" % (
        res["worst"], res["sum_worst"], int((got == 0).sum())))
    assert res["ok"], res
    assert (got >= 0).all() and (got == 0).sum() > 100 and not np.signbit(got).any()


@pytest.mark.parametrize("name", ["small", "mixed", "ash85", "banded", "powerlaw", "nd24k_slice"])
def test_backward_within_the_bound(sblas, cuda, name):
    import torch
    rp = XN.pattern(name)
    rows = XN.sample_rows(rp)
    p, dp = gradients(rp, 5)
    for scale in SCALES:
        got = backward(sblas, torch, cuda, rp, p, dp, scale)
        res = XN.check_backward(got, rp, p, dp, scale, rows)
        print("softmax backward %s scale=%g: %d entries, worst err/bound = %.3g" % (name, scale, res["entries"], res["worst"]))
        assert res["ok"], res


# ---- 2. the bits follow the row ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "powerlaw"])
def test_backward_equals_the_documented_order_bit_for_bit(sblas, cuda, name):
    """Every operation of the backward is a correctly rounded IEEE +, -, * or fma, so the documented order can be carried
    out in numpy: the kernels (8-lane groups, register rows, rows in passes, supercells across workgroups) must give its bits."""
    import torch
    rp = XN.pattern(name)
    p, dp = gradients(rp, 9)
    for scale in (1.0, -0.3):
        got = backward(sblas, torch, cuda, rp, p, dp, scale)
        want = XN.emulate_backward(rp, p, dp, scale)
        bad = np.flatnonzero(bits(got) != bits(want))
        assert len(bad) == 0, "%d entries differ, first %d: %r != %r" % (len(bad), bad[0], got[bad[0]], want[bad[0]])


def test_backward_edge_lengths_equal_the_documented_order(sblas, cuda):
    import torch
    rp = rowptr_of(EDGES)
    p, dp = gradients(rp, 2)
    got = backward(sblas, torch, cuda, rp, p, dp, 0.7)
    assert (bits(got) == bits(XN.emulate_backward(rp, p, dp, 0.7))).all()


def permuted(rp, order):
    """(rowptr, source index of every entry) of the matrix whose rows are rows `order` of rp's"""
    lens = np.diff(rp.astype(np.int64))[order]
    src = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in order] + [np.zeros(0, np.int64)]).astype(np.int64)
    return rowptr_of(lens), src


@pytest.mark.parametrize("name", ["mixed", "powerlaw", "banded"])
def test_permuting_the_rows_permutes_the_bits(sblas, cuda, name):
    import torch
    rp = XN.pattern(name)
    x = XN.scores(rp, seed=4)
    p, dp = gradients(rp, 4)
    ref_f = bits(forward(sblas, torch, cuda, rp, x, 0.5))
    ref_b = bits(backward(sblas, torch, cuda, rp, p, dp, 0.5))
    order = np.random.default_rng(1).permutation(len(rp) - 1)
    rp2, src = permuted(rp, order)
    assert (bits(forward(sblas, torch, cuda, rp2, x[src], 0.5)) == ref_f[src]).all()
    assert (bits(backward(sblas, torch, cuda, rp2, p[src], dp[src], 0.5)) == ref_b[src]).all()


def test_a_row_keeps_its_bits_wherever_it_is_copied(sblas, cuda):
    import torch
    rp = XN.pattern("mixed")
    x = XN.scores(rp, seed=6)
    p, dp = gradients(rp, 6)
    ref_f = bits(forward(sblas, torch, cuda, rp, x, 1.0))
    ref_b = bits(backward(sblas, torch, cuda, rp, p, dp, 1.0))
    nrows = len(rp) - 1
    # inside the same matrix: every row once more, behind the last one
    order = np.concatenate([np.arange(nrows), np.arange(nrows)])
    rp2, src = permuted(rp, order)
    got = bits(forward(sblas, torch, cuda, rp2, x[src], 1.0))
    assert (got == ref_f[src]).all()
    # into another matrix among different neighbours: between the rows of the banded input, one every 700 rows
    other = XN.pattern("banded")
    xo = XN.scores(other, seed=8)
    po, dpo = gradients(other, 8)
    lens, vals, ps, dps, marks = [], [], [], [], []
    k = 0
    for r in range(len(other) - 1):
        if r % 700 == 350 and k < nrows:
            marks.append((sum(lens), k))
            lens.append(rp[k + 1] - rp[k])
            vals.append(x[rp[k]:rp[k + 1]]), ps.append(p[rp[k]:rp[k + 1]]), dps.append(dp[rp[k]:rp[k + 1]])
            k += 1
        lens.append(other[r + 1] - other[r])
        vals.append(xo[other[r]:other[r + 1]]), ps.append(po[other[r]:other[r + 1]]), dps.append(dpo[other[r]:other[r + 1]])
    assert k == nrows
    rp3 = rowptr_of(lens)
    gf = bits(forward(sblas, torch, cuda, rp3, np.concatenate(vals), 1.0))
    gb = bits(backward(sblas, torch, cuda, rp3, np.concatenate(ps), np.concatenate(dps), 1.0))
    for at, k in marks:
        n = rp[k + 1] - rp[k]
        assert (gf[at:at + n] == ref_f[rp[k]:rp[k + 1]]).all(), k
        assert (gb[at:at + n] == ref_b[rp[k]:rp[k + 1]]).all(), k


@pytest.mark.parametrize("name", ["mixed", "powerlaw"])
def test_rebased_row_aligned_blocks_give_the_bits_of_the_whole_call(sblas, cuda, name):
    import torch
    rp = XN.pattern(name)
    x = XN.scores(rp, seed=7)
    p, dp = gradients(rp, 7)
    ref_f = bits(forward(sblas, torch, cuda, rp, x, 0.25))
    ref_b = bits(backward(sblas, torch, cuda, rp, p, dp, 0.25))
    nrows = len(rp) - 1
    cuts = [0, nrows // 5, nrows // 5 + 1, nrows // 2, (3 * nrows) // 4, nrows]
    R = torch.from_numpy(rp).to(cuda)
    X, P, DP = (torch.from_numpy(a).to(cuda) for a in (x, p, dp))
    out = torch.full_like(X, float("nan"))
    dx = torch.full_like(X, float("nan"))
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        e0, e1 = int(rp[r0]), int(rp[r1])
        Rb = (R[r0:r1 + 1] - e0).contiguous()
        sblas.csr_softmax(Rb, X[e0:e1], out[e0:e1], 0.25)
        sblas.csr_softmax_backward(Rb, P[e0:e1], DP[e0:e1], dx[e0:e1], 0.25)
    assert (bits(out.cpu().numpy()) == ref_f).all()
    assert (bits(dx.cpu().numpy()) == ref_b).all()


def test_rows_alone_and_between_two_long_rows_give_the_same_bits(sblas, cuda):
    """Rows of every length 1 .. 130 and of the lengths around every path and cell boundary: alone (in order of length: the
    first eight fit the 8-lane groups) and between two rows of 100 000 entries (other wave tasks, two rows a wave, the long
    kernels at work on the neighbours)."""
    import torch
    lens = list(range(1, 131)) + EDGES
    rp = rowptr_of(lens)
    x = XN.scores(rp, seed=11)
    p, dp = gradients(rp, 11)
    alone_f = bits(forward(sblas, torch, cuda, rp, x, 0.125))
    alone_b = bits(backward(sblas, torch, cuda, rp, p, dp, 0.125))
    rng = np.random.default_rng(0)
    for chunk in (slice(0, 130), slice(130, len(lens))):
        sub = lens[chunk]
        e0, e1 = int(rp[chunk.start]), int(rp[chunk.stop])
        rp2 = rowptr_of([LONG] + sub + [LONG])
        pad = lambda a: np.concatenate([rng.uniform(-1, 1, LONG), a, rng.uniform(-1, 1, LONG)])
        xf = pad(x[e0:e1])
        got = bits(forward(sblas, torch, cuda, rp2, xf, 0.125))
        assert (got[LONG:LONG + e1 - e0] == alone_f[e0:e1]).all()
        pl = np.full(LONG, 1.0 / LONG)
        pf, dpf = np.concatenate([pl, p[e0:e1], pl]), pad(dp[e0:e1])
        got = bits(backward(sblas, torch, cuda, rp2, pf, dpf, 0.125))
        assert (got[LONG:LONG + e1 - e0] == alone_b[e0:e1]).all()


@pytest.mark.parametrize("name", ["mixed", "powerlaw"])
def test_in_place_and_out_of_place_agree(sblas, cuda, name):
    import torch
    rp = XN.pattern(name)
    x = XN.scores(rp, seed=12)
    p, dp = gradients(rp, 12)
    assert (bits(forward(sblas, torch, cuda, rp, x, 2.0, inplace=True)) == bits(forward(sblas, torch, cuda, rp, x, 2.0))).all()
    a, b = backward(sblas, torch, cuda, rp, p, dp, 2.0, inplace=True), backward(sblas, torch, cuda, rp, p, dp, 2.0)
    assert (bits(a) == bits(b)).all()                       # dx aliasing dp


def test_repeated_calls_and_graph_replay_give_the_same_bits(sblas, cuda):
    import torch
    rp = XN.pattern("mixed")
    nnz, rows = int(rp[-1]), len(rp) - 1
    x = XN.scores(rp, seed=13)
    first = bits(forward(sblas, torch, cuda, rp, x, 0.5))
    for _ in range(4):
        assert (bits(forward(sblas, torch, cuda, rp, x, 0.5)) == first).all()
    R = torch.from_numpy(rp).to(cuda)
    X = torch.from_numpy(x).to(cuda)
    DP = torch.zeros_like(X)
    out, dx = torch.zeros_like(X), torch.zeros_like(X)
    ws = torch.empty((sblas.csr_softmax_workspace_bytes(rows, nnz) + 7) // 8, dtype=torch.float64, device=cuda)
    assert ws.numel() > 0

    def both():
        sblas.csr_softmax(R, X, out, 0.5, workspace=ws)
        sblas.csr_softmax_backward(R, out, DP, dx, 0.5, workspace=ws)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()                                               # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    for step in range(3):
        xn = XN.scores(rp, seed=50 + step)
        dpn = np.random.default_rng(step).uniform(-1, 1, nnz)
        X.copy_(torch.from_numpy(xn).to(cuda))
        DP.copy_(torch.from_numpy(dpn).to(cuda))
        graph.replay()
        torch.cuda.synchronize()
        eager = forward(sblas, torch, cuda, rp, xn, 0.5)
        assert (bits(out.cpu().numpy()) == bits(eager)).all(), step
        assert (bits(dx.cpu().numpy()) == bits(backward(sblas, torch, cuda, rp, eager, dpn, 0.5))).all(), step


# ---- 3. IEEE classes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, -0.5, 0.0])
def test_ieee_classes_and_padding_is_never_read(sblas, cuda, scale):
    import torch
    inf, nan = np.inf, np.nan
    rng = np.random.default_rng(3)
    # hand-written rows, then every row of the mixed pattern with a special value planted by kind
    hand = [[1.0, nan, 2.0], [1.0, -inf, 3.0], [1.0, inf, -inf], [-inf, -inf], [-inf], [inf], [nan], [0.0, -800.0], [],
            [inf, inf, 1.0], [5.0]]
    mixed = XN.pattern("mixed")
    lens = [len(r) for r in hand] + list(np.diff(mixed))
    rp = rowptr_of(lens)
    x = rng.uniform(-20, 20, int(rp[-1]))
    x[:rp[len(hand)]] = [v for r in hand for v in r]
    kinds = [None, nan, -inf, inf, "all-neg-inf", "nan-last", "neg-inf-many"]
    for i, r in enumerate(range(len(hand), len(lens))):
        lo, hi = rp[r], rp[r + 1]
        kind = kinds[i % len(kinds)]
        if hi == lo or kind is None:
            continue
        if kind == "all-neg-inf":
            x[lo:hi] = -inf
        elif kind == "nan-last":
            x[hi - 1] = nan
        elif kind == "neg-inf-many":
            x[lo:hi][rng.random(hi - lo) < 0.5] = -inf
            x[lo] = 1.0
        else:
            x[lo + (hi - lo) // 2] = kind
    want = XN.predict_class(rp, x, scale)
    assert {XN.NAN, XN.ZERO, XN.FINITE} <= set(want) or scale == 0.0
    R = torch.from_numpy(rp).to(cuda)
    for lead in (2, 3):                                      # 16-byte aligned values, and 8 bytes off
        buf = torch.full((lead + len(x) + 5,), nan, dtype=torch.float64, device=cuda)
        xv = buf[lead:lead + len(x)]
        xv.copy_(torch.from_numpy(x).to(cuda))
        obuf = torch.full_like(buf, -7.0)
        sblas.csr_softmax(R, xv, obuf[lead:lead + len(x)], scale)
        got = obuf.cpu().numpy()
        assert (got[:lead] == -7.0).all() and (got[lead + len(x):] == -7.0).all()      # nothing written outside
        bad = XN.class_mismatches(want, got[lead:lead + len(x)])
        assert len(bad) == 0, "%d entries in the wrong class, first %d (row %d): want %d got %r" % (
            len(bad), bad[0], np.searchsorted(rp, bad[0], "right") - 1, want[bad[0]], got[lead + bad[0]])
        # the NaN padding reached no output: the finite rows equal those of a call on an unpadded copy
        plain = forward(sblas, torch, cuda, rp, x, scale)
        assert (bits(plain)[want != XN.NAN] == bits(got[lead:lead + len(x)])[want != XN.NAN]).all()
    # backward: NaN padding around p and dp reaches nothing
    p, dp = gradients(rp, 1)
    ref = bits(backward(sblas, torch, cuda, rp, p, dp, 0.5))
    pb = torch.full((3 + len(p) + 3,), nan, dtype=torch.float64, device=cuda)
    db = torch.full_like(pb, nan)
    pb[3:3 + len(p)].copy_(torch.from_numpy(p).to(cuda))
    db[3:3 + len(p)].copy_(torch.from_numpy(dp).to(cuda))
    dx = torch.empty(len(p), dtype=torch.float64, device=cuda)
    sblas.csr_softmax_backward(R, pb[3:3 + len(p)], db[3:3 + len(p)], dx, 0.5)
    assert (bits(dx.cpu().numpy()) == ref).all() and np.isfinite(dx.cpu().numpy()).all()


# ---- 4. SBLAS_VALIDATE ---------------------------------------------------------------------------------------------
def test_validate_refuses_a_row_pointer_that_descends_and_writes_nothing(sblas, cuda, monkeypatch):
    import torch
    rp = XN.pattern("mixed")
    x = XN.scores(rp, seed=1)
    bad = rp.copy()
    bad[5], bad[6] = bad[6] + 3, bad[5]
    assert (np.diff(bad) < 0).any() and bad[-1] == rp[-1]
    X = torch.from_numpy(x).to(cuda)
    out = torch.full_like(X, -7.0)
    monkeypatch.setenv("SBLAS_VALIDATE", "1")
    sblas.reload_env()
    try:
        for wrong in (bad, np.concatenate([rp[:-1], [rp[-1] - 1]]).astype(np.int32)):     # descending; not ending at nnz
            with pytest.raises(sblas.SblasError, match="code 1"):
                sblas.csr_softmax(torch.from_numpy(wrong).to(cuda), X, out, 1.0)
            with pytest.raises(sblas.SblasError, match="code 1"):
                sblas.csr_softmax_backward(torch.from_numpy(wrong).to(cuda), X, X, out, 1.0)
            torch.cuda.synchronize()
            assert (out == -7.0).all()
        sblas.csr_softmax(torch.from_numpy(rp).to(cuda), X, out, 1.0)
        assert (bits(out.cpu().numpy()) == bits(forward(sblas, torch, cuda, rp, x, 1.0))).all()
    finally:
        monkeypatch.delenv("SBLAS_VALIDATE")
        sblas.reload_env()


# ---- 5. autograd ---------------------------------------------------------------------------------------------------
def attention_pattern():
    """12 x 9: unsorted columns, duplicates, empty rows (rows 3 and 11)"""
    rng = np.random.default_rng(0)
    parts = []
    for r in range(12):
        if r in (3, 11):
            parts.append(np.zeros(0, np.int64))
            continue
        c = rng.integers(0, 9, int(rng.integers(1, 6)))
        parts.append(np.concatenate([c, c[:1]]) if r % 4 == 0 else c)
    return 12, 9, rowptr_of([len(q) for q in parts]), np.concatenate(parts).astype(np.int32)


def operator(torch, dev, rows, cols, rp, ci, **kw):
    from sblas_amd.autograd import CsrOperator
    return CsrOperator(rows, cols, torch.from_numpy(rp).to(dev), torch.from_numpy(ci).to(dev), **kw)


def rand(torch, dev, g, *shape):
    return (torch.rand(*shape, dtype=torch.float64, generator=g) * 2 - 1).to(dev).requires_grad_()


def test_gradcheck_softmax(sblas, cuda):
    import torch
    rows, cols, rp, ci = attention_pattern()
    op = operator(torch, cuda, rows, cols, rp, ci)
    g = torch.Generator(device="cpu").manual_seed(1)
    val = rand(torch, cuda, g, len(ci))
    for scale in (1.0, 0.35, -2.0):
        assert torch.autograd.gradcheck(lambda v: op.softmax(v, scale=scale), (val,), nondet_tol=0)
    # a longer pattern: rows that take the register, pass and long paths
    rp2 = rowptr_of([70, 0, 600, 5000, 3])
    op2 = operator(torch, cuda, 5, 8, rp2, np.zeros(int(rp2[-1]), np.int32))
    v2 = rand(torch, cuda, g, int(rp2[-1]))
    w = rand(torch, cuda, g, int(rp2[-1])).detach()
    op2.softmax(v2, scale=3.0).mul(w).sum().backward()
    p = XN.numpy_forward(rp2, v2.detach().cpu().numpy(), 3.0)
    want = XN.numpy_backward(rp2, p, w.cpu().numpy(), 3.0)
    assert np.allclose(v2.grad.cpu().numpy(), want, rtol=1e-11, atol=1e-15)


@pytest.mark.parametrize("k", [1, 5, 16])
def test_gradcheck_sddmm(sblas, cuda, k):
    import torch
    rows, cols, rp, ci = attention_pattern()
    op = operator(torch, cuda, rows, cols, rp, ci, n=16 if k == 16 else 0)          # k == n: the planned SpMM computes dX
    g = torch.Generator(device="cpu").manual_seed(k)
    X, Y = rand(torch, cuda, g, rows, k), rand(torch, cuda, g, cols, k)
    Xc, Yc = X.detach(), Y.detach()
    assert torch.autograd.gradcheck(lambda x: op.sddmm(x, Yc), (X,), nondet_tol=0)            # X alone
    assert op.transpose_plan is None                                                         # dY was not asked for
    assert torch.autograd.gradcheck(lambda y: op.sddmm(Xc, y), (Y,), nondet_tol=0)            # Y alone
    assert op.transpose_plan is not None
    assert torch.autograd.gradcheck(op.sddmm, (X, Y), nondet_tol=0)                          # both
    Xt, Yt = rand(torch, cuda, g, k, rows), rand(torch, cuda, g, k, cols)                    # transposed views
    assert torch.autograd.gradcheck(lambda x, y: op.sddmm(x.t(), y.t()), (Xt, Yt), nondet_tol=0)
    assert torch.autograd.gradcheck(lambda x, y: op.sddmm(x.t(), y), (Xt, Y), nondet_tol=0)


def test_sddmm_honours_needs_input_grad(sblas, cuda):
    import torch
    rows, cols, rp, ci = attention_pattern()
    op = operator(torch, cuda, rows, cols, rp, ci)
    g = torch.Generator(device="cpu").manual_seed(0)
    X, Y = rand(torch, cuda, g, rows, 4), rand(torch, cuda, g, cols, 4).detach()
    op.sddmm(X, Y).sum().backward()                                              # an expanded incoming gradient
    assert X.grad is not None and Y.grad is None and op.transpose_plan is None
    r = torch.from_numpy(np.repeat(np.arange(rows), np.diff(rp))).to(cuda)
    want = torch.zeros(rows, 4, dtype=torch.float64, device=cuda).index_add_(0, r, Y[torch.from_numpy(ci).long().to(cuda)])
    assert torch.allclose(X.grad, want, rtol=1e-13, atol=1e-15)
    Y2 = Y.clone().requires_grad_()
    op.sddmm(X.detach(), Y2).sum().backward()
    assert Y2.grad is not None and op.transpose_plan is not None
    op.sddmm(X.detach(), Y2).mul(2.0).sum().backward()                           # the plan is refreshed, not rebuilt
    c = torch.from_numpy(ci).long().to(cuda)
    wantY = torch.zeros(cols, 4, dtype=torch.float64, device=cuda).index_add_(0, c, X.detach()[r])
    assert torch.allclose(Y2.grad, 3.0 * wantY, rtol=1e-13, atol=1e-15)


def test_gradcheck_attention(sblas, cuda):
    """O = A(softmax(scale * sddmm(Q, K))) V in Q, K and V, on a pattern with empty rows and duplicates"""
    import torch
    rows, cols, rp, ci = attention_pattern()
    d = 6
    op = operator(torch, cuda, rows, cols, rp, ci, n=d)
    g = torch.Generator(device="cpu").manual_seed(7)
    Q, K, V = rand(torch, cuda, g, rows, d), rand(torch, cuda, g, cols, d), rand(torch, cuda, g, cols, d)

    def attention(q, k, v):
        return op.matmul(op.softmax(op.sddmm(q, k), scale=d ** -0.5), v)

    assert torch.autograd.gradcheck(attention, (Q, K, V), nondet_tol=0)
    # the values against a dense restatement
    O = attention(Q, K, V).detach()
    S = (Q.detach() @ K.detach().t()) * d ** -0.5
    want = torch.zeros_like(O)
    for r in range(rows):
        cs = torch.from_numpy(ci[rp[r]:rp[r + 1]].astype(np.int64)).to(cuda)
        if len(cs):
            want[r] = torch.softmax(S[r, cs], 0) @ V.detach()[cs]
    assert torch.allclose(O, want, rtol=1e-12, atol=1e-14)
