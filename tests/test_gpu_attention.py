"""Fused attention on a CSR pattern on the GPU (sblas_hip_csr_attention_f64_i32 and its backward through sblas_amd, and
CsrOperator.attention): contract (B) -- the probabilities and score gradients are the composition's bit for bit --, O and
dQ within the dot-product bound of attention_numerics against the exact sum over the GPU's own P / dS, contract (A) -- the
bits of a row of O / dQ follow the row, not its place --, the IEEE classes, autograd and the memory the forward keeps."""
import numpy as np
import pytest

import attention_numerics as AN

pytestmark = pytest.mark.gpu

LONG = 100000                    # the neighbours of the embedding test
NAMES = ["small", "edges", "big"]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def up(torch, dev, a):
    return torch.from_numpy(np.array(a, order="C")).to(dev)          # a copy: the shared patterns are read-only


_structures = {}


def structure(torch, dev, name):
    """the pattern on the device, uploaded once"""
    if name not in _structures:
        rows, cols, rp, ci = AN.pattern(name)
        _structures[name] = (rows, cols, up(torch, dev, rp), up(torch, dev, ci))
    return _structures[name]


def fused(S, torch, A, Q, K, V, dO, scale, want=("dQ", "P", "dS"), O=None, dQ=None):
    """forward and backward through the tensor-level calls; every output starts as NaN"""
    rows, cols, R, Ci = A
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=R.device)
    O = nan(rows, V.shape[1]) if O is None else O
    m, z = nan(rows), nan(rows)
    S.csr_attention(A, Q, K, V, scale, O, m, z)
    dQ = (nan(rows, Q.shape[1]) if dQ is None else dQ) if "dQ" in want else None
    P = nan(Ci.numel()) if "P" in want else None
    dS = nan(Ci.numel()) if "dS" in want else None
    S.csr_attention_backward(A, Q, K, V, dO, m, z, scale, dQ, P, dS)
    return dict(O=O, m=m, z=z, dQ=dQ, P=P, dS=dS)


def composition(S, torch, A, Q, K, V, dO, scale):
    """the library's own chain: SDDMM, softmax, SDDMM of (dO, V), softmax backward"""
    rows, cols, R, Ci = A
    new = lambda: torch.empty(Ci.numel(), dtype=torch.float64, device=R.device)
    Sc, dP = new(), new()
    S.sddmm_tensor(A, Q, K, Sc)
    P = S.csr_softmax(R, Sc, None, scale)
    S.sddmm_tensor(A, dO, V, dP)
    dS = S.csr_softmax_backward(R, P, dP, None, scale)
    return dict(S=Sc, P=P, dP=dP, dS=dS)


def run_np(S, torch, dev, rows, cols, rp, ci, Q, K, V, dO, scale):
    """(bits of O, bits of dQ) of numpy inputs"""
    A = (rows, cols, up(torch, dev, np.asarray(rp, np.int32)), up(torch, dev, np.asarray(ci, np.int32)))
    out = fused(S, torch, A, up(torch, dev, Q), up(torch, dev, K), up(torch, dev, V), up(torch, dev, dO), scale, want=("dQ",))
    return bits(out["O"].cpu().numpy()), bits(out["dQ"].cpu().numpy())


# ---- 1. contract (B): P, dS and the row max are the composition's ----------------------------------------------------
@pytest.mark.parametrize("d,dv", AN.WIDTHS)
@pytest.mark.parametrize("name", NAMES)
def test_probabilities_and_score_gradients_equal_the_composition_bit_for_bit(sblas, cuda, name, d, dv):
    import torch
    A = structure(torch, cuda, name)
    rows, cols, rp, ci = AN.pattern(name)
    lens = np.diff(rp.astype(np.int64))
    Q, K, V, dO = (up(torch, cuda, x) for x in AN.operands(rows, cols, d, dv))
    for scale in AN.SCALES:
        got = fused(sblas, torch, A, Q, K, V, dO, scale)
        ref = composition(sblas, torch, A, Q, K, V, dO, scale)
        assert (bits(got["P"].cpu().numpy()) == bits(ref["P"].cpu().numpy())).all(), scale
        assert (bits(got["dS"].cpu().numpy()) == bits(ref["dS"].cpu().numpy())).all(), scale
        t = scale * ref["S"].cpu().numpy()
        want = np.full(rows, -np.inf)
        want[lens > 0] = np.maximum.reduceat(t, rp[:-1][lens > 0].astype(np.int64))
        m, z = got["m"].cpu().numpy(), got["z"].cpu().numpy()
        assert (m == want).all(), scale
        assert (z[lens > 0] >= 1.0).all() and (bits(z[lens == 0]) == 0).all()          # exp(0) = 1 is among the terms


# ---- 2. O and dQ within the derived bound -----------------------------------------------------------------------------
@pytest.mark.parametrize("d,dv", AN.WIDTHS)
@pytest.mark.parametrize("name", NAMES)
def test_output_and_query_gradient_within_the_dot_product_bound(sblas, cuda, name, d, dv):
    """Reference: the exact sum of the GPU's own P[e] * V[c(e), c] (dS[e] * K[c(e), c]) over whole sampled rows and the
    longest one; bound: attention_numerics' docstring."""
    import torch
    A = structure(torch, cuda, name)
    rows, cols, rp, ci = AN.pattern(name)
    Qn, Kn, Vn, dOn = AN.operands(rows, cols, d, dv, seed=1)
    got = fused(sblas, torch, A, up(torch, cuda, Qn), up(torch, cuda, Kn), up(torch, cuda, Vn), up(torch, cuda, dOn), 0.125)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    sample = AN.sample_rows(rp, count=4)
    res_o = AN.check_rows(got["O"], rp, ci, got["P"], Vn, sample)
    res_q = AN.check_rows(got["dQ"], rp, ci, got["dS"], Kn, sample)
    print("%s d=%d dv=%d: worst error / bound O %.3g at %s, dQ %.3g at %s (%d + %d outputs)" %
          (name, d, dv, res_o["worst"], res_o["where"], res_q["worst"], res_q["where"], res_o["outputs"], res_q["outputs"]))
    assert res_o["ok"], res_o
    assert res_q["ok"], res_q
    lens = np.diff(rp.astype(np.int64))
    assert (bits(got["O"][lens == 0]) == 0).all() and (bits(got["dQ"][lens == 0]) == 0).all()      # empty rows: +0
    assert np.isfinite(got["O"]).all() and np.isfinite(got["dQ"]).all()


# ---- 3. contract (A): the bits follow the row -------------------------------------------------------------------------
A_WIDTHS = [(64, 64), (5, 3)]


@pytest.mark.parametrize("d,dv", A_WIDTHS)
def test_permuting_the_rows_permutes_the_bits(sblas, cuda, d, dv):
    import torch
    rows, cols, rp, ci = AN.pattern("edges")
    Q, K, V, dO = AN.operands(rows, cols, d, dv, seed=2)
    o, q = run_np(sblas, torch, cuda, rows, cols, rp, ci, Q, K, V, dO, 0.125)
    order = np.random.default_rng(3).permutation(rows)
    lens = np.diff(rp.astype(np.int64))
    rp2 = AN.rowptr_of(lens[order])
    ci2 = np.concatenate([ci[rp[r]:rp[r + 1]] for r in order])
    o2, q2 = run_np(sblas, torch, cuda, rows, cols, rp2, ci2, Q[order], K, V, dO[order], 0.125)
    assert (o2 == o[order]).all() and (q2 == q[order]).all()


@pytest.mark.parametrize("d,dv", A_WIDTHS)
def test_a_row_alone_between_two_long_rows_and_in_a_rebased_block_gives_the_same_bits(sblas, cuda, d, dv):
    import torch
    rows, cols, rp, ci = AN.pattern("edges")
    Q, K, V, dO = AN.operands(rows, cols, d, dv, seed=4)
    o, q = run_np(sblas, torch, cuda, rows, cols, rp, ci, Q, K, V, dO, -0.3)
    # alone: a matrix of one row (other workgroup boundaries, block positions and, for the long rows, other slots)
    for r in range(rows):
        lo, hi = int(rp[r]), int(rp[r + 1])
        o1, q1 = run_np(sblas, torch, cuda, 1, cols, [0, hi - lo], ci[lo:hi], Q[r:r + 1], K, V, dO[r:r + 1], -0.3)
        assert (o1[0] == o[r]).all() and (q1[0] == q[r]).all(), (r, hi - lo)
    # between two rows of 10^5 entries: the long kernels at work on the neighbours, every supercell in another block
    rng = np.random.default_rng(5)
    lens = np.diff(rp.astype(np.int64))
    rp2 = AN.rowptr_of([LONG] + list(lens) + [LONG])
    ci2 = np.concatenate([rng.integers(0, cols, LONG), ci, rng.integers(0, cols, LONG)]).astype(np.int32)
    wrap = lambda X: np.concatenate([rng.uniform(-1, 1, (1, X.shape[1])), X, rng.uniform(-1, 1, (1, X.shape[1]))])
    o2, q2 = run_np(sblas, torch, cuda, rows + 2, cols, rp2, ci2, wrap(Q), K, V, wrap(dO), -0.3)
    assert (o2[1:-1] == o).all() and (q2[1:-1] == q).all()
    # a row-aligned block, row pointers re-based, the operands advanced to its first row
    r0, r1 = 9, 27
    e0, e1 = int(rp[r0]), int(rp[r1])
    o3, q3 = run_np(sblas, torch, cuda, r1 - r0, cols, rp[r0:r1 + 1] - e0, ci[e0:e1], Q[r0:r1], K, V, dO[r0:r1], -0.3)
    assert (o3 == o[r0:r1]).all() and (q3 == q[r0:r1]).all()


@pytest.mark.parametrize("d,dv", A_WIDTHS)
def test_leading_dimension_padding_and_alignment_do_not_change_the_bits(sblas, cuda, d, dv):
    import torch
    rows, cols, rp, ci = AN.pattern("edges")
    A = structure(torch, cuda, "edges")
    Qn, Kn, Vn, dOn = AN.operands(rows, cols, d, dv, seed=6)
    o, q = run_np(sblas, torch, cuda, rows, cols, rp, ci, Qn, Kn, Vn, dOn, 0.125)

    def padded(X, before, after, fill):
        """X as a view into a wider buffer full of `fill`: `before` columns in front (a base 8 bytes off 16-byte
        alignment when odd), `after` behind"""
        buf = torch.full((X.shape[0], before + X.shape[1] + after), fill, dtype=torch.float64, device=cuda)
        view = buf[:, before:before + X.shape[1]]
        view.copy_(up(torch, cuda, X))
        return buf, view

    for before, after, fill in ((0, 3, float("nan")), (0, 2, float("inf")), (1, 0, float("nan")), (1, 2, float("-inf"))):
        (_, Q), (_, K), (_, V), (_, dO) = (padded(X, before, after, fill) for X in (Qn, Kn, Vn, dOn))
        obuf, O = padded(np.zeros((rows, dv)), before, after, fill)
        qbuf, dQ = padded(np.zeros((rows, d)), before, after, fill)
        assert (Q.data_ptr() % 16 == 8) == (before == 1)
        got = fused(sblas, torch, A, Q, K, V, dO, 0.125, want=("dQ",), O=O, dQ=dQ)
        assert (bits(got["O"].cpu().numpy()) == o).all() and (bits(got["dQ"].cpu().numpy()) == q).all(), (before, after)
        for buf, w in ((obuf, dv), (qbuf, d)):                           # the padding of the outputs is not written
            pad = torch.cat([buf[:, :before], buf[:, before + w:]], dim=1)
            assert bool(torch.isnan(pad).all() if fill != fill else (pad == fill).all())


@pytest.mark.parametrize("d,dv", A_WIDTHS)
def test_repeated_calls_and_graph_replay_give_the_same_bits(sblas, cuda, d, dv):
    import torch
    rows, cols, rp, ci = AN.pattern("edges")
    A = structure(torch, cuda, "edges")
    nnz = int(rp[-1])
    Qn, Kn, Vn, dOn = AN.operands(rows, cols, d, dv, seed=7)
    first = run_np(sblas, torch, cuda, rows, cols, rp, ci, Qn, Kn, Vn, dOn, 0.5)
    for _ in range(3):
        again = run_np(sblas, torch, cuda, rows, cols, rp, ci, Qn, Kn, Vn, dOn, 0.5)
        assert (again[0] == first[0]).all() and (again[1] == first[1]).all()
    Q, K, V, dO = (up(torch, cuda, x) for x in (Qn, Kn, Vn, dOn))
    new = lambda *shape: torch.zeros(*shape, dtype=torch.float64, device=cuda)
    O, m, z, dQ, P, dS = new(rows, dv), new(rows), new(rows), new(rows, d), new(nnz), new(nnz)
    ws = torch.empty((sblas.csr_attention_workspace_bytes(rows, nnz, d, dv) + 7) // 8, dtype=torch.float64, device=cuda)
    assert ws.numel() > 0

    def both():
        sblas.csr_attention(A, Q, K, V, 0.5, O, m, z, workspace=ws)
        sblas.csr_attention_backward(A, Q, K, V, dO, m, z, 0.5, dQ, P, dS, workspace=ws)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()                                               # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    for step in range(2):
        Qs, Ks, Vs, dOs = AN.operands(rows, cols, d, dv, seed=50 + step)
        for t, x in ((Q, Qs), (K, Ks), (V, Vs), (dO, dOs)):
            t.copy_(up(torch, cuda, x))
        graph.replay()
        torch.cuda.synchronize()
        eager = fused(sblas, torch, A, Q, K, V, dO, 0.5)
        for name, t in (("O", O), ("dQ", dQ), ("P", P), ("dS", dS), ("m", m), ("z", z)):
            assert (bits(t.cpu().numpy()) == bits(eager[name].cpu().numpy())).all(), (step, name)


# ---- 4. IEEE classes ---------------------------------------------------------------------------------------------------
def one_row_pattern(length=700, cols=50):
    return 1, cols, AN.rowptr_of([length]), np.random.default_rng(8).integers(0, cols, length).astype(np.int32)


@pytest.mark.parametrize("scale", [0.5, 0.0])
@pytest.mark.parametrize("which", ["small", "row700"])
def test_ieee_classes_are_the_compositions(sblas, cuda, which, scale):
    import torch
    rows, cols, rp, ci = AN.pattern("small") if which == "small" else one_row_pattern()
    A = (rows, cols, up(torch, cuda, rp), up(torch, cuda, ci))
    d, dv = 5, 3
    Qn, Kn, Vn, dOn = AN.operands(rows, cols, d, dv, seed=9)
    lens = np.diff(rp.astype(np.int64))
    row = int(np.flatnonzero(lens > 0)[0])
    col = int(ci[rp[row]])                                   # a row of K / V that the first non-empty row reads
    seen = set()
    for operand, (i, j) in (("Q", (row, 0)), ("K", (col, d - 1)), ("V", (col, dv - 1))):
        for value in (np.nan, np.inf, -np.inf):
            X = dict(Q=Qn.copy(), K=Kn.copy(), V=Vn.copy())
            X[operand][i, j] = value
            Q, K, V, dO = (up(torch, cuda, x) for x in (X["Q"], X["K"], X["V"], dOn))
            got = fused(sblas, torch, A, Q, K, V, dO, scale, want=("P",))
            ref = composition(sblas, torch, A, Q, K, V, dO, scale)
            Oc = torch.full((rows, dv), float("nan"), dtype=torch.float64, device=cuda)
            sblas.spmm_tensor((rows, cols, A[2], A[3], ref["P"]), V, Oc, 1.0, 0.0)
            have, want = AN.classes(got["O"].cpu().numpy()), AN.classes(Oc.cpu().numpy())
            assert (have == want).all(), (operand, value, have.tolist(), want.tolist())
            seen |= set(have[row].tolist())
            m, z, O = got["m"].cpu().numpy(), got["z"].cpu().numpy(), got["O"].cpu().numpy()
            assert (m[lens == 0] == -np.inf).all() and (bits(z[lens == 0]) == 0).all() and (bits(O[lens == 0]) == 0).all()
    assert 1 in seen                                         # the planted values reached the output: a NaN at least


# ---- 5. autograd -------------------------------------------------------------------------------------------------------
def operator(torch, dev, name, **kw):
    from sblas_amd.autograd import CsrOperator
    rows, cols, R, Ci = structure(torch, dev, name)
    return CsrOperator(rows, cols, R, Ci, **kw)


def leaves(torch, dev, rows, cols, d, dv, seed, grad=(True, True, True)):
    Q, K, V, dO = AN.operands(rows, cols, d, dv, seed=seed)
    return [up(torch, dev, x).requires_grad_(g) for x, g in zip((Q, K, V), grad)] + [up(torch, dev, dO)]


@pytest.mark.parametrize("d,dv", [(5, 3), (8, 8)])
def test_gradcheck_attention(sblas, cuda, d, dv, monkeypatch):
    import torch
    import sblas_amd.autograd as AG
    rows, cols, rp, ci = AN.pattern("small")
    op = operator(torch, cuda, "small")
    Q, K, V, _ = leaves(torch, cuda, rows, cols, d, dv, 10)
    assert torch.autograd.gradcheck(lambda q, k, v: op.attention(q, k, v, 0.7), (Q, K, V), nondet_tol=0)
    asked = []
    real = AG.csr_attention_backward
    monkeypatch.setattr(AG, "csr_attention_backward",
                        lambda A, q, k, v, dO, m, z, scale, dQ, P, dS, **kw: (asked.append((dQ is not None, P is not None, dS is not None)),
                                                                            real(A, q, k, v, dO, m, z, scale, dQ, P, dS, **kw))[1])
    for only in range(3):
        grad = tuple(i == only for i in range(3))
        q, k, v, dO = leaves(torch, cuda, rows, cols, d, dv, 11 + only, grad)
        free = [t for t in (q, k, v) if t.requires_grad]
        fn = lambda x: op.attention(*[x if t.requires_grad else t for t in (q, k, v)], 0.7)
        assert torch.autograd.gradcheck(fn, tuple(free), nondet_tol=0)
        del asked[:]
        O = op.attention(q, k, v, 0.7)
        O.backward(dO)
        assert [t.grad is not None for t in (q, k, v)] == list(grad)
        # dQ comes from the kernel, dV needs P, dK needs dS: nothing else is allocated
        assert asked == [(grad[0], grad[2], grad[1])]
    # no gradient wanted: nothing is saved for a backward
    q, k, v, _ = leaves(torch, cuda, rows, cols, d, dv, 20, (False, False, False))
    assert op.attention(q, k, v).grad_fn is None


def test_big_case_gradients_and_the_fallback(sblas, cuda):
    """`big` at (64, 64): dK and dV are the composition's bit for bit (same operator, same TransposePlan and, by (B), the
    same dS / P); O and dQ meet the bound.  d = 200 runs the composition inside attention: its bits throughout."""
    import torch
    rows, cols, rp, ci = AN.pattern("big")
    op = operator(torch, cuda, "big")
    Q, K, V, dO = leaves(torch, cuda, rows, cols, 64, 64, 30)
    O = op.attention(Q, K, V, 0.125)
    dQ, dK, dV = torch.autograd.grad(O, (Q, K, V), dO)
    Oc = op.matmul(op.softmax(op.sddmm(Q, K), 0.125), V)
    dQc, dKc, dVc = torch.autograd.grad(Oc, (Q, K, V), dO)
    assert (bits(dK.cpu().numpy()) == bits(dKc.cpu().numpy())).all()
    assert (bits(dV.cpu().numpy()) == bits(dVc.cpu().numpy())).all()
    A = structure(torch, cuda, "big")
    raw = fused(sblas, torch, A, Q.detach(), K.detach(), V.detach(), dO, 0.125)
    assert (bits(raw["O"].cpu().numpy()) == bits(O.detach().cpu().numpy())).all()
    assert (bits(raw["dQ"].cpu().numpy()) == bits(dQ.cpu().numpy())).all()
    sample = AN.sample_rows(rp, count=4, seed=1)
    res_o = AN.check_rows(O.detach().cpu().numpy(), rp, ci, raw["P"].cpu().numpy(), V.detach().cpu().numpy(), sample)
    res_q = AN.check_rows(dQ.cpu().numpy(), rp, ci, raw["dS"].cpu().numpy(), K.detach().cpu().numpy(), sample)
    print("big (64, 64) through autograd: worst error / bound O %.3g, dQ %.3g" % (res_o["worst"], res_q["worst"]))
    assert res_o["ok"] and res_q["ok"], (res_o, res_q)
    # the fallback
    rows, cols, rp, ci = AN.pattern("small")
    op = operator(torch, cuda, "small")
    rng = np.random.default_rng(31)
    q, k, v = (up(torch, cuda, rng.uniform(-1, 1, s)).requires_grad_() for s in ((rows, 200), (cols, 200), (cols, 3)))
    g = up(torch, cuda, rng.uniform(-1, 1, (rows, 3)))
    a = op.attention(q, k, v, 0.1)
    b = op.matmul(op.softmax(op.sddmm(q, k), 0.1), v)
    for x, y in zip((a,) + torch.autograd.grad(a, (q, k, v), g), (b,) + torch.autograd.grad(b, (q, k, v), g)):
        assert (bits(x.detach().cpu().numpy()) == bits(y.detach().cpu().numpy())).all()
    # a column-major V takes it too
    vt = up(torch, cuda, rng.uniform(-1, 1, (3, cols))).requires_grad_()
    q8, k8 = q[:, :8].detach().contiguous(), k[:, :8].detach().contiguous()
    a = op.attention(q8, k8, vt.t(), 0.1)
    b = op.matmul(op.softmax(op.sddmm(q8, k8), 0.1), vt.t())
    assert (bits(a.detach().cpu().numpy()) == bits(b.detach().cpu().numpy())).all()


def test_attention_rejects_wrong_shapes_dtypes_and_devices(sblas, cuda):
    """CsrOperator.attention and the tensor-level calls on GPU tensors: every refusal is an SblasError that names the
    operand, on the fused route (d <= 128) and on the composition's (d > 128) alike, and nothing is launched."""
    import torch
    rows, cols, rp, ci = AN.pattern("small")
    op = operator(torch, cuda, "small")
    A = structure(torch, cuda, "small")
    E = sblas.SblasError
    Z = lambda *shape, **kw: torch.zeros(*shape, dtype=kw.get("dtype", torch.float64), device=kw.get("device", cuda))
    for d in (8, 200):                                               # fused, and the fallback
        Q, K, V = Z(rows, d), Z(cols, d), Z(cols, 3)
        assert op.attention(Q, K, V).shape == (rows, 3)               # the well-formed call runs
        for what, bad in (("Q", Z(rows + 1, d)), ("K", Z(cols + 1, d)), ("V", Z(cols - 1, 3))):      # a wrong row count
            args = dict(Q=Q, K=K, V=V)
            args[what] = bad
            with pytest.raises(E, match="%s must have 2 dimension" % what):
                op.attention(args["Q"], args["K"], args["V"])
        for what in ("Q", "K", "V"):
            args = dict(Q=Q, K=K, V=V)
            args[what] = args[what].float()                          # float32
            with pytest.raises(E, match="%s must be float64" % what):
                op.attention(args["Q"], args["K"], args["V"])
            args = dict(Q=Q, K=K, V=V)
            args[what] = args[what][:, 0]                            # 1-D
            with pytest.raises(E, match="%s must have 2 dimension" % what):
                op.attention(args["Q"], args["K"], args["V"])
            args = dict(Q=Q, K=K, V=V)
            args[what] = args[what].cpu()                            # the wrong device
            with pytest.raises(E, match="%s must be a GPU tensor" % what):
                op.attention(args["Q"], args["K"], args["V"])
        with pytest.raises(E, match="Q and K must have the same number of columns, got %d and %d" % (d, d - 1)):
            op.attention(Q, Z(cols, d - 1), V)                       # the widths of Q and K differ
        with pytest.raises(E, match="Q and K must have the same number of columns"):
            op.attention(Z(rows, d + 1), K, V)
        with pytest.raises(E, match="strides"):
            op.attention(Z(rows, 2 * d)[:, ::2], K, V)               # a view no kernel reads
    with pytest.raises(E, match="Q and K must have the same number of columns, got 8 and 200"):
        op.attention(Z(rows, 8), Z(cols, 200), Z(cols, 3))           # one side of the limit each
    # the tensor-level calls
    Q, K, V = Z(rows, 8), Z(cols, 8), Z(cols, 3)
    with pytest.raises(E, match="out must be"):
        sblas.csr_attention(A, Q, K, V, out=Z(rows, 4))
    with pytest.raises(E, match="K must be"):
        sblas.csr_attention(A, Q, Z(cols, 7), V)
    with pytest.raises(E, match="1 .. 128"):
        sblas.csr_attention(A, Z(rows, 129), Z(cols, 129), V)
    with pytest.raises(E, match="row-major"):
        sblas.csr_attention(A, Q, K, Z(3, cols).t())
    with pytest.raises(E, match="float64"):
        sblas.csr_attention(A, Q, K, V.float())
    with pytest.raises(E, match="one value per row"):
        sblas.csr_attention(A, Q, K, V, row_max=Z(rows + 1), row_sum=Z(rows))
    with pytest.raises(E, match="both or neither"):
        sblas.csr_attention(A, Q, K, V, row_sum=Z(rows))
    with pytest.raises(E, match="GPU tensor"):
        sblas.csr_attention(A, Q, K.cpu(), V)
    m, z = Z(rows), Z(rows)
    with pytest.raises(E, match="dO must be"):
        sblas.csr_attention_backward(A, Q, K, V, Z(rows, 4), m, z, dQ=Z(rows, 8))
    with pytest.raises(E, match="dQ must be"):
        sblas.csr_attention_backward(A, Q, K, V, Z(rows, 3), m, z, dQ=Z(rows, 7))
    with pytest.raises(E, match="one value per stored entry"):
        sblas.csr_attention_backward(A, Q, K, V, Z(rows, 3), m, z, dS=Z(len(ci) - 1))
    with pytest.raises(E, match="one value per row"):
        sblas.csr_attention_backward(A, Q, K, V, Z(rows, 3), m[:-1], z, dQ=Z(rows, 8))


# ---- 6. memory: a condition, not a measurement -------------------------------------------------------------------------
def test_the_forward_keeps_nothing_nnz_sized(sblas, cuda):
    """2048 rows of 512 entries (nnz = 2^20), d = dv = 8, Q, K, V requiring grad.  With the graph alive the fused forward
    has grown the allocated memory by less than 8 * nnz bytes -- O, the two row vectors, the workspace, nothing
    nnz-sized -- and that holds for its PEAK too.  The composition's 16 bytes per stored entry are S and P side by side
    while the softmax runs: S is released when P exists (no Function saves it), so the composition is judged at its
    peak (>= 16 * nnz) and, once it has returned, by the P its graph keeps (>= 8 * nnz; measured 8 799 744 bytes)."""
    import torch
    from sblas_amd.autograd import CsrOperator
    rows, per_row, cols, d = 2048, 512, 4096, 8
    nnz = rows * per_row
    assert nnz == 2 ** 20 and sblas.csr_attention_workspace_bytes(rows, nnz, d, d) < 2 ** 20
    rng = np.random.default_rng(40)
    R = up(torch, cuda, AN.rowptr_of([per_row] * rows))
    Ci = up(torch, cuda, rng.integers(0, cols, nnz).astype(np.int32))
    op = CsrOperator(rows, cols, R, Ci)
    Q, K, V = (up(torch, cuda, rng.uniform(-1, 1, s)).requires_grad_() for s in ((rows, d), (cols, d), (cols, d)))

    def growth(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        assert out.grad_fn is not None                                   # the graph is alive
        return torch.cuda.memory_allocated() - before, torch.cuda.max_memory_allocated() - before

    kept, peak = growth(lambda: op.attention(Q, K, V, 0.35))
    kept_c, peak_c = growth(lambda: op.matmul(op.softmax(op.sddmm(Q, K), 0.35), V))
    print("bytes after / at the peak of the forward: fused %d / %d, composition %d / %d (nnz = %d)" % (kept, peak, kept_c, peak_c, nnz))
    assert kept < 8 * nnz and peak < 8 * nnz, (kept, peak)
    assert peak_c >= 16 * nnz and kept_c >= 8 * nnz, (kept_c, peak_c)
