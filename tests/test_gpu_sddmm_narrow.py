"""The narrow SDDMM on the GPU (sblas_hip_sddmm_narrow_f64_i32 through sblas_amd.sddmm_narrow) against the device SDDMM it
promises the bits of: part="all" equals sddmm_tensor bit for bit at every k <= 8, whatever the leading dimensions and
alignments, and every other part equals that result masked on the host.  The pattern is built around the kernel's run
length, read from sddmm_narrow_limits(): a row over three runs, a row that starts on a run boundary, empty rows on a
boundary and a last run of 1, 2 and 3 entries."""
import numpy as np
import pytest

import sddmm_numerics as SN

pytestmark = pytest.mark.gpu

KS = list(range(1, 9))
PARTS = ["all", "lower", "upper", "strict_lower", "strict_upper"]
_cache = {}


def part_mask(part, r, c):
    return {"all": np.ones(len(c), bool), "lower": c <= r, "upper": c >= r, "strict_lower": c < r, "strict_upper": c > r}[part]


def pattern(S, tail):
    """(n, n, rowptr, colidx): 6 runs and `tail` entries, about 3 000 rows; columns unsorted, duplicates allowed"""
    key = ("pat", tail)
    if key in _cache:
        return _cache[key]
    L = S.sddmm_narrow_limits()["chunk"]
    rng = np.random.default_rng(100 + tail)
    lens = []

    def short_rows_until(total):
        while sum(lens) < total:
            lens.append(min(int(rng.integers(0, 5)), total - sum(lens)))
    short_rows_until(L - 10)
    lens.append(L + 30)                      # entries [L - 10, 2 L + 20): one row over three runs
    short_rows_until(3 * L)
    lens.append(5)                           # starts exactly on a run boundary
    short_rows_until(4 * L)
    lens.extend([0] * 5)                     # empty rows on a boundary, then the row that starts there
    lens.append(3)
    short_rows_until(6 * L)
    lens.append(tail)                        # the last run: a ragged group of one lane
    n = len(lens)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = rng.integers(0, n, int(rp[-1])).astype(np.int32)
    assert rp[-1] == 6 * L + tail and 5000 <= rp[-1] <= 9000 and 2000 <= n <= 4000, (n, rp[-1])
    starts = set(rp[:-1][np.diff(rp) > 0].tolist())
    assert 3 * L in starts and 4 * L in starts and (np.diff(rp)[np.searchsorted(rp, 4 * L):][:5] == 0).all()
    _cache[key] = (n, n, rp, ci)
    return _cache[key]


def operands(pat, k, seed=0):
    rows, cols, rp, ci = pat
    rng = np.random.default_rng(1000 * k + seed)
    return SN.log_uniform(rng, (rows, k), 24), SN.log_uniform(rng, (cols, k), 24), SN.log_uniform(rng, len(ci), 24)


def dev_pattern(torch, dev, pat, offset=False):
    rows, cols, rp, ci = pat
    R = torch.from_numpy(rp).to(dev)
    if offset:                               # colidx as a view one element (4 bytes) into its base
        base = torch.zeros(len(ci) + 1, dtype=torch.int32, device=dev)
        base[1:].copy_(torch.from_numpy(ci))
        return rows, cols, R, base[1:]
    return rows, cols, R, torch.from_numpy(ci).to(dev)


def sliced(torch, dev, M, ld, off):
    """M (r x k numpy) as a row-major device view with leading dimension ld that starts `off` elements into its base;
    everything around it holds NaN"""
    r, k = M.shape
    base = torch.full((r * ld + off + ld,), float("nan"), dtype=torch.float64, device=dev)
    view = base[off:off + r * ld].view(r, ld)[:, :k]
    view.copy_(torch.from_numpy(np.ascontiguousarray(M)))
    return view


def bits(t):
    return t.cpu().numpy().view(np.uint64)


def reference(S, torch, dev, pat, k, alpha=1.0, beta=0.0):
    """sddmm_tensor on contiguous operands: (X, Y, old, result) on the device, computed once per (pattern, k, alpha, beta)"""
    key = ("ref", pat[2][-1], k, alpha, beta)
    if key not in _cache:
        Xh, Yh, oldh = operands(pat, k)
        X, Y, old = (torch.from_numpy(a).to(dev) for a in (Xh, Yh, oldh))
        A = dev_pattern(torch, dev, pat)
        out = old.clone()
        S.sddmm_tensor(A, X, Y, out, alpha, beta)
        _cache[key] = (X, Y, old, out)
    return _cache[key]


@pytest.mark.parametrize("k", KS)
def test_all_equals_sddmm_tensor(sblas, cuda, k):
    import torch
    for tail in (1, 2, 3):
        pat = pattern(sblas, tail)
        X, Y, old, want = reference(sblas, torch, cuda, pat, k)
        out = torch.full_like(old, float("nan"))        # beta == 0 never reads out
        sblas.sddmm_narrow(dev_pattern(torch, cuda, pat), X, Y, out)
        assert (bits(out) == bits(want)).all(), (k, tail, int((bits(out) != bits(want)).sum()))


@pytest.mark.parametrize("k", KS)
def test_layouts_alignments_and_beta(sblas, cuda, k):
    """ld > k, an odd ld, a base 8 bytes off (the 8-byte row loads), colidx 4 bytes off and out 8 bytes off (the narrow
    index loads and stores), beta != 0: the same bits each time.  `even` and `odd` are leading dimensions above k of that
    parity: aligned bases with two even ones run the 16-byte row loads at every k, the odd widths' scalar last element
    included; one even and one odd must fall back to the 8-byte loads."""
    import torch
    pat = pattern(sblas, 3)
    nnz = len(pat[3])
    Xh, Yh, _ = operands(pat, k)
    even, odd = k + 2 - k % 2, k + 1 + k % 2
    assert even % 2 == 0 and odd % 2 == 1 and min(even, odd) > k
    for alpha, beta in ((1.0, 0.0), (-2.0, 0.5)):
        X, Y, old, want = reference(sblas, torch, cuda, pat, k, alpha, beta)
        for ldx, offx, ldy, offy, off_ci, off_out in ((k + 2, 0, k + 4, 0, False, False), (k + 1 + k % 2, 0, k + 3 - k % 2, 0, False, False),
                                                      (k + 2, 1, k + 2, 1, False, False), (k, 0, k + 2, 1, True, True),
                                                      (k, 0, k, 0, True, False), (k, 0, k, 0, False, True),
                                                      (even, 0, even + 2, 0, False, False), (even, 0, odd, 0, False, False),
                                                      (odd, 0, even, 0, False, False), (even, 0, even, 0, True, True)):
            A = dev_pattern(torch, cuda, pat, offset=off_ci)
            base = torch.full((nnz + 1,), float("nan"), dtype=torch.float64, device=cuda)
            out = base[1:] if off_out else base[:nnz]
            out.copy_(old)
            sblas.sddmm_narrow(A, sliced(torch, cuda, Xh, ldx, offx), sliced(torch, cuda, Yh, ldy, offy), out, alpha, beta)
            assert (bits(out) == bits(want)).all(), (k, alpha, beta, ldx, offx, ldy, offy, off_ci, off_out)
            assert torch.isnan(base[0] if off_out else base[nnz])          # nothing written beside out


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("k", KS)
def test_parts_equal_the_masked_sddmm(sblas, cuda, k, part):
    import torch
    for tail, (alpha, beta) in ((1, (1.0, 0.0)), (2, (-2.0, 0.5))):
        pat = pattern(sblas, tail)
        rows, cols, rp, ci = pat
        X, Y, old, full = reference(sblas, torch, cuda, pat, k, alpha, beta)
        mask = part_mask(part, SN.row_of_entries(rp), ci.astype(np.int64))
        assert part == "all" or (mask.any() and not mask.all())
        outside = np.zeros(len(ci)) if beta == 0 else beta * old.cpu().numpy()
        want = np.where(mask, full.cpu().numpy(), outside)
        out = old.clone() if beta else torch.full_like(old, float("nan"))
        sblas.sddmm_narrow(dev_pattern(torch, cuda, pat), X, Y, out, alpha, beta, part=part)
        assert (bits(out) == want.view(np.uint64)).all(), (k, part, tail)


@pytest.mark.parametrize("k", KS)
def test_rows_outside_the_part_are_never_read(sblas, cuda, k):
    """Inf and NaN in every row of X and Y that only entries outside the part name: every output is finite, and equal to
    the clean run's"""
    import torch
    pat = pattern(sblas, 2)
    rows, cols, rp, ci = pat
    r, c = SN.row_of_entries(rp), ci.astype(np.int64)
    for part in ("strict_lower", "upper"):
        mask = part_mask(part, r, c)
        Xh, Yh, _ = operands(pat, k)
        bad_x = np.setdiff1d(r[~mask], r[mask])
        bad_y = np.setdiff1d(c[~mask], c[mask])
        assert len(bad_x) > 10 and len(bad_y) > 10
        Xp, Yp = Xh.copy(), Yh.copy()
        Xp[bad_x] = np.where(np.arange(len(bad_x))[:, None] % 2 == 0, np.nan, np.inf)
        Yp[bad_y] = np.where(np.arange(len(bad_y))[:, None] % 2 == 0, -np.inf, np.nan)
        A = dev_pattern(torch, cuda, pat)
        clean = torch.empty(len(ci), dtype=torch.float64, device=cuda)
        got = torch.empty_like(clean)
        sblas.sddmm_narrow(A, torch.from_numpy(Xh).to(cuda), torch.from_numpy(Yh).to(cuda), clean, part=part)
        sblas.sddmm_narrow(A, torch.from_numpy(Xp).to(cuda), torch.from_numpy(Yp).to(cuda), got, part=part)
        assert torch.isfinite(got).all() and (bits(got) == bits(clean)).all()
        assert (got.cpu().numpy()[~mask] == 0).all() and not np.signbit(got.cpu().numpy()[~mask]).any()
        # inside the part the classes follow the operands: poison a row that an inside entry names
        e = int(np.flatnonzero(mask)[0])
        Xq = Xh.copy()
        Xq[r[e]] = np.inf
        sblas.sddmm_narrow(A, torch.from_numpy(Xq).to(cuda), torch.from_numpy(Yh).to(cuda), got, part=part)
        cls = SN.predict_class(rp, ci, Xq, Yh, None, 1.0, 0.0)
        g = got.cpu().numpy()
        seen = np.where(np.isnan(g), 1, np.where(g == np.inf, 2, np.where(g == -np.inf, 3, 0)))
        assert (seen[mask] == cls[mask]).all() and (seen[~mask] == 0).all() and seen[e] != 0


def test_one_dimensional_operands_are_k1(sblas, cuda):
    import torch
    pat = pattern(sblas, 1)
    X, Y, old, want = reference(sblas, torch, cuda, pat, 1)
    out = torch.empty_like(old)
    sblas.sddmm_narrow(dev_pattern(torch, cuda, pat), X[:, 0], Y[:, 0], out)
    assert (bits(out) == bits(want)).all()
    wide = torch.from_numpy(operands(pat, 3)[1]).to(cuda)                   # a strided 1-D view: ld = 3
    want = torch.empty_like(old)
    sblas.sddmm_tensor(dev_pattern(torch, cuda, pat), X, wide[:, 1:2], want)
    sblas.sddmm_narrow(dev_pattern(torch, cuda, pat), X[:, 0], wide[:, 1], out)
    assert (bits(out) == bits(want)).all()


def test_degenerate_sizes(sblas, cuda):
    import torch
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=cuda)
    f64 = lambda *shape: torch.ones(*shape, dtype=torch.float64, device=cuda)
    sblas.sddmm_narrow((0, 0, i32([0]), i32([])), f64(0, 2), f64(0, 2), f64(0))                    # rows = 0
    sblas.sddmm_narrow((4, 3, i32([0] * 5), i32([])), f64(4, 2), f64(3, 2), f64(0), part="lower")   # nnz = 0
    for part, want in (("all", 6.0), ("lower", 6.0), ("strict_upper", 0.0)):                         # nnz = 1: entry (2, 1)
        out = torch.full((1,), float("nan"), dtype=torch.float64, device=cuda)
        sblas.sddmm_narrow((4, 3, i32([0, 0, 0, 1, 1]), i32([1])), 2 * f64(4, 3), f64(3, 3), out, part=part)
        assert out.item() == want
    for bad in (dict(k=9), dict(k=0), dict(part=5), dict(part=-1)):
        k = bad.get("k", 2)
        with pytest.raises(sblas.SblasError):
            sblas.sddmm_narrow((4, 3, i32([0, 0, 0, 1, 1]), i32([1])), f64(4, k), f64(3, k), f64(1), part=bad.get("part", "all"))
    with pytest.raises(sblas.SblasError):
        sblas.sddmm_narrow((4, 3, i32([0, 0, 0, 1, 1]), i32([1])), f64(4, 2).cpu(), f64(3, 2), f64(1))
    with pytest.raises(sblas.SblasError):
        sblas.sddmm_narrow((4, 3, i32([0, 0, 0, 1, 1]), i32([1])), f64(4, 2).float(), f64(3, 2), f64(1))
    buf = f64(12)                                                          # out inside X's extent, then inside Y's
    for X, Y in ((buf[:8].view(4, 2), f64(3, 2)), (f64(4, 2), buf[2:8].view(3, 2))):
        with pytest.raises(sblas.SblasError, match="overlap"):
            sblas.sddmm_narrow((4, 3, i32([0, 0, 0, 1, 1]), i32([1])), X, Y, buf[3:4])
    sblas.sddmm_narrow((4, 3, i32([0, 0, 0, 1, 1]), i32([1])), buf[:8].view(4, 2), f64(3, 2), buf[8:9])     # just behind X: fine
    assert buf[8].item() == 2.0


@pytest.mark.parametrize("k", KS)
def test_graph_capture_replays_on_new_values(sblas, cuda, k):
    import torch
    pat = pattern(sblas, 3)
    A = dev_pattern(torch, cuda, pat)
    Xh, Yh, _ = operands(pat, k)
    X, Y = torch.from_numpy(Xh).to(cuda), torch.from_numpy(Yh).to(cuda)
    out = torch.zeros(len(pat[3]), dtype=torch.float64, device=cuda)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sblas.sddmm_narrow(A, X, Y, out, 0.5, 0.0, part="lower")           # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sblas.sddmm_narrow(A, X, Y, out, 0.5, 0.0, part="lower")
    X2h, Y2h, _ = operands(pat, k, seed=7)
    X.copy_(torch.from_numpy(X2h))
    Y.copy_(torch.from_numpy(Y2h))
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    eager = torch.empty_like(out)
    sblas.sddmm_narrow(A, X, Y, eager, 0.5, 0.0, part="lower")
    assert (bits(out) == bits(eager)).all() and torch.isfinite(out).all()
