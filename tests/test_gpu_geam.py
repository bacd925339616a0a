"""GEAM on the GPU (GeamPlan, csr_add, autograd.csr_add) against the library's scalar reference geam_ref, which
tests/test_geam_host.py pins to the numpy restatement of the contract.  Every case runs as create makes it, with
general=True, and as create makes it with the two-launch ordered-scatter numeric (scatter=True); all three must give
the reference's rowptr, colidx, dest_a and dest_b exactly and its values bit for bit
(spgemm_numerics.same_bits: equal bits; where the reference holds a NaN, a NaN).  Then one device cross-check through
coo_to_csr(dup="sum"), the plan's behaviour, contract (I), what is built on C, autograd and the refusals."""
import ctypes as C

import numpy as np
import pytest

import geam_numerics as AN
import spgemm_numerics as GN

pytestmark = pytest.mark.gpu

INVALID = 1
CASES = AN.shape_cases()
_ref = {}


@pytest.fixture(scope="module")
def env(sblas, cuda):
    import torch
    return sblas, torch, cuda


def up(torch, cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def ascending(M):
    rp, ci = M[0], M[1]
    return all((np.diff(ci[rp[i]:rp[i + 1]]) > 0).all() for i in range(len(rp) - 1))


def reference(S, name, rows, cols, A, B, alpha, beta):
    key = (name, alpha, beta)
    if key not in _ref:
        _ref[key] = S.geam_ref(rows, cols, A[0], A[1], A[2], B[0], B[1], B[2], alpha, beta)
    return _ref[key]


def run_case(env, name, rows, cols, A, B, alpha=1.0, beta=1.0):
    """both plans against the reference -> {route: (info, rowptr, colidx, val, dest_a, dest_b)} as numpy"""
    S, torch, cuda = env
    ref = reference(S, name, rows, cols, A, B, alpha, beta)
    dA, dB = up(torch, cuda, *A), up(torch, cuda, *B)
    want_path = "sorted" if ascending(A) and ascending(B) else "general"
    out = {}
    for route, kw in (("auto", dict()), ("general", dict(general=True)), ("scatter", dict(scatter=True))):
        plan = S.GeamPlan(rows, cols, dA[0], dA[1], dB[0], dB[1], **kw)
        info = plan.info()
        rp, ci = plan.csr()
        da, db = plan.maps()
        val = plan.add(dA[2], dB[2], alpha, beta)
        torch.cuda.synchronize()
        got = (info,) + tuple(t.cpu().numpy().copy() for t in (rp, ci, val, da, db))
        plan.destroy()
        assert info["path"] == ("general" if route == "general" else want_path) and info["scatter"] == (route == "scatter"), (name, route)
        assert info["a_ascending"] == ascending(A) and info["b_ascending"] == ascending(B), (name, route)
        assert info["nnz_c"] == len(ref[1]) and info["matched"] == len(A[1]) + len(B[1]) - len(ref[1]), (name, route)
        assert info["launches"] == (0 if not len(ref[1]) else 1 if info["path"] == "sorted" and route != "scatter" else 2), (name, route)
        for k, what in ((1, "rowptr"), (2, "colidx"), (4, "dest_a"), (5, "dest_b")):
            assert np.array_equal(got[k], ref[k - 1]), (name, route, what)
        if not GN.same_bits(got[3], ref[2]):
            bad = np.flatnonzero(GN.bits(got[3]) != GN.bits(ref[2]))
            pytest.fail("%s / %s: %d of %d values differ from the reference, first at %d: %r vs %r"
                        % (name, route, len(bad), len(ref[2]), bad[0], got[3][bad[0]], ref[2][bad[0]]))
        out[route] = got
    return out


# ---------------------------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_host_cases(env, name):
    rows, cols, A, B = CASES[name]
    run_case(env, name, rows, cols, A, B, *AN.scalars_of(name))


def test_special_values_on_both_paths(env):
    for k, name in enumerate(("identical", "a_in_b", "unsorted", "dup_both", "random3_sorted")):
        rows, cols, A, B = CASES[name]
        A, B = AN.special_values(A, B, 3410 + k)
        for alpha, beta in ((1.0, 1.0), (0.0, -1.0), (0.5, 3e200), (3e200, 0.0)):
            run_case(env, "special_" + name, rows, cols, A, B, alpha, beta)


def test_zeros_and_a_zero_alpha(env):
    inf, nan, tiny = np.inf, np.nan, 5e-324
    A = AN.csr_of_rows([([2], [-0.0]), ([3], [-0.0]), ([1, 6], [inf, 2.0]), ([0], [tiny]), ([4], [inf]), ([4], [nan])])
    B = AN.csr_of_rows([([5], [1.0]), ([3], [0.0]), ([], []), ([0], [tiny]), ([4], [-inf]), ([1], [1.0])])
    for route, got in run_case(env, "zeros", 6, 7, A, B).items():
        _, rp, ci, val = got[:4]
        assert val[rp[0]] == 0.0 and np.signbit(val[rp[0]]), route           # -0.0 alone stays -0.0
        assert val[rp[1]] == 0.0 and not np.signbit(val[rp[1]]), route       # (-0.0) + 0.0 is +0.0
        assert val[rp[3]] == 2 * tiny and np.isnan(val[rp[4]]), route
    for route, got in run_case(env, "zeros_alpha0", 6, 7, A, B, 0.0, 1.0).items():
        _, rp, ci, val = got[:4]
        assert rp.tolist() == [0, 2, 3, 5, 6, 7, 9] and np.isnan(val[rp[2]]), route   # A's pattern stays; 0 * Inf is a stored NaN


def test_no_product_is_fused_into_the_add(env):
    """The mutation pair (geam_numerics.FMA_*): alpha * a = 3 * fl(1/3) rounds to 1 and beta * b = -3 * fl(1/3) to -1, so the
    contract's sum is +0.0; a kernel that contracts A's product into the add gives -2^-54, one that contracts B's gives
    +2^-54.  (Checked once by hand: with the contraction pragma taken out of geam.hip the compiler emits the fused
    instruction in the sorted path's numeric kernel, and this test then fails with +2^-54 in every entry.)  Swapping
    the two terms of a matched entry cannot show in a two-term sum, which commutes; the order shows with three terms, on (0, 3) of dup_both: ((1e16 + 1) - 1e16) + 5 = 5, any other order 6."""
    n = 700                                                                  # more than one workgroup, a ragged last one
    A = (np.arange(n + 1, dtype=np.int32), np.zeros(n, np.int32), np.full(n, AN.FMA_A))
    B = (np.arange(n + 1, dtype=np.int32), np.zeros(n, np.int32), np.full(n, AN.FMA_B))
    for route, got in run_case(env, "fma", n, 1, A, B, AN.FMA_ALPHA, AN.FMA_BETA).items():
        assert (got[3] == 0.0).all() and not np.signbit(got[3]).any(), route
    rows, cols, A, B = CASES["dup_both"]
    got = run_case(env, "dup_both_11", rows, cols, A, B)["auto"]
    assert got[3][got[1][0] + list(got[2][got[1][0]:got[1][1]]).index(3)] == 5.0


def test_one_row_that_spans_many_workgroups(env):
    rng = np.random.default_rng(3420)
    n, cols = 5000, 20000
    ca = np.sort(np.concatenate((3 * np.arange(n // 3 + 1), 3 * rng.choice(6000, n - n // 3 - 1, replace=False) + 1)))
    cb = np.sort(np.concatenate((3 * np.arange(n // 3 + 1), 3 * rng.choice(6000, n - n // 3 - 1, replace=False) + 2)))
    assert len(ca) == len(cb) == n and len(np.intersect1d(ca, cb)) == n // 3 + 1          # every third column is shared
    row = lambda c: (np.array([0, 0, n, n], np.int32), c.astype(np.int32), rng.random(n) * 2 - 1)   # rows 0 and 2 are empty
    out = run_case(env, "long_row", 3, cols, row(ca), row(cb), 0.5, -1.0)
    assert out["auto"][0]["matched"] == n // 3 + 1


def test_many_short_rows_with_empty_rows_at_workgroup_edges(env):
    rng = np.random.default_rng(3421)
    rows, cols = 3000, 40

    def short(empty_every):
        lens = rng.integers(0, 4, rows)
        lens[::empty_every] = 0
        rp = np.zeros(rows + 1, np.int32)
        rp[1:] = np.cumsum(lens)
        ci = np.concatenate([np.sort(rng.choice(cols, L, replace=False)) for L in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
        return rp, ci, rng.random(len(ci)) * 2 - 1
    A, B = short(4), short(5)
    assert len(A[1]) > 4 * 256 and any(A[0][i] % 256 == 0 and A[0][i] == A[0][i + 1] for i in range(1, rows))  # an empty row on an edge
    run_case(env, "short_rows", rows, cols, A, B, -1.0, 0.5)


def test_sizes_that_are_multiples_of_the_workgroup_and_an_empty_last_row(env):
    rng = np.random.default_rng(3422)
    cols = 900

    def blocky(lens):
        rp = np.zeros(len(lens) + 1, np.int32)
        rp[1:] = np.cumsum(lens)
        ci = np.concatenate([np.sort(rng.choice(cols, L, replace=False)) for L in lens]).astype(np.int32)
        return rp, ci, rng.random(len(ci)) * 2 - 1
    A = blocky([256, 0, 100, 156, 256, 0])                                    # row boundaries on 256, 512, 768; the last row empty
    B = blocky([128, 128, 256, 0, 512, 0])
    assert len(A[1]) == 768 and len(B[1]) == 1024
    run_case(env, "blocky", 6, cols, A, B)
    one = (np.array([0, 0, 0, 1, 1, 1, 1], np.int32), np.array([int(A[1][300])], np.int32), np.array([2.5]))   # nnz(B) = 1, matched
    run_case(env, "one_b", 6, cols, A, one)
    run_case(env, "one_a", 6, cols, one, A, 3.0, 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# the device cross-check
# ---------------------------------------------------------------------------------------------------------------------
def test_plan_equals_coo_to_csr_sum_of_the_scaled_triplets_on_the_device(env):
    S, torch, cuda = env
    rng = np.random.default_rng(3423)
    rows, cols, alpha, beta = 400, 300, 0.75, -3.0
    A, B = GN.random_csr(rng, rows, cols, 6), GN.random_csr(rng, rows, cols, 5)
    row = np.concatenate((AN.rows_of(A[0]), AN.rows_of(B[0])))
    col = np.concatenate((A[1], B[1]))
    val = np.concatenate((alpha * A[2], beta * B[2]))                        # rounded once on the host: the same bits
    d = up(torch, cuda, row, col, val)
    rp, ci, v, _, _ = S.coo_to_csr(rows, cols, d[0], d[1], d[2], dup="sum")
    dA, dB = up(torch, cuda, *A), up(torch, cuda, *B)
    for kw in (dict(), dict(general=True)):
        plan = S.GeamPlan(rows, cols, dA[0], dA[1], dB[0], dB[1], **kw)
        prp, pci = plan.csr()
        pv = plan.add(dA[2], dB[2], alpha, beta)
        torch.cuda.synchronize()
        assert torch.equal(prp, rp) and torch.equal(pci, ci) and torch.equal(pv.view(torch.int64), v.view(torch.int64))
        plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# plan behaviour
# ---------------------------------------------------------------------------------------------------------------------
def small_pair(seed, sort=True):
    rng = np.random.default_rng(seed)
    rows, cols = 180, 150
    return rows, cols, GN.random_csr(rng, rows, cols, 5, sort=sort, empty_every=7), GN.random_csr(rng, rows, cols, 4, sort=sort, empty_every=5)


@pytest.mark.parametrize("sort", [True, False])
def test_add_again_with_new_values_into_out_and_at_an_offset(env, sort):
    S, torch, cuda = env
    rows, cols, A, B = small_pair(3424, sort)
    rng = np.random.default_rng(3425)
    dA, dB = up(torch, cuda, *A), up(torch, cuda, *B)
    plan = S.GeamPlan(rows, cols, dA[0], dA[1], dB[0], dB[1])
    assert plan.info()["path"] == ("sorted" if sort else "general")
    ref = lambda va, vb, al, be: S.geam_ref(rows, cols, A[0], A[1], va, B[0], B[1], vb, al, be)[2]
    first = plan.add(dA[2], dB[2], 1.0, 1.0)
    va2, vb2 = rng.random(len(A[1])) - 0.5, rng.random(len(B[1])) - 0.5
    dva2, dvb2 = up(torch, cuda, va2, vb2)
    second = plan.add(dva2, dvb2, -0.5, 3.0)
    out = torch.full((plan.nnz_c + 3,), -7.0, dtype=torch.float64, device=cuda)
    given = plan.add(dA[2], dB[2], 2.0, -1.0, out=out)
    assert given.data_ptr() == out.data_ptr()
    # the three value arrays one element off 16-byte alignment
    pad = lambda t: torch.cat((torch.zeros(1, dtype=torch.float64, device=cuda), t))[1:]
    oa, ob, oo = pad(dva2), pad(dvb2), torch.empty(plan.nnz_c + 1, dtype=torch.float64, device=cuda)[1:]
    assert oa.data_ptr() % 16 == 8 and ob.data_ptr() % 16 == 8 and oo.data_ptr() % 16 == 8
    plan.add(oa, ob, -0.5, 3.0, out=oo)
    torch.cuda.synchronize()
    assert GN.same_bits(first.cpu().numpy(), ref(A[2], B[2], 1.0, 1.0))
    assert GN.same_bits(second.cpu().numpy(), ref(va2, vb2, -0.5, 3.0))
    assert GN.same_bits(out[:plan.nnz_c].cpu().numpy(), ref(A[2], B[2], 2.0, -1.0)) and (out[plan.nnz_c:] == -7.0).all()
    assert torch.equal(oo.view(torch.int64), second.view(torch.int64))
    # the one-shot call owns its tensors
    rpc, cic, vc = S.csr_add((rows, cols) + tuple(dA), (rows, cols) + tuple(dB), 1.0, 1.0)
    prp, pci = plan.csr()
    assert torch.equal(rpc, prp) and torch.equal(cic, pci) and torch.equal(vc.view(torch.int64), first.view(torch.int64))
    assert rpc.data_ptr() != prp.data_ptr()
    plan.destroy()


@pytest.mark.parametrize("sort,scatter", [(True, False), (False, False), (True, True)])
def test_add_replays_in_a_graph_with_refilled_value_buffers(env, sort, scatter):
    S, torch, cuda = env
    rows, cols, A, B = small_pair(3426, sort)
    dA, dB = up(torch, cuda, *A), up(torch, cuda, *B)
    plan = S.GeamPlan(rows, cols, dA[0], dA[1], dB[0], dB[1], scatter=scatter)
    bufa, bufb = dA[2].clone(), dB[2].clone()
    out = torch.empty(plan.nnz_c, dtype=torch.float64, device=cuda)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            plan.add(bufa, bufb, 0.5, -2.0, out=out)
    rng = np.random.default_rng(3427)
    for _ in range(2):
        na, nb = rng.random(len(A[1])) * 2 - 1, rng.random(len(B[1])) * 2 - 1
        bufa.copy_(torch.from_numpy(na)), bufb.copy_(torch.from_numpy(nb))
        out.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        assert GN.same_bits(out.cpu().numpy(), S.geam_ref(rows, cols, A[0], A[1], na, B[0], B[1], nb, 0.5, -2.0)[2])
    plan.destroy()


def test_a_rows_bits_do_not_depend_on_where_the_row_stands(env):
    rows, cols, A, B = small_pair(3428)
    rng = np.random.default_rng(3429)
    perm = rng.permutation(rows)                                             # row i of the pair becomes row perm[i]

    def permuted(M):
        rp, ci, v = M
        lens = np.zeros(rows, np.int64)
        lens[perm] = np.diff(rp)
        rp2 = np.zeros(rows + 1, np.int32)
        rp2[1:] = np.cumsum(lens)
        ci2, v2 = np.zeros_like(ci), np.zeros_like(v)
        for i in range(rows):
            ci2[rp2[perm[i]]:rp2[perm[i] + 1]], v2[rp2[perm[i]]:rp2[perm[i] + 1]] = ci[rp[i]:rp[i + 1]], v[rp[i]:rp[i + 1]]
        return rp2, ci2, v2
    base = run_case(env, "indep", rows, cols, A, B, 0.3, -1.7)
    moved = run_case(env, "indep_moved", rows, cols, permuted(A), permuted(B), 0.3, -1.7)
    for route in base:
        _, rp, ci, val = base[route][:4]
        _, rq, cj, wal = moved[route][:4]
        for i in range(rows):
            p = perm[i]
            assert np.array_equal(ci[rp[i]:rp[i + 1]], cj[rq[p]:rq[p + 1]]), (route, i)
            assert np.array_equal(GN.bits(val[rp[i]:rp[i + 1]]), GN.bits(wal[rq[p]:rq[p + 1]])), (route, i)


# ---------------------------------------------------------------------------------------------------------------------
# downstream
# ---------------------------------------------------------------------------------------------------------------------
def test_spmv_on_the_sum_is_the_sum_of_the_spmvs_exactly_on_integers(env):
    S, torch, cuda = env
    rng = np.random.default_rng(3430)
    rows, cols, alpha, beta = 210, 160, 3.0, -2.0
    A, B = GN.random_csr(rng, rows, cols, 5, integer=True), GN.random_csr(rng, rows, cols, 6, integer=True)
    x = rng.integers(-4, 5, cols).astype(np.float64)
    dA, dB = up(torch, cuda, *A), up(torch, cuda, *B)
    (dx,) = up(torch, cuda, x)
    plan = S.GeamPlan(rows, cols, dA[0], dA[1], dB[0], dB[1])
    rpc, cic = plan.csr()
    vc = plan.add(dA[2], dB[2], alpha, beta)
    y = torch.zeros(rows, dtype=torch.float64, device=cuda)
    sp = S.SpmvPlan(rows, cols, rpc, cic)
    sp(vc, dx, 1.0, 0.0, y)
    torch.cuda.synchronize()
    want = alpha * (GN.to_dense(rows, cols, *A) @ x) + beta * (GN.to_dense(rows, cols, *B) @ x)
    assert np.array_equal(y.cpu().numpy(), want)
    sp.destroy(), plan.destroy()


def test_a_plus_its_transpose_is_structurally_symmetric(env):
    S, torch, cuda = env
    rng = np.random.default_rng(3431)
    n = 230
    A = GN.random_csr(rng, n, n, 5)
    dA = up(torch, cuda, *A)
    tp = S.TransposePlan(n, n, dA[0], dA[1], dA[2])
    colptr, rowidx, valT = tp.csc()
    plan = S.GeamPlan(n, n, dA[0], dA[1], colptr, rowidx)
    assert plan.info()["path"] == "sorted"
    rp, ci = plan.csr()
    val = plan.add(dA[2], valT)
    torch.cuda.synchronize()
    rp, ci, val = rp.cpu().numpy(), ci.cpu().numpy(), val.cpu().numpy()
    pat = GN.pattern_dense(n, n, rp, ci)
    assert np.array_equal(pat, pat.T)
    dense = GN.to_dense(n, n, rp, ci, val)
    assert np.array_equal(dense, dense.T)                                    # a + b and b + a are the same bits
    tp.destroy(), plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# autograd
# ---------------------------------------------------------------------------------------------------------------------
def grad_pair(kind):
    if kind == "sorted":                                                     # 6 x 7, (1, 2) and (4, 6) shared
        A = AN.csr_of_rows([([0, 3], [1.0, 2.0]), ([2], [0.5]), ([], []), ([1, 5, 6], [1.5, -1.0, 2.5]), ([6], [3.0]), ([4], [-2.0])])
        B = AN.csr_of_rows([([1], [1.0]), ([2, 4], [2.0, -0.5]), ([0], [1.0]), ([], []), ([0, 6], [0.25, 4.0]), ([3], [1.0])])
    else:                                                                    # duplicates in A, in B, and on (0, 3) in both
        A = AN.csr_of_rows([([3, 1, 3], [1.0, 2.0, 0.5]), ([2], [0.5]), ([], []), ([5, 5], [1.5, -1.0]), ([6], [3.0]), ([4], [-2.0])])
        B = AN.csr_of_rows([([3, 3], [1.0, -4.0]), ([4, 2], [2.0, -0.5]), ([0], [1.0]), ([], []), ([6, 0, 6], [0.25, 4.0, 1.0]), ([3], [1.0])])
    return 6, 7, A, B


@pytest.mark.parametrize("kind,need", [("sorted", (True, True)), ("general", (True, True)), ("sorted", (True, False)), ("general", (False, True))])
def test_gradcheck_of_csr_add(env, kind, need):
    S, torch, cuda = env
    import sblas_amd.autograd as AG
    rows, cols, A, B = grad_pair(kind)
    dA, dB = up(torch, cuda, *A), up(torch, cuda, *B)
    plan = S.GeamPlan(rows, cols, dA[0], dA[1], dB[0], dB[1])
    assert plan.info()["path"] == kind
    va, vb = dA[2].clone().requires_grad_(need[0]), dB[2].clone().requires_grad_(need[1])
    assert torch.autograd.gradcheck(lambda a, b: AG.csr_add(plan, a, b, 0.75, -1.5), (va, vb), eps=1e-6, atol=1e-7)
    out = AG.csr_add(plan, va, vb, 0.75, -1.5)
    w = torch.arange(1, plan.nnz_c + 1, dtype=torch.float64, device=cuda)
    (out * w).sum().backward()
    da, db = plan.maps()
    if need[0]:
        assert torch.equal(va.grad, 0.75 * w[da.long()])
    else:
        assert va.grad is None
    if need[1]:
        assert torch.equal(vb.grad, -1.5 * w[db.long()])
    else:
        assert vb.grad is None
    plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(env):
    S, torch, cuda = env
    L = S.lib()
    rows, cols, A, B = small_pair(3432)

    def create(A, B, rows=rows, cols=cols, null=(), flags=0, out=True):
        d = up(torch, cuda, A[0], A[1], B[0], B[1])
        ptrs = [None if j in null else t.data_ptr() for j, t in enumerate(d)]
        h = C.c_void_p()
        rc = L.sblas_hip_geam_plan_create(-1, None, rows, cols, ptrs[0], ptrs[1], ptrs[2], ptrs[3], flags, C.byref(h) if out else None)
        torch.cuda.synchronize()
        assert rc == 0 or not h.value                                        # no plan is made
        if rc == 0:
            L.sblas_hip_geam_plan_destroy(h)
        return rc

    assert create(A, B) == 0 and create(A, B, flags=1) == 0 and create(A, B, flags=2) == 0
    for which, M in ((0, A), (1, B)):
        down, late, high, neg = M[0].copy(), M[0].copy(), M[1].copy(), M[1].copy()
        down[1] = down[2] + 1
        late[0] = 1
        high[3] = cols
        neg[5] = -1
        for bad in ((down, M[1], M[2]), (late, M[1], M[2]), (M[0], high, M[2]), (M[0], neg, M[2])):
            for flags in (0, 1):
                assert create(*((bad, B) if which == 0 else (A, bad)), flags=flags) == INVALID
    for null in ((0,), (1,), (2,), (3,)):
        assert create(A, B, null=null) == INVALID
    assert create(A, B, out=False) == INVALID
    assert create(A, B, rows=-1) == INVALID and create(A, B, cols=1 << 31) == INVALID and create(A, B, flags=3) == INVALID
    # numeric: the argument path
    dA, dB = up(torch, cuda, *A), up(torch, cuda, *B)
    plan = S.GeamPlan(rows, cols, dA[0], dA[1], dB[0], dB[1])
    out = torch.empty(plan.nnz_c, dtype=torch.float64, device=cuda)
    num = L.sblas_hip_geam_plan_numeric
    assert num(None, None, dA[2].data_ptr(), dB[2].data_ptr(), 1.0, 1.0, out.data_ptr()) == INVALID
    assert num(plan.handle, None, None, dB[2].data_ptr(), 1.0, 1.0, out.data_ptr()) == INVALID
    assert num(plan.handle, None, dA[2].data_ptr(), None, 1.0, 1.0, out.data_ptr()) == INVALID
    assert num(plan.handle, None, dA[2].data_ptr(), dB[2].data_ptr(), 1.0, 1.0, None) == INVALID
    big = torch.zeros(plan.nnz_c + len(A[1]), dtype=torch.float64, device=cuda)          # val_c over val_a's tail; over val_b
    assert num(plan.handle, None, big.data_ptr(), dB[2].data_ptr(), 1.0, 1.0, big.data_ptr() + 8 * (len(A[1]) - 1)) == INVALID
    assert num(plan.handle, None, dA[2].data_ptr(), dB[2].data_ptr(), 1.0, 1.0, dB[2].data_ptr()) == INVALID
    assert num(plan.handle, None, big.data_ptr(), dB[2].data_ptr(), 1.0, 1.0, big.data_ptr() + 8 * len(A[1])) == 0   # side by side
    assert L.sblas_hip_geam_plan_info(None, (C.c_int64 * 12)()) == INVALID
    assert L.sblas_hip_geam_plan_csr(None, None, None) == INVALID and L.sblas_hip_geam_plan_maps(None, None, None) == INVALID
    with pytest.raises(S.SblasError, match="out has"):
        plan.add(dA[2], dB[2], out=out[:-1])
    with pytest.raises(S.SblasError, match="entries"):
        plan.add(dA[2][:-1], dB[2])
    with pytest.raises(S.SblasError, match="float64"):
        plan.add(dA[2].float(), dB[2])
    with pytest.raises(S.SblasError, match="row pointers end"):
        S.GeamPlan(rows, cols, dA[0], dA[1][:-1], dB[0], dB[1])
    with pytest.raises(S.SblasError):
        S.csr_add((rows, cols) + tuple(dA), (rows + 1, cols) + tuple(dB))
    with pytest.raises(S.SblasError, match="exclude"):
        S.GeamPlan(rows, cols, dA[0], dA[1], dB[0], dB[1], general=True, scatter=True)
    plan.destroy()
    torch.cuda.synchronize()


def test_a_plan_used_on_another_current_device_is_refused(env):
    S, torch, cuda = env
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    rows, cols, A, B = small_pair(3433)
    dA, dB = up(torch, cuda, *A), up(torch, cuda, *B)
    plan = S.GeamPlan(rows, cols, dA[0], dA[1], dB[0], dB[1])
    out = torch.empty(plan.nnz_c, dtype=torch.float64, device=cuda)
    with torch.cuda.device(1):
        assert S.lib().sblas_hip_geam_plan_numeric(plan.handle, None, dA[2].data_ptr(), dB[2].data_ptr(), 1.0, 1.0, out.data_ptr()) == INVALID
    plan.destroy()
