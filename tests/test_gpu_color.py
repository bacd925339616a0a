"""Multicolour reordering on the GPU (ColorPlan, PermutePlan, csr_color) against tests/color_numerics.py.

The colours are a function of the pattern and the seed alone, so everything is compared with ==: color with the host rule
(color_ref, itself held against the numpy restatement in test_color_host.py), perm / inv / color_ptr with numpy's stable
sort, P A P^T and src with the host permutation.  Every threshold (the boundaries of the lane-group width G(p), the colour
window) is read from color_limits()."""
import numpy as np
import pytest

import color_numerics as CN
import ilu0_numerics as IN
import sptrsv_numerics as TN

pytestmark = pytest.mark.gpu

INVALID = 1
CASES = CN.cases()


@pytest.fixture(scope="module")
def env(sblas, cuda):
    import torch
    return sblas, torch, cuda


def up(torch, cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def colour(env, name, n, rp, ci, seed):
    """the plan's arrays as numpy, after color == the host rule's, the order == numpy's and info() agrees with both"""
    S, torch, cuda = env
    want, k, sync = S.color_ref(n, rp, ci, seed)
    drp, dci = up(torch, cuda, rp, ci)
    plan = S.ColorPlan(n, drp, dci, seed=seed)
    info = plan.info()
    color, perm, inv, ptr = (t.cpu().numpy() for t in plan.order())
    plan.destroy()
    assert color.dtype == np.int32 and np.array_equal(color, want), "%s seed %d: %d colours differ, first at %s" % (
        name, seed, (color != want).sum(), np.flatnonzero(color != want)[:3])
    wperm, winv, wptr, wk = CN.order(want)
    assert wk == k
    assert np.array_equal(perm, wperm) and np.array_equal(inv, winv) and np.array_equal(ptr, wptr), (name, seed)
    sizes = np.diff(wptr)
    deg = CN.degrees(n, rp, ci)
    assert info == dict(n=n, nnz=len(ci), colors=k, rounds=info["rounds"], largest_class=int(sizes.max()) if n else 0,
                        smallest_class=int(sizes.min()) if n else 0, largest_degree=int(deg.max()) if n else 0,
                        bytes=info["bytes"]), (name, seed, info)
    print("%s seed %d: %d colours, %d rounds on the device, %d synchronous" % (name, seed, k, info["rounds"], sync))
    assert (1 <= info["rounds"] <= sync) if n else info["rounds"] == 0, (name, seed, info, sync)
    assert info["bytes"] >= 12 * n
    return color, perm, inv, ptr, info


# ---------------------------------------------------------------------------------------------------------------------
# colours and order
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("seed", [0, 1])
def test_colours_and_order_equal_the_host_rule(env, name, seed):
    n, rp, ci, _ = CASES[name]
    colour(env, name, n, rp, ci, seed)


def test_counts_of_the_issue(env):
    for name, k in (("grid48", 5), ("tridiagonal3000", 3), ("band600", 31), ("block_diagonal", 70), ("clique130", 130),
                    ("star5000", 2), ("diagonal", 1)):
        n, rp, ci, _ = CASES[name]
        assert colour(env, name, n, rp, ci, 0)[4]["colors"] == k


def test_a_vertex_at_below_and_above_each_lane_group_boundary(env):
    lim = env[0].color_limits()
    lengths = [0, 1, lim["g4_max"] - 1, lim["g4_max"], lim["g4_max"] + 1, lim["g16_max"] - 1, lim["g16_max"], lim["g16_max"] + 1,
               63, 64, 65, 2 * lim["window"] + 3]
    rp, ci, first = CN.degree_rows(lengths)
    n = len(rp) - 1
    assert CN.degrees(n, rp, ci)[first:].tolist() == lengths                # rows of exactly these p
    for seed in (0, 1, 2):
        info = colour(env, "degree rows", n, rp, ci, seed)[4]
        assert info["largest_degree"] == max(lengths)
    # the same with every entry doubled and each row reversed: p doubles, the graph and so the colours do not change
    rp64 = rp.astype(np.int64)
    rows = [ci[rp64[i]:rp64[i + 1]].tolist() for i in range(n)]
    rp2, ci2 = CN.csr_of_rows([(r + r)[::-1] for r in rows])
    assert np.array_equal(colour(env, "degree rows doubled", n, rp2, ci2, 0)[0], env[0].color_ref(n, rp, ci, 0)[0])


def test_cliques_that_need_the_second_and_the_third_colour_window(env):
    W = env[0].color_limits()["window"]
    for size in (W, W + 1, 2 * W, 2 * W + 1):
        rp, ci = CN.clique(size)
        color, perm, _, ptr, info = colour(env, "clique %d" % size, size, rp, ci, 0)
        assert info["colors"] == size and info["largest_class"] == info["smallest_class"] == 1
        assert sorted(color.tolist()) == list(range(size))
    # a clique of W + 1 inside a sparse graph, stored as its lower triangle only (half of every vertex's entries are in A^T)
    size = W + 1
    rows = [list(range(i + 1)) for i in range(size)] + [[i, i - size] for i in range(size, 3 * size)]
    rp, ci = CN.csr_of_rows(rows)
    assert colour(env, "lower clique with tails", 3 * size, rp, ci, 1)[4]["colors"] == size


def test_the_one_shot_returns_tensors_of_its_own(env):
    S, torch, cuda = env
    n, rp, ci, _ = CASES["grid48"]
    drp, dci = up(torch, cuda, rp, ci)
    color, perm, ptr = S.csr_color((n, drp, dci), seed=2)
    want = S.color_ref(n, rp, ci, 2)[0]
    wperm, _, wptr, _ = CN.order(want)
    assert np.array_equal(color.cpu().numpy(), want) and np.array_equal(perm.cpu().numpy(), wperm)
    assert np.array_equal(ptr.cpu().numpy(), wptr)


def test_create_refuses_a_bad_structure_and_names_the_row(env):
    S, torch, cuda = env

    def refused(rp, ci, **kw):
        with pytest.raises(S.SblasError) as e:
            S.ColorPlan(len(rp) - 1, *up(torch, cuda, np.asarray(rp, np.int32), np.asarray(ci, np.int32)), **kw)
        return e.value

    e = refused([0, 2, 4, 6], [0, 1, 1, 3, 2, -1])                          # rows 1 and 2 hold a column outside
    assert e.bad_row == 1 and "row 1" in str(e) and "code %d" % INVALID in str(e)
    assert refused([0, 2, 1, 3], [0, 1, 2]).bad_row == 1                    # row 1 ends before it starts
    assert refused([0, 2, 1, 3], [0, 7, 2]).bad_row == 1                    # ... and rowptr comes before the columns
    assert refused([0, 1, 2, 3], [0, 1, 2, 2]).bad_row == 2                 # ends short of nnz
    n, rp, ci, _ = CASES["grid48"]
    drp, dci = up(torch, cuda, rp, ci)
    bad = [lambda: S.ColorPlan(n, drp.cpu(), dci), lambda: S.ColorPlan(n, drp, dci.cpu()), lambda: S.ColorPlan(n, drp.long(), dci),
           lambda: S.ColorPlan(n, drp, dci.long()), lambda: S.ColorPlan(n + 1, drp, dci), lambda: S.ColorPlan(n, rp, ci)]
    for k, call in enumerate(bad):
        with pytest.raises(S.SblasError):
            call()
            pytest.fail("call %d was accepted" % k)


# ---------------------------------------------------------------------------------------------------------------------
# P A P^T
# ---------------------------------------------------------------------------------------------------------------------
def permuted(env, name, n, rp, ci, perm, plan):
    """the plan's B == the host's, values() an exact gather; -> (rowptr_b, colidx_b, src) as numpy"""
    S, torch, cuda = env
    wrp, wci, wsrc = CN.permute(n, rp, ci, perm)
    rpb, cib, src = (t.cpu().numpy() for t in plan.csr())
    assert rpb.dtype == cib.dtype == src.dtype == np.int32
    assert np.array_equal(rpb, wrp) and np.array_equal(cib, wci) and np.array_equal(src, wsrc), name
    inv = np.zeros(n, np.int64)
    inv[np.asarray(perm, np.int64)] = np.arange(n)
    assert np.array_equal(plan.inverse().cpu().numpy(), inv)
    val = np.random.default_rng(5).standard_normal(len(ci))
    val[::7] = -0.0
    dval, = up(torch, cuda, val)
    out = torch.full_like(dval, -7.0)
    assert plan.values(dval, out=out) is out
    assert np.array_equal(TN.bits(out.cpu().numpy()), TN.bits(val[wsrc]))
    assert np.array_equal(TN.bits(plan.values(dval).cpu().numpy()), TN.bits(val[wsrc]))
    info = plan.info()
    assert info["n"] == n and info["nnz"] == len(ci) and info["bytes"] >= 4 * (2 * n + 2 * len(ci))
    return wrp, wci, wsrc


@pytest.mark.parametrize("name", ["grid48", "random4000", "messy", "arrow_band", "block_diagonal", "star5000", "n0", "n1"])
def test_permuted_structure_and_values_equal_the_host_s(env, name):
    S, torch, cuda = env
    n, rp, ci, _ = CASES[name]
    drp, dci = up(torch, cuda, rp, ci)
    cp = S.ColorPlan(n, drp, dci)
    perm = cp.order()[1].cpu().numpy()
    plan = cp.permute(drp, dci)
    cp.destroy()                                                            # the permute plan keeps nothing of it
    rpb, cib, _ = permuted(env, name, n, rp, ci, perm, plan)
    plan.destroy()
    if n:
        assert (np.diff(cib.astype(np.int64))[np.diff(np.repeat(np.arange(n), np.diff(rpb))) == 0] >= 0).all()   # sorted rows
    if name == "messy":
        assert (np.diff(cib.astype(np.int64))[np.diff(np.repeat(np.arange(n), np.diff(rpb))) == 0] == 0).any()   # duplicates kept


def test_any_permutation_not_only_a_colouring_s(env):
    S, torch, cuda = env
    rng = np.random.default_rng(6)
    n, rp, ci, _ = CASES["messy"]
    for perm in (rng.permutation(n), np.arange(n), np.arange(n)[::-1]):
        perm = np.ascontiguousarray(perm, np.int32)
        drp, dci, dperm = up(torch, cuda, rp, ci, perm)
        plan = S.PermutePlan(n, drp, dci, dperm)
        dperm.fill_(0)                                                      # the plan has its own copy
        permuted(env, "messy", n, rp, ci, perm, plan)
        plan.destroy()


def test_vectors_go_there_and_back_with_their_bits(env):
    S, torch, cuda = env
    n, rp, ci, _ = CASES["random4000"]
    perm = np.random.default_rng(7).permutation(n).astype(np.int32)
    drp, dci, dperm = up(torch, cuda, rp, ci, perm)
    plan = S.PermutePlan(n, drp, dci, dperm)
    x = np.random.default_rng(8).standard_normal(n)
    x[::5] = -0.0
    dx, = up(torch, cuda, x)
    xb = plan.to_permuted(dx)
    assert np.array_equal(TN.bits(xb.cpu().numpy()), TN.bits(x[perm]))
    back = torch.full_like(dx, -7.0)
    assert plan.from_permuted(xb, out=back) is back
    assert np.array_equal(TN.bits(back.cpu().numpy()), TN.bits(x))
    for call in (lambda: plan.to_permuted(dx[:-1]), lambda: plan.to_permuted(dx.float()), lambda: plan.to_permuted(dx.cpu()),
                 lambda: plan.from_permuted(dx, out=dx), lambda: plan.values(dx)):
        with pytest.raises(S.SblasError):
            call()
    plan.destroy()


def test_a_perm_that_is_no_permutation_is_refused_with_its_index(env):
    S, torch, cuda = env
    n, rp, ci, _ = CASES["grid48"]
    drp, dci = up(torch, cuda, rp, ci)
    good = np.random.default_rng(9).permutation(n).astype(np.int32)

    def refused(perm):
        with pytest.raises(S.SblasError) as e:
            S.PermutePlan(n, drp, dci, up(torch, cuda, perm)[0])
        assert "code %d" % INVALID in str(e.value) and "perm[%d]" % e.value.bad_index in str(e.value)
        return e.value.bad_index

    p = good.copy()
    p[1500] = p[20]                                                         # a repeat: its second place is the bad one
    assert refused(p) == 1500
    p = good.copy()
    p[1700], p[300] = n, -1                                                 # out of range, both ends
    assert refused(p) == 300
    p = good.copy()
    p[900] = p[10]
    p[40] = n + 5
    assert refused(p) == 40                                                 # the first index, whatever its fault
    p[40] = good[40]
    assert refused(p) == 900
    for call in (lambda: S.PermutePlan(n, drp, dci, up(torch, cuda, good.astype(np.int64))[0]),
                 lambda: S.PermutePlan(n, drp, dci, up(torch, cuda, good[:-1])[0]),
                 lambda: S.PermutePlan(n, drp, dci, torch.from_numpy(good))):
        with pytest.raises(S.SblasError):
            call()
    bad_ci = ci.copy()
    bad_ci[5] = n
    with pytest.raises(S.SblasError):                                       # a bad structure never reaches the relabel kernel
        S.PermutePlan(n, drp, up(torch, cuda, bad_ci)[0], up(torch, cuda, good)[0])


def test_values_replays_in_a_graph_as_one_node(env):
    S, torch, cuda = env
    n, rp, ci, _ = CASES["random4000"]
    rng = np.random.default_rng(10)
    perm = rng.permutation(n).astype(np.int32)
    drp, dci, dperm = up(torch, cuda, rp, ci, perm)
    plan = S.PermutePlan(n, drp, dci, dperm)
    src = plan.csr()[2].cpu().numpy()
    dval, = up(torch, cuda, rng.standard_normal(len(ci)))
    out = torch.empty_like(dval)
    plan.values(dval, out=out)                                              # warm: the code object is loaded
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):                                 # a linear chain: one node
            plan.values(dval, out=out)
    for _ in range(2):
        val = rng.standard_normal(len(ci))
        dval.copy_(torch.from_numpy(val))
        out.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(TN.bits(out.cpu().numpy()), TN.bits(val[src]))
    plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# the consumers
# ---------------------------------------------------------------------------------------------------------------------
def multicolour(env, n, rp, ci, val, seed=0):
    """-> (PermutePlan, B on the host as (rowptr, colidx, val), B on the device likewise, colours)"""
    S, torch, cuda = env
    drp, dci, dval = up(torch, cuda, rp, ci, val)
    cp = S.ColorPlan(n, drp, dci, seed=seed)
    k = cp.info()["colors"]
    perm = cp.order()[1].cpu().numpy()
    plan = cp.permute(drp, dci)
    cp.destroy()
    rpb, cib, src = CN.permute(n, rp, ci, perm)
    drpb, dcib, _ = plan.csr()
    return plan, (rpb, cib, val[src]), (drpb, dcib, plan.values(dval)), k


def test_ilu0_on_the_permuted_grid_has_as_many_levels_as_colours(env):
    S, torch, cuda = env
    side = 48
    n = side * side
    rp, ci = IN.grid5(side)
    val = IN.dominant_values(np.random.default_rng(11), n, rp, ci)
    plan, (rpb, cib, valb), (drpb, dcib, dvalb), k = multicolour(env, n, rp, ci, val)
    assert k == 5
    ilu = S.Ilu0Plan(n, drpb, dcib)
    info = ilu.info()
    assert info["levels"] == k == 5, info
    lu = ilu.factor(dvalb).cpu().numpy()
    assert np.array_equal(TN.bits(lu), TN.bits(IN.ilu0_ref(n, rpb, cib, valb)))
    lower, upper = ilu.solvers()
    assert lower.info()["levels"] == upper.info()["levels"] == k
    ilu.destroy(), plan.destroy()


def host_pcg(n, rp, ci, val, b, lu, tol, limit=1000):
    """preconditioned CG on the host: A p by rows, M^-1 r by the reference's factor and substitution in stored order;
    lu = None is plain CG.  -> iterations until |r| <= tol |b|"""
    rp = rp.astype(np.int64)
    row = np.repeat(np.arange(n), np.diff(rp))
    matvec = lambda x: np.bincount(row, val * x[ci], minlength=n)

    def precond(r):
        if lu is None:
            return r.copy()
        y = np.zeros(n)
        for i in range(n):
            c, v = ci[rp[i]:rp[i + 1]], lu[rp[i]:rp[i + 1]]
            y[i] = r[i] - np.dot(v[c < i], y[c[c < i]])
        z = np.zeros(n)
        for i in range(n - 1, -1, -1):
            c, v = ci[rp[i]:rp[i + 1]], lu[rp[i]:rp[i + 1]]
            z[i] = (y[i] - np.dot(v[c > i], z[c[c > i]])) / v[c == i][0]
        return z

    x, r = np.zeros(n), b.copy()
    z = precond(r)
    p, rz, stop = z.copy(), r @ z, tol * np.linalg.norm(b)
    for it in range(1, limit + 1):
        q = matvec(p)
        alpha = rz / (p @ q)
        x, r = x + alpha * p, r - alpha * q
        if np.linalg.norm(r) <= stop:
            return it
        z = precond(r)
        rz, old = r @ z, rz
        p = z + (rz / old) * p
    return limit + 1


def device_pcg(env, n, drp, dci, dval, db, ilu, lu, tol, limit=1000):
    """the same loop in torch: SpmvPlan for A p, Ilu0Plan.apply for M^-1 r (ilu = None: plain CG)"""
    S, torch, cuda = env
    spmv = S.SpmvPlan(n, n, drp, dci)
    x, r = torch.zeros_like(db), db.clone()
    q, z, tmp = torch.empty_like(db), torch.empty_like(db), torch.empty_like(db)
    precond = (lambda r: ilu.apply(lu, r, out=z, tmp=tmp)) if ilu is not None else (lambda r: r)
    zz = precond(r)
    p, rz, stop = zz.clone(), torch.dot(r, zz), tol * float(torch.linalg.norm(db))
    count = limit + 1
    for it in range(1, limit + 1):
        spmv(dval, p, 1.0, 0.0, q)
        alpha = rz / torch.dot(p, q)
        x += alpha * p
        r -= alpha * q
        if float(torch.linalg.norm(r)) <= stop:
            count = it
            break
        zz = precond(r)
        rz, old = torch.dot(r, zz), rz
        p = zz + (rz / old) * p
    spmv.destroy()
    return count


def test_it_is_still_a_preconditioner(env):
    """The 32 x 32 Laplacian, b from rng(30), tol 1e-10, as in test_gpu_ilu0.py.  The multicolour order weakens ILU(0): the
    host reference takes 62 iterations against 41 in the natural order and 115 without a preconditioner, so the bound
    on the device count is the reference's count on the permuted system, and it must still beat plain CG -- not by the
    factor of two the natural order is held to."""
    S, torch, cuda = env
    side, tol = 32, 1e-10
    n = side * side
    rp, ci = IN.grid5(side)
    val = np.where(TN.on_diagonal(rp, ci), 4.0, -1.0)                       # the five-point Laplacian
    b = np.random.default_rng(30).standard_normal(n)
    plan, (rpb, cib, valb), (drpb, dcib, dvalb), k = multicolour(env, n, rp, ci, val)
    db, = up(torch, cuda, b)
    bb = plan.to_permuted(db)
    assert np.array_equal(TN.bits(bb.cpu().numpy()), TN.bits(b[plan.perm.cpu().numpy()]))
    host = host_pcg(n, rpb, cib, valb, bb.cpu().numpy(), IN.ilu0_ref(n, rpb, cib, valb), tol)
    natural = host_pcg(n, rp, ci, val, b, IN.ilu0_ref(n, rp, ci, val), tol)
    ilu = S.Ilu0Plan(n, drpb, dcib)
    assert ilu.info()["levels"] == k
    lu = ilu.factor(dvalb)
    dev = device_pcg(env, n, drpb, dcib, dvalb, bb, ilu, lu, tol)
    plain = device_pcg(env, n, drpb, dcib, dvalb, bb, None, None, tol)
    ilu.destroy(), plan.destroy()
    counts = "PCG iterations in the multicolour order (%d colours): device %d, host reference %d; host reference in the natural " \
             "order %d; plain CG on the device %d" % (k, dev, host, natural, plain)
    print(counts)
    assert dev <= host + 2, counts
    assert dev < plain, counts
