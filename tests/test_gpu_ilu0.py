"""ILU(0) on the GPU (Ilu0Plan, ilu0) against tests/ilu0_numerics.py.

Every case is factored under six schedules -- auto, per_level, chain, and auto with chain_rows = 1, one below the widest
level and the widest level itself -- which must agree bit for bit with one another and with ilu0_ref(), the contract's
loop in scalar float64: the bits of lu are a function of val and the pattern alone.  Every threshold (the default
chain_rows, the boundaries of the lane-group width G(p), the longest row factored in LDS) is read from ilu0_limits()."""
import ctypes as C

import numpy as np
import pytest

import ilu0_numerics as IN
import sptrsv_numerics as TN

pytestmark = pytest.mark.gpu

INVALID = 1


@pytest.fixture(scope="module")
def env(sblas, cuda):
    import torch
    return sblas, torch, cuda


def up(torch, cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def schedules(widest):
    return [("auto", dict()), ("per_level", dict(mode="per_level")), ("chain", dict(mode="chain")),
            ("auto/1", dict(chain_rows=1)), ("auto/widest-1", dict(chain_rows=max(widest - 1, 1))),
            ("auto/widest", dict(chain_rows=max(widest, 1)))]


def same_bits(name, label, got, want):
    """== on the bits, NaNs compared as NaNs (which NaN a difference holds is the subtractor's choice)"""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "%s: %s has its NaNs elsewhere" % (name, label)
    same = IN.bits(got)[~nan] == IN.bits(want)[~nan]
    assert same.all(), "%s: %s differs from the reference in %d of %d entries, first at %d: %r vs %r" % (
        name, label, (~same).sum(), same.size, np.flatnonzero(~same)[0], got[~nan][~same][0], want[~nan][~same][0])


def factor_all(env, name, n, rp, ci, val, ref=None):
    """lu as numpy, after every schedule has given the reference's bits; also -> {schedule: info}"""
    S, torch, cuda = env
    if ref is None:
        ref = IN.ilu0_ref(n, rp, ci, val)
    lv, nl = TN.levels(n, rp, ci, True)
    widest = int(TN.level_widths(lv, nl).max()) if n else 0
    lds_max = S.ilu0_limits()["lds_max"]
    drp, dci, dval = up(torch, cuda, rp, ci, val)
    infos = {}
    for label, kw in schedules(widest):
        plan = S.Ilu0Plan(n, drp, dci, **kw)
        info = plan.info()
        out = torch.full_like(dval, -7.0)
        assert plan.factor(dval, out=out) is out
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert info["n"] == n and info["nnz"] == len(ci) and info["levels"] == nl and info["widest_level"] == widest, (name, label, info)
        assert info["launches"] == info["wide_launches"] + info["chain_launches"]
        assert info["longest_row"] == (int(np.diff(rp).max()) if n else 0)
        assert info["long_rows"] == int((np.diff(rp) > lds_max).sum())
        if label == "per_level":
            assert info["wide_launches"] == nl and info["chain_launches"] == 0
        if label == "chain":
            assert info["wide_launches"] == 0 and info["chain_launches"] == (1 if n else 0)
        if label == "auto/widest" and n:
            assert info["wide_launches"] == 0 and info["chain_launches"] == 1
        if label == "auto/widest-1" and widest > 1:
            assert info["wide_launches"] >= 1
        if n:
            assert np.array_equal(plan.diag().cpu().numpy(), IN.check(n, rp, ci)[0]), name
        plan.destroy()
        infos[label] = info
        same_bits(name, label, got, ref)
    return ref, infos


def run_case(env, name, n, rp, ci, seed):
    val = IN.dominant_values(np.random.default_rng(seed), n, rp, ci)
    lu, infos = factor_all(env, name, n, rp, ci, val)
    assert np.isfinite(lu).all()
    return lu, infos, val


# ---------------------------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------------------------
def test_grid_48_has_wide_and_chain_launches(env):
    side = 48
    rp, ci = IN.grid5(side)
    lu, infos, _ = run_case(env, "grid48", side * side, rp, ci, 1)
    a = infos["auto"]
    cr = env[0].ilu0_limits()["chain_rows"]
    assert a["levels"] == 95 and a["chain_rows"] == cr
    assert a["chain_launches"] == 2 and a["wide_launches"] == 95 - 2 * cr, a   # the antidiagonals 1 .. 48 .. 1


def test_ash85_plus_its_diagonal(env, ash85):
    n = ash85["m"]
    rp, ci = IN.full_sorted(n, ash85["rowptr"], ash85["colidx"])
    run_case(env, "ash85", n, rp, ci, 2)


def test_tridiagonal_chain_of_3000_levels(env):
    rp, ci = IN.tridiagonal(3000)
    lu, infos, _ = run_case(env, "tridiagonal", 3000, rp, ci, 3)
    assert infos["auto"]["levels"] == 3000 and infos["auto"]["launches"] == 1 and infos["auto"]["chain_launches"] == 1


def test_diagonal_matrix(env):
    rp, ci = IN.csr_of_rows([[i] for i in range(5000)])
    lu, infos, val = run_case(env, "diagonal", 5000, rp, ci, 4)
    assert infos["auto"]["levels"] == 1 and np.array_equal(lu, val)         # no L part anywhere: nothing changes


def test_exact_product_returns_l0_and_u0_themselves(env):
    rp, ci, val, lu0 = IN.exact_bidiagonal_product(np.random.default_rng(5), 3000)
    lu, _ = factor_all(env, "L0 U0", 3000, rp, ci, val)
    assert np.array_equal(lu, lu0)


def test_rows_around_every_group_boundary_and_the_lds_limit(env):
    lim = env[0].ilu0_limits()
    g4, g16, lds = lim["g4_max"], lim["g16_max"], lim["lds_max"]
    assert (g4, g16) == (4, 32)
    lengths = [1, g4, g4 + 1, g16, g16 + 1, lds - 1, lds, lds + 1, 4 * lds]
    rp, ci, first = IN.arrow_band(lengths)
    n = len(rp) - 1
    lu, infos, val = run_case(env, "arrow and band", n, rp, ci, 6)
    assert infos["auto"]["long_rows"] == 2 and infos["auto"]["longest_row"] == 4 * lds
    # the long rows took real updates, not only divisions: their diagonals moved
    rp64 = rp.astype(np.int64)
    for t in (len(lengths) - 2, len(lengths) - 1):
        b, e = rp64[first + t], rp64[first + t + 1]
        assert lu[e - 1] != val[e - 1]                                      # a diagonal moves by updates alone


def test_levels_wider_than_a_chain_pass_and_than_a_workgroup(env):
    lim = env[0].ilu0_limits()
    rp, ci = IN.block_diagonal(3000, 3)
    lu, infos, _ = run_case(env, "blocks", 9000, rp, ci, 7)
    a = infos["auto"]
    assert a["levels"] == 3 and a["widest_level"] == 3000 and a["wide_launches"] == 3
    assert 4 * 3000 > lim["chain_threads"] and 4 * 3000 > lim["wide_threads"]   # several passes; several workgroups


# ---------------------------------------------------------------------------------------------------------------------
# a random matrix; the residual
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_2000():
    rng = np.random.default_rng(8)
    n = 2000
    rp, ci = IN.random_near_diagonal(rng, n, 12, 100)
    return n, rp, ci, IN.dominant_values(rng, n, rp, ci)


def test_random_dominant_2000(env, random_2000):
    n, rp, ci, val = random_2000
    assert 10.5 < len(ci) / n < 12.5
    lu, infos = factor_all(env, "random 2000", n, rp, ci, val)
    assert np.isfinite(lu).all() and infos["auto"]["levels"] > 20


def test_residual_on_the_leading_300_block(env, random_2000):
    S, torch, cuda = env
    n, rp, ci, val = random_2000
    rp3, ci3, val3 = IN.leading_block(300, rp, ci, val)
    drp, dci, dval = up(torch, cuda, rp3, ci3, val3)
    lu = S.Ilu0Plan(300, drp, dci).factor(dval).cpu().numpy()
    ratio = IN.residual_ratio(300, rp3, ci3, val3, lu)
    print("leading 300 block (%d entries): residual / bound at most %.3g" % (len(ci3), ratio))
    assert ratio <= 1.0, ratio


# ---------------------------------------------------------------------------------------------------------------------
# the plan's behaviour
# ---------------------------------------------------------------------------------------------------------------------
def small_case(seed, n=900):
    rng = np.random.default_rng(seed)
    rp, ci = IN.random_near_diagonal(rng, n, 9, 60)
    return rng, n, rp, ci, IN.dominant_values(rng, n, rp, ci)


def test_in_place_equals_out_of_place(env):
    S, torch, cuda = env
    rng, n, rp, ci, val = small_case(20)
    rp2, ci2, _ = IN.arrow_band([300])                                      # and a row on the long tier
    val2 = IN.dominant_values(rng, len(rp2) - 1, rp2, ci2)
    for n_, rp_, ci_, val_ in ((n, rp, ci, val), (len(rp2) - 1, rp2, ci2, val2)):
        drp, dci, dval = up(torch, cuda, rp_, ci_, val_)
        for kw in (dict(), dict(mode="per_level"), dict(mode="chain")):
            plan = S.Ilu0Plan(n_, drp, dci, **kw)
            lu = plan.factor(dval)
            w = dval.clone()
            assert plan.factor(w, out=w) is w
            assert torch.equal(w.view(torch.int64), lu.view(torch.int64)), kw
            plan.destroy()


def test_new_values_on_the_same_plan_the_one_shot_and_the_pivots(env):
    S, torch, cuda = env
    rng, n, rp, ci, val = small_case(21)
    drp, dci, dval = up(torch, cuda, rp, ci, val)
    plan = S.Ilu0Plan(n, drp, dci)
    first = plan.factor(dval).cpu().numpy()
    val2 = IN.dominant_values(rng, n, rp, ci)
    lu2 = plan.factor(torch.from_numpy(val2).to(cuda))
    second = lu2.cpu().numpy()
    again = plan.factor(dval).cpu().numpy()
    assert np.array_equal(IN.bits(first), IN.bits(again)) and not np.array_equal(first, second)
    assert np.array_equal(IN.bits(second), IN.bits(IN.ilu0_ref(n, rp, ci, val2)))
    piv = plan.pivots(lu2).cpu().numpy()
    assert np.array_equal(IN.bits(piv), IN.bits(second[IN.check(n, rp, ci)[0]]))
    assert np.array_equal(piv, second[plan.diag().cpu().numpy()])
    plan.destroy()
    one = S.ilu0((n, drp, dci, dval)).cpu().numpy()
    assert np.array_equal(IN.bits(one), IN.bits(first))


def test_n_0_and_n_1(env):
    S, torch, cuda = env
    lu, infos = factor_all(env, "n = 0", 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    assert lu.size == 0 and infos["auto"]["launches"] == 0
    lu, infos = factor_all(env, "n = 1", 1, np.array([0, 1], np.int32), np.array([0], np.int32), np.array([4.0]))
    assert lu.tolist() == [4.0] and infos["auto"]["launches"] == 1
    plan = S.Ilu0Plan(0, *up(torch, cuda, np.zeros(1, np.int32), np.zeros(0, np.int32)))
    empty = torch.zeros(0, dtype=torch.float64, device=cuda)
    assert plan.pivots(empty).numel() == 0 and plan.diag().numel() == 0
    assert plan.apply(empty, empty).numel() == 0
    plan.destroy()


def test_apply_on_an_empty_block_with_numpys_strides(env):
    """found by tools/fuzz_plans.py: apply() on a matrix without rows refused a 0 x 3 block that came from numpy, whose
    strides are (0, 0) (SptrsvPlan.solve read them as a layout)"""
    S, torch, cuda = env
    plan = S.Ilu0Plan(0, *up(torch, cuda, np.zeros(1, np.int32), np.zeros(0, np.int32)))
    empty = torch.zeros(0, dtype=torch.float64, device=cuda)
    r = empty.as_strided((0, 3), (0, 0))
    assert tuple(plan.apply(empty, r).shape) == (0, 3)
    plan.destroy()


def test_factor_and_apply_replay_in_a_graph_after_val_and_r_are_overwritten(env):
    S, torch, cuda = env
    rng, n, rp, ci, val = small_case(22, n=1200)
    drp, dci, dval = up(torch, cuda, rp, ci, val)
    dr = torch.from_numpy(rng.standard_normal(n)).to(cuda)
    plan = S.Ilu0Plan(n, drp, dci, chain_rows=8)                            # both kinds of launch in the graph
    assert plan.info()["wide_launches"] >= 1 and plan.info()["chain_launches"] >= 1
    lu, tmp, z = (torch.empty(k, dtype=torch.float64, device=cuda) for k in (len(ci), n, n))
    plan.factor(dval, out=lu)                                               # warm: the code objects are loaded,
    plan.solvers()                                                          # and the two solve plans exist
    plan.apply(lu, dr, out=z, tmp=tmp)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):                                 # a linear chain: no parallel branches
            plan.factor(dval, out=lu)
            plan.apply(lu, dr, out=z, tmp=tmp)
    for _ in range(2):
        dval.copy_(torch.from_numpy(IN.dominant_values(rng, n, rp, ci)))
        dr.copy_(torch.from_numpy(rng.standard_normal(n)))
        lu.fill_(-7.0), tmp.fill_(-7.0), z.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        rlu, rz = lu.clone(), z.clone()
        elu = plan.factor(dval)
        ez = plan.apply(elu, dr)
        torch.cuda.synchronize()
        assert torch.equal(rlu.view(torch.int64), elu.view(torch.int64))
        assert torch.equal(rz.view(torch.int64), ez.view(torch.int64))
        assert np.array_equal(IN.bits(rlu.cpu().numpy()), IN.bits(IN.ilu0_ref(n, rp, ci, dval.cpu().numpy())))
    plan.destroy()


def test_a_zero_pivot_makes_inf_and_nan_where_the_reference_does(env):
    rng = np.random.default_rng(23)
    n, r = 300, 150
    rp, ci = IN.band(n, 6)
    rp64 = rp.astype(np.int64)
    rows = [ci[rp64[i]:rp64[i + 1]].tolist() for i in range(n)]
    rows[r] = [c for c in rows[r] if c >= r]                                # row r eliminates nothing: its pivot is val itself
    rp, ci = IN.csr_of_rows(rows)
    val = IN.dominant_values(rng, n, rp, ci)
    dpos = IN.check(n, rp, ci)[0]
    clean = IN.ilu0_ref(n, rp, ci, val)
    val[dpos[r]] = 0.0
    ref = IN.ilu0_ref(n, rp, ci, val)
    row = np.repeat(np.arange(n), np.diff(rp))
    bad = ~np.isfinite(ref)
    assert np.isnan(ref).any() and np.isinf(ref).any() and bad.sum() > 20 and np.isfinite(ref[row > r]).any()
    assert not bad[row <= r].any()                                          # the dependants only
    assert np.array_equal(IN.bits(ref[row < r]), IN.bits(clean[row < r]))
    factor_all(env, "zero pivot", n, rp, ci, val, ref=ref)                  # classes, positions and the finite rest


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_create_refuses_a_bad_structure_and_names_the_row(env):
    S, torch, cuda = env

    def refused(rows=None, rp=None, ci=None, **kw):
        if rows is not None:
            rp, ci = IN.csr_of_rows(rows)
        with pytest.raises(S.SblasError) as e:
            S.Ilu0Plan(len(rp) - 1, *up(torch, cuda, rp, ci), **kw)
        return e.value

    e = refused([[0], [0, 1], [1], [0, 3], [0]])                            # rows 2 and 4 lack a diagonal
    assert e.bad_row == 2 and "row 2" in str(e) and "code %d" % INVALID in str(e)
    assert refused([[0], [1, 0], [2]]).bad_row == 1                         # unsorted
    assert refused([[0], [1], [1, 2, 2]]).bad_row == 2                      # a doubled entry
    assert refused([[0], [1, 0], [2, 3]]).bad_row == 2                      # the ranges of every row come first
    assert refused(rp=np.array([0, 2, 1, 3], np.int32), ci=np.array([0, 1, 2], np.int32)).bad_row == 1
    assert refused(rp=np.array([0, 1, 2, 3], np.int32), ci=np.array([0, 1, 2, 2], np.int32)).bad_row == 2   # ends short of nnz
    with pytest.raises(S.SblasError):
        S.Ilu0Plan(3, *up(torch, cuda, np.array([0, 1, 2, 3], np.int32), np.array([0, 1, 2], np.int32)), mode="fastest")


def test_calls_are_refused_before_anything_is_launched(env):
    S, torch, cuda = env
    rng, n, rp, ci, val = small_case(24, n=300)
    drp, dci, dval = up(torch, cuda, rp, ci, val)
    plan = S.Ilu0Plan(n, drp, dci)
    lu = torch.full_like(dval, -7.0)
    L = S.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    other_rp, other_ci = drp.clone(), dci.clone()                            # the same structure at other addresses
    for prp, pci in ((other_rp, dci), (drp, other_ci)):
        assert L.sblas_hip_ilu0_f64_i32_planned(plan.handle, stream, prp.data_ptr(), pci.data_ptr(), dval.data_ptr(),
                                                lu.data_ptr()) == INVALID
    assert L.sblas_hip_ilu0_f64_i32_planned(None, stream, drp.data_ptr(), dci.data_ptr(), dval.data_ptr(), lu.data_ptr()) == INVALID
    assert L.sblas_hip_ilu0_f64_i32_planned(plan.handle, stream, drp.data_ptr(), dci.data_ptr(), None, lu.data_ptr()) == INVALID
    assert L.sblas_hip_ilu0_f64_i32_planned(plan.handle, stream, drp.data_ptr(), dci.data_ptr(), dval.data_ptr(), None) == INVALID
    bad = [lambda: plan.factor(dval.cpu()), lambda: plan.factor(dval, out=lu.cpu()), lambda: plan.factor(dval.float()),
           lambda: plan.factor(dval[:-1]), lambda: plan.factor(dval, out=lu[:-1]), lambda: plan.factor(dval, out=lu.float()),
           lambda: plan.pivots(lu[:-1]),
           lambda: S.Ilu0Plan(n, drp.cpu(), dci), lambda: S.Ilu0Plan(n, drp, dci.cpu()),
           lambda: S.Ilu0Plan(n, drp.long(), dci), lambda: S.Ilu0Plan(n, drp, dci.long()),
           lambda: S.Ilu0Plan(n + 1, drp, dci), lambda: S.Ilu0Plan(n, drp, dci[:-1])]
    for k, call in enumerate(bad):
        with pytest.raises(S.SblasError):
            call()
            pytest.fail("call %d was accepted" % k)
    torch.cuda.synchronize()
    assert bool((lu == -7.0).all())                                         # nothing ran
    plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# it is a preconditioner
# ---------------------------------------------------------------------------------------------------------------------
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


def test_it_is_a_preconditioner(env):
    S, torch, cuda = env
    side, tol = 32, 1e-10
    n = side * side
    rp, ci = IN.grid5(side)
    val = np.where(TN.on_diagonal(rp, ci), 4.0, -1.0)                       # the five-point Laplacian
    b = np.random.default_rng(30).standard_normal(n)
    host = host_pcg(n, rp, ci, val, b, IN.ilu0_ref(n, rp, ci, val), tol)    # the count to beat comes from the reference
    drp, dci, dval, db = up(torch, cuda, rp, ci, val, b)
    ilu = S.Ilu0Plan(n, drp, dci)
    lu = ilu.factor(dval)
    dev = device_pcg(env, n, drp, dci, dval, db, ilu, lu, tol)
    plain = device_pcg(env, n, drp, dci, dval, db, None, None, tol)
    ilu.destroy()
    counts = "PCG iterations: device %d, host reference %d; plain CG on the device %d" % (dev, host, plain)
    print(counts)
    assert dev <= host + 2, counts
    assert 2 * dev < plain, counts
