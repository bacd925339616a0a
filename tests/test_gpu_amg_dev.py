"""Aggregation on the device (amg_aggregate.hip and amg.hip's create with aggregation="device"): the
stand-alone aggregation against the host rule on every case, both sides of every lane-group bound and a randomised sweep;
plans made in the two modes array for array, value for value, in apply (eager and replayed from a graph) and inside PCG; the
refusals.  Every integer comparison is ==, every value comparison is on the bits."""
import ctypes

import numpy as np
import pytest

import amg_dev_numerics as DN
import amg_numerics as AN
import amg_sa_numerics as SA
import krylov_numerics as KN

pytestmark = pytest.mark.gpu

RTOL = 1e-10
SALTS = ((0, 0), (7, 0), (0, 3), (7, 3))                                     # (seed, level)


@pytest.fixture(scope="module")
def env(sblas, cuda):
    import torch
    return sblas, torch, cuda


def up(torch, cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def shifted(torch, cuda, a):
    """a on the device, one element into its allocation"""
    a = np.ascontiguousarray(a)
    buf = torch.zeros(len(a) + 1, dtype=torch.from_numpy(a).dtype, device=cuda)
    buf[1:].copy_(torch.from_numpy(a))
    return buf[1:]


def same(a, b):
    return KN.same_bits(a, b)


def host(t):
    return t.cpu().numpy() if t is not None else np.zeros(0)


def assert_aggregation(env, c, salts=SALTS, offset=False):
    """amg_aggregate_device == amg_aggregate in agg, aggptr and members; 1 <= rounds <= the synchronous form's"""
    S, torch, cuda = env
    n, rp, ci, val, theta = c["n"], c["rp"], c["ci"], DN.values(c), c["theta"]
    put = (lambda a: shifted(torch, cuda, a)) if offset else (lambda a: up(torch, cuda, a)[0])
    drp, dci = put(rp), put(ci)
    dval = put(val) if val is not None else None
    for seed, level in salts:
        want_agg, want_ptr, want_members = S.amg_aggregate(n, rp, ci, val, theta, seed=seed, level=level)
        bound = S.amg_roots_rounds_ref(n, rp, ci, val, theta, seed=seed, level=level)[1]
        agg, aggptr, members, rounds = S.amg_aggregate_device(n, drp, dci, dval, theta, seed=seed, level=level)
        what = (c["name"], seed, level, offset)
        print("%s seed %d level %d: %d aggregates, %d rounds on the device, %d in the synchronous form" % (c["name"], seed, level, len(want_ptr) - 1,
                                                                                                          rounds, bound))
        assert agg.dtype == aggptr.dtype == members.dtype == torch.int32, what
        assert np.array_equal(host(agg), want_agg), what
        assert np.array_equal(host(aggptr), want_ptr), what
        assert np.array_equal(host(members), want_members), what
        assert rounds <= bound and (rounds >= 1 if n >= 1 else rounds == 0), (what, rounds, bound)
        assert np.array_equal(host(drp), rp) and np.array_equal(host(dci), ci)   # read only


# ---------------------------------------------------------------------------------------------------------------------
# the stand-alone aggregation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", AN.CASES)
def test_the_device_aggregation_equals_the_host_rule(env, name):
    c = AN.case(name)
    assert_aggregation(env, c)
    assert_aggregation(env, c, salts=SALTS[:1], offset=True)


def test_the_priority_path_needs_more_rounds_than_one_batch_allows_for(env):
    S, torch, cuda = env
    c = DN.priority_path(300)
    assert S.amg_roots_rounds_ref(c["n"], c["rp"], c["ci"])[1] == 300
    assert_aggregation(env, c)
    assert_aggregation(env, c, salts=SALTS[:1], offset=True)
    assert len(S.amg_aggregate_device(c["n"], *up(torch, cuda, c["rp"], c["ci"]))[1]) - 1 == 150


def test_one_way_edges(env):
    c, _ = DN.one_way()
    assert_aggregation(env, c)
    assert_aggregation(env, c, salts=SALTS[:1], offset=True)


@pytest.mark.parametrize("theta", [0.25, 1.0])
@pytest.mark.parametrize("kind", DN.BOUND_CLASSES)
def test_bound_classes(env, kind, theta):
    c = DN.bound_class(kind, theta)
    assert_aggregation(env, c)
    assert_aggregation(env, c, salts=SALTS[:1], offset=True)


@pytest.mark.parametrize("theta", [0.0, 0.3])
def test_width_boundaries(env, theta):
    c = DN.widths(theta)
    assert set(DN.WIDTH_LENGTHS) <= set(np.diff(c["rp"]).tolist())
    assert_aggregation(env, c)
    assert_aggregation(env, c, salts=SALTS[:1], offset=True)


def test_the_randomised_sweep(env):
    ran = 0
    for k in range(DN.SWEEP):
        c = DN.sweep_case(k)
        assert 1 <= c["n"] <= 400
        assert_aggregation(env, c, salts=((k, k % 4),))
        ran += 1
    assert ran == 24


# ---------------------------------------------------------------------------------------------------------------------
# plans made in the two modes
# ---------------------------------------------------------------------------------------------------------------------
PLANS = [(name, kind) for name in ("grid24", "grid32", "aniso32", "clique130", "star5000", "random4000", "random600")
         for kind in ("plain", "smoothed") if not (name == "random4000" and kind == "smoothed")]


def plan_arrays(torch, plan, smoothed):
    """every level's arrays and sizes (and a smoothed plan's transfers) on the host"""
    out = []
    for l in range(plan.info()["levels"]):
        L = {k: (host(v) if hasattr(v, "cpu") else v) for k, v in plan.level(l).items()}
        if smoothed and l + 1 < plan.info()["levels"]:
            L.update({"t_" + k: (host(v) if hasattr(v, "cpu") else v) for k, v in plan.transfer(l).items()})
        out.append(L)
    return out


def assert_same_arrays(A, B, keys=None, what=None):
    assert len(A) == len(B), what
    for l, (La, Lb) in enumerate(zip(A, B)):
        assert La.keys() == Lb.keys()
        for k in La:
            if keys is not None and k not in keys:
                continue
            a, b = La[k], Lb[k]
            if isinstance(a, np.ndarray) and a.dtype == np.float64:
                assert same(a, b), (what, l, k)
            elif isinstance(a, np.ndarray):
                assert np.array_equal(a, b), (what, l, k)
            else:
                assert a == b or (a is None and b is None), (what, l, k)


INTEGERS = ("n", "nnz", "n_coarse", "units", "rowptr", "colidx", "agg", "aggptr", "members", "t_n", "t_n_coarse", "t_nnz", "t_p_rowptr", "t_p_colidx",
            "t_r_rowptr", "t_r_colidx")


@pytest.mark.parametrize("name,kind", PLANS)
def test_a_device_plan_is_the_host_plan(env, name, kind):
    S, torch, cuda = env
    c = SA.case(name)
    n, theta = c["n"], c["theta"]
    drp, dci, dval = up(torch, cuda, c["rp"], c["ci"], c["val"])
    kw = dict(val=dval if theta > 0.0 else None, theta=theta, prolongator=kind)
    plans = {mode: S.AmgPlan(n, drp, dci, aggregation=mode, **kw) for mode in ("host", "device")}
    H, D = plans["host"], plans["device"]
    smoothed = kind == "smoothed"
    strip = lambda info: {k: v for k, v in info.items() if k not in ("aggregation", "bytes")}
    print("%s %s: levels %s, %d / %d bytes" % (name, kind, D.levels(), H.info()["bytes"], D.info()["bytes"]))
    assert H.info()["aggregation"] == "host" and D.info()["aggregation"] == "device"
    assert H.levels() == D.levels() and strip(H.info()) == strip(D.info()) and H.info()["levels"] >= (1 if name == "star5000" and smoothed else 2)
    assert_same_arrays(plan_arrays(torch, H, smoothed), plan_arrays(torch, D, smoothed), INTEGERS, (name, kind, "create"))
    r, = up(torch, cuda, np.random.default_rng(5).standard_normal(n))
    for values in (c["val"], c["val"] * (1.0 + 0.25 * np.sin(np.arange(len(c["val"]))))):
        dv, = up(torch, cuda, values)
        H.setup(dv), D.setup(dv)
        assert strip(H.info()) == strip(D.info()) and H.check() == D.check()
        assert_same_arrays(plan_arrays(torch, H, smoothed), plan_arrays(torch, D, smoothed), None, (name, kind, "setup"))
        assert same(host(H.apply(r)), host(D.apply(r))), (name, kind)
    for p in plans.values():
        p.destroy()


@pytest.mark.parametrize("name,kind", [("grid32", "plain"), ("grid32", "smoothed"), ("aniso32", "plain"), ("random600", "smoothed")])
def test_apply_replays_from_a_graph_after_a_second_setup(env, name, kind):
    S, torch, cuda = env
    c = SA.case(name)
    n, theta = c["n"], c["theta"]
    drp, dci, dval = up(torch, cuda, c["rp"], c["ci"], c["val"])
    kw = dict(val=dval if theta > 0.0 else None, theta=theta, prolongator=kind)
    H, D = S.AmgPlan(n, drp, dci, aggregation="host", **kw), S.AmgPlan(n, drp, dci, aggregation="device", **kw)
    r, = up(torch, cuda, np.random.default_rng(6).standard_normal(n))
    dv = dval.clone()
    H.setup(dv), D.setup(dv)
    z = torch.zeros(n, dtype=torch.float64, device=cuda)
    D.apply(r, out=z)                                                        # eager first: loads the code objects
    assert same(host(z), host(H.apply(r)))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            D.apply(r, out=z, stream=s)
    dv.copy_(up(torch, cuda, c["val"] * (1.0 + 0.1 * np.cos(np.arange(len(c["val"])))))[0])
    H.setup(dv), D.setup(dv)                                                 # the same pointer, new values: every level follows
    z.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    want = host(H.apply(r))
    assert same(host(z), want) and same(host(D.apply(r)), want), (name, kind)
    H.destroy(), D.destroy()


def test_the_guard_keeps_the_star_at_one_level_in_both_modes(env):
    S, torch, cuda = env
    c = SA.case("star5000")
    drp, dci, dval = up(torch, cuda, c["rp"], c["ci"], c["val"])
    r, = up(torch, cuda, np.random.default_rng(5).standard_normal(c["n"]))
    for kind in ("plain", "smoothed"):
        out = []
        for mode in ("host", "device"):
            plan = S.AmgPlan(c["n"], drp, dci, prolongator=kind, min_reduction=0.2, aggregation=mode)
            assert plan.levels() == [(5000, len(c["ci"]))] and plan.info()["min_reduction"] == 0.2 and plan.level(0)["agg"] is None
            plan.setup(dval)
            out.append(host(plan.apply(r)))
            plan.destroy()
        assert same(out[0], out[1])


# ---------------------------------------------------------------------------------------------------------------------
# in PCG
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,iterations", [("plain", 32), ("smoothed", 12)])
def test_pcg_takes_the_host_plans_iterations_and_bits(env, kind, iterations):
    S, torch, cuda = env
    n, rp, ci, val = KN.laplacian(32)
    drp, dci, dval = up(torch, cuda, rp.astype(np.int32), ci.astype(np.int32), val)
    db, = up(torch, cuda, np.random.default_rng(30).standard_normal(n))
    got = {}
    for mode in ("host", "device"):
        amg = S.AmgPlan(n, drp, dci, prolongator=kind, aggregation=mode)
        amg.setup(dval)
        plan = S.KrylovPlan(n, drp, dci, method="pcg", precond=amg)
        x, st = plan.solve(dval, db, rtol=RTOL, max_iter=1000)
        got[mode] = (host(x), st)
        plan.destroy(), amg.destroy()
    (xh, sh), (xd, sd) = got["host"], got["device"]
    print("PCG with %s AMG: %d iterations with the host's aggregation, %d with the device's" % (kind, sh["iterations"], sd["iterations"]))
    assert sh["status"] == sd["status"] == "converged"
    assert sh["iterations"] == sd["iterations"] == iterations
    assert sd == sh and same(xd, xh)


# ---------------------------------------------------------------------------------------------------------------------
# the refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_name_the_host_modes_row(env):
    S, torch, cuda = env
    E = S.SblasError
    c = AN.case("grid24")
    n, rp, ci, val = c["n"], c["rp"], c["ci"], c["val"]
    drp, dci, dval = up(torch, cuda, rp, ci, val)
    swapped = ci.copy()
    swapped[rp[5]], swapped[rp[5] + 1] = ci[rp[5] + 1], ci[rp[5]]
    no_diag = ci.copy()
    no_diag[rp[9]:rp[10]][ci[rp[9]:rp[10]] == 9] = 8
    outside = ci.copy()
    outside[rp[30]] = n
    short = rp.copy()
    short[-1] -= 1
    for bad_rp, bad_ci in ((rp, swapped), (rp, no_diag), (rp, outside), (short, ci)):
        brp, bci = up(torch, cuda, bad_rp, bad_ci)
        rows = []
        for mode in ("host", "device"):
            with pytest.raises(E) as err:
                S.AmgPlan(n, brp, bci, aggregation=mode)
            rows.append((err.value.bad_row, str(err.value).split("failed")[1]))
        assert rows[0] == rows[1] and rows[0][0] >= 0, rows
        with pytest.raises(E) as err:                                         # the stand-alone wrapper checks before it launches
            S.amg_aggregate_device(n, brp, bci)
        assert err.value.bad_row == rows[0][0]
    for call in (lambda: S.AmgPlan(n, drp, dci, aggregation="gpu"), lambda: S.AmgPlan(n, drp, dci, theta=0.25, aggregation="device"),
                 lambda: S.AmgPlan(n, drp, dci, val=dval, theta=float("nan"), aggregation="device"),
                 lambda: S.AmgPlan(n, drp, dci, val=dval, theta=1.5, aggregation="device"),
                 lambda: S.amg_aggregate_device(n, drp, dci, None, 0.25), lambda: S.amg_aggregate_device(n, drp, dci, dval, float("nan")),
                 lambda: S.amg_aggregate_device(n + 1, drp, dci), lambda: S.amg_aggregate_device(n, rp, ci)):
        with pytest.raises(E):
            call()
    # the C entry points: the same codes as the host mode, and nothing written
    L = S.lib()
    h, row = ctypes.c_void_p(), ctypes.c_int64(-1)
    create = lambda mode, theta, v, kind=0, w=0.0, m=0.0: L.sblas_hip_amg_plan_create_dev(
        -1, None, n, len(ci), drp.data_ptr(), dci.data_ptr(), v, theta, 0, 0, 0, kind, w, m, mode, ctypes.byref(h), ctypes.byref(row))
    for args in ((0.25, None), (float("nan"), dval.data_ptr()), (-0.5, dval.data_ptr()), (0.0, None, 2), (0.0, None, 1, 0.0, 0.2), (0.0, None, 0, 0.0, 1.0)):
        codes = [create(mode, *args) for mode in (0, 1)]
        assert codes[0] == codes[1] != 0 and not h.value, args
    assert create(2, 0.0, None) != 0 and create(-1, 0.0, None) != 0 and not h.value
    guard = torch.full((n + 1,), -7, dtype=torch.int32, device=cuda)
    ws = torch.zeros(S.lib().sblas_hip_amg_aggregate_workspace(n, len(ci)) + 16, dtype=torch.uint8, device=cuda)
    n_agg, rounds = ctypes.c_int64(9), ctypes.c_int64(9)
    agg_call = lambda theta, v, wsp, wsb, nn=n, nz=len(ci): L.sblas_hip_amg_aggregate_i32(
        -1, None, nn, nz, drp.data_ptr(), dci.data_ptr(), v, theta, 0, 0, guard.data_ptr(), guard.data_ptr(), guard.data_ptr(), wsp, wsb,
        ctypes.byref(n_agg), ctypes.byref(rounds))
    full = ws.numel() - 16
    assert agg_call(float("nan"), dval.data_ptr(), ws.data_ptr(), full) == 1 and agg_call(1.5, dval.data_ptr(), ws.data_ptr(), full) == 1
    assert agg_call(0.25, None, ws.data_ptr(), full) == 1
    assert agg_call(0.0, None, ws.data_ptr(), full - 1) == 3 and agg_call(0.0, None, None, full) == 3      # SBLAS_E_WORKSPACE
    assert agg_call(0.0, None, ws.data_ptr() + 4, full) == 1                                                 # not 16-byte aligned
    assert agg_call(0.0, None, ws.data_ptr(), full, nn=2 ** 31) == 1 and agg_call(0.0, None, ws.data_ptr(), full, nz=2 ** 31) == 1
    torch.cuda.synchronize()
    assert bool((guard == -7).all()) and bool((ws == 0).all()) and n_agg.value == 0 and rounds.value == 0


def test_the_host_mode_is_the_default_and_the_old_creates(env):
    """aggregation="device" is a TypeError on the parent commit: the argument is this feature's"""
    S, torch, cuda = env
    c = AN.case("grid24")
    drp, dci = up(torch, cuda, c["rp"], c["ci"])
    plans = [S.AmgPlan(c["n"], drp, dci), S.AmgPlan(c["n"], drp, dci, aggregation="host"), S.AmgPlan(c["n"], drp, dci, aggregation="device")]
    assert [p.info()["aggregation"] for p in plans] == ["host", "host", "device"]
    assert plans[0].info() == plans[1].info()
    opt = (ctypes.c_double * 4)()
    assert S.lib().sblas_hip_amg_plan_options(plans[2].handle, opt) == 0 and opt[3] == 1.0
    for p in plans:
        p.destroy()
