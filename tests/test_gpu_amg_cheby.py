"""The Chebyshev polynomial as the AMG plan's smoother on the device (amg.hip with cheby.hip's launches):
every level's estimate and table against the host reference, apply against the reference cycle for both prolongators and
both aggregation modes (eager and replayed from a graph), the way back to Jacobi and forth, the bytes of a plan that never
saw the smoother, the refusal of a first setup under capture, and the plan inside PCG against its composition.  Every
comparison of values is ==."""
import numpy as np
import pytest

import amg_numerics as AN
import cheby_numerics as CN
import krylov_numerics as KN
import solver_compose as SC

pytestmark = pytest.mark.gpu

RTOL = 1e-10
KINDS = [("plain", "host"), ("smoothed", "host"), ("plain", "device"), ("smoothed", "device")]


@pytest.fixture(scope="module")
def env(sblas, cuda):
    import torch
    return sblas, torch, cuda


def up(torch, cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def same(a, b):
    return KN.same_bits(a, b)


def download(plan):
    """the plan's hierarchy as the host references take it: the level arrays, and a smoothed plan's P and R"""
    out = []
    info = plan.info()
    for l in range(info["levels"]):
        L = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in plan.level(l).items() if v is not None}
        if info["prolongator"] == "smoothed" and l + 1 < info["levels"]:
            L.update({k: v.cpu().numpy() for k, v in plan.transfer(l).items() if hasattr(v, "cpu")})
        out.append(L)
    return out


def host_levels(S, H, degree, coarse_sweeps, seed=0, steps=10, boost=1.1, ratio=30.0):
    """the downloaded hierarchy with wd = 1 / a_ii, every level's estimate and table by the host reference"""
    def estimate_of(c, steps, boost, seed, level):
        E = S.cheby_lanczos_ref(c["n"], c["rp"], c["ci"], c["val"], eig_steps=steps, seed=seed, level=level)
        ritz = S.cheby_ritz_ref(E["alpha"], E["beta"])["ritz"] if E["m"] else 0.0
        g = S.cheby_rowbound_ref(c["n"], c["rp"], c["ci"], c["val"])
        return dict(m=E["m"], ritz=ritz, g=g, lambda_max=S.cheby_lambda_ref(E["m"], ritz, g, boost))
    W = CN.chebyshev_levels(H, degree, coarse_sweeps, steps, boost, ratio, seed, estimate_of)
    for L in W:                                                              # the tables by the C function, not the restatement
        L["table"] = S.cheby_coef_ref(L["eig"]["lambda_max"], degree=len(L["table"]), eig_ratio=ratio)["table"]
    return W


def reference(S, W, r, kind, **kw):
    return (S.amg_cycle_sa_ref if kind == "smoothed" else S.amg_cycle_ref)(W, r, **kw)


@pytest.fixture(scope="module")
def plans(env):
    """grid24 (and clique130, whose rows take 64 lanes) in the four kinds, made once"""
    S, torch, cuda = env
    made = {}

    def get(name, kind, aggregation):
        key = (name, kind, aggregation)
        if key not in made:
            c = AN.case(name)
            drp, dci, dval = up(torch, cuda, c["rp"], c["ci"], c["val"])
            made[key] = dict(c=c, drp=drp, dci=dci, dval=dval, plan=S.AmgPlan(c["n"], drp, dci, prolongator=kind, aggregation=aggregation))
        return made[key]
    yield get
    for b in made.values():
        b["plan"].destroy()


@pytest.mark.parametrize("kind,aggregation", KINDS)
def test_every_level_and_apply_equal_the_reference(env, plans, kind, aggregation):
    S, torch, cuda = env
    for name in ("grid24", "clique130") if aggregation == "host" else ("grid24",):
        B = plans(name, kind, aggregation)
        plan, n = B["plan"], B["c"]["n"]
        r = np.random.default_rng(5).standard_normal(n)
        dr, = up(torch, cuda, r)
        for nu, degree, coarse, scale in ((1, 2, 8, 1.0), (2, 3, 3, 1.5), (1, 3, 8, 1.0), (2, 2, 5, 1.0)):
            plan.setup(B["dval"], smoother="chebyshev", nu=nu, degree=degree, coarse_sweeps=coarse, coarse_scale=scale)
            info = plan.info()
            H = download(plan)
            W = host_levels(S, H, degree, coarse)
            eig = plan.eig()
            assert len(eig) == len(W) == info["levels"]
            for l, (E, L) in enumerate(zip(eig, W)):
                assert E["m"] == L["eig"]["m"] and same(E["ritz"], L["eig"]["ritz"]) and same(E["g"], L["eig"]["g"]), (name, l, E, L["eig"])
                assert same(E["lambda_max"], L["eig"]["lambda_max"]) and same(E["table"], L["table"]), (name, l)
                assert same(H[l]["wd"], L["wd"])                             # wd holds 1 / a_ii
            z = plan.apply(dr)
            z2 = torch.full((n,), -7.0, dtype=torch.float64, device=cuda)
            assert plan.apply(dr, out=z2) is z2
            want = reference(S, W, r, kind, nu=nu, coarse_sweeps=coarse, coarse_scale=scale, degree=degree)
            assert same(z.cpu().numpy(), want) and same(z2.cpu().numpy(), want), (name, kind, aggregation, nu, degree)
            assert info["smoother"] == "chebyshev" and info["launches"] == CN.launches(len(W), nu, degree, coarse) == S.amg_launches(len(W), nu, coarse, degree)
            assert plan.check() is None and same(dr.cpu().numpy(), r)
        print("%s %s %s: levels %s, lambda_max %s" % (name, kind, aggregation, plan.levels(), [round(E["lambda_max"], 6) for E in eig]))


@pytest.mark.parametrize("kind", ["plain", "smoothed"])
def test_apply_replays_in_a_graph_after_a_new_setup(env, plans, kind):
    S, torch, cuda = env
    B = plans("grid24", kind, "host")
    plan, n = B["plan"], B["c"]["n"]
    r = np.random.default_rng(6).standard_normal(n)
    dr, = up(torch, cuda, r)
    dval = B["dval"].clone()
    plan.setup(dval, smoother="chebyshev", degree=2)
    z = torch.zeros(n, dtype=torch.float64, device=cuda)
    plan.apply(dr, out=z)                                                    # eager first: loads the code objects
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            plan.setup(dval, smoother="chebyshev", degree=2, stream=s)       # a later setup allocates nothing: it may be captured
            plan.apply(dr, out=z, stream=s)
    dval.mul_(1.0 + 0.1 * torch.cos(torch.arange(len(dval), device=cuda, dtype=torch.float64)))
    torch.cuda.synchronize()
    z.fill_(-7.0)
    g.replay()
    torch.cuda.synchronize()
    got = z.cpu().numpy().copy()
    W = host_levels(S, download(plan), 2, 8)
    assert same(got, reference(S, W, r, kind, degree=2))
    assert same(plan.apply(dr).cpu().numpy(), got)
    plan.setup(B["dval"])


def test_chebyshev_then_jacobi_then_chebyshev_equal_fresh_plans(env, plans):
    S, torch, cuda = env
    B = plans("grid24", "plain", "host")
    plan, n = B["plan"], B["c"]["n"]
    dr, = up(torch, cuda, np.random.default_rng(8).standard_normal(n))
    for kw in (dict(smoother="chebyshev", degree=3), dict(), dict(smoother="l1", nu=2), dict(smoother="chebyshev", degree=2, nu=2), dict()):
        plan.setup(B["dval"], **kw)
        fresh = S.AmgPlan(n, B["drp"], B["dci"])
        fresh.setup(B["dval"], **kw)
        assert same(plan.apply(dr).cpu().numpy(), fresh.apply(dr).cpu().numpy()), kw
        assert plan.info()["launches"] == fresh.info()["launches"] and plan.info()["smoother"] == kw.get("smoother", "jacobi")
        fresh.destroy()


def plain_bytes(plan):
    """what a plain host-aggregated plan holds, by create's layout: the flag word, and a level's integers (units | dpos |
    agg | aggptr | members, each padded to 16 bytes) and doubles (wd, x0, [x1, b,] [res] padded to 256 bytes, [val])"""
    pad = lambda b, q: (b + q - 1) // q * q
    total, levels = 256, plan.info()["levels"]
    for l in range(levels):
        L = plan.level(l)
        n, nnz, nc, last = L["n"], L["nnz"], L["n_coarse"], l + 1 == levels
        total += pad(16 * L["units"], 16) + pad(4 * n, 16) + (0 if last else 2 * pad(4 * n, 16) + pad(4 * (nc + 1), 16))
        total += pad(8 * n, 256) * (2 + (2 if l > 0 else 0) + (0 if last else 1)) + (pad(8 * nnz, 256) if l > 0 else 0)
    return total


def test_a_plan_that_never_saw_the_smoother_holds_what_it_held(env, plans):
    S, torch, cuda = env
    B = plans("grid24", "plain", "host")
    n = B["c"]["n"]
    fresh = S.AmgPlan(n, B["drp"], B["dci"])
    before = fresh.info()["bytes"]
    assert before == plain_bytes(fresh)
    for kw in (dict(), dict(smoother="l1", nu=2)):
        fresh.setup(B["dval"], **kw)
        assert fresh.info()["bytes"] == before
    fresh.setup(B["dval"], smoother="chebyshev")
    pad = lambda b: (b + 255) // 256 * 256
    extra = 4 * pad(8 * n) + sum(pad(8 * ln) + pad(8 * S.cheby_limits()["block_slots"]) + pad(8 * -(-ln // S.krylov_limits()["cell"]))
                                 for ln, _ in fresh.levels())
    assert fresh.info()["bytes"] == before + extra
    fresh.setup(B["dval"])
    assert fresh.info()["bytes"] == before + extra                           # kept for the next Chebyshev setup
    fresh.destroy()


def test_the_first_chebyshev_setup_is_refused_under_capture(env, plans):
    S, torch, cuda = env
    B = plans("grid24", "plain", "host")
    n = B["c"]["n"]
    fresh = S.AmgPlan(n, B["drp"], B["dci"])
    fresh.setup(B["dval"])
    dr, = up(torch, cuda, np.ones(n))
    want = fresh.apply(dr).cpu().numpy()
    z = torch.zeros(n, dtype=torch.float64, device=cuda)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            with pytest.raises(S.SblasError, match="capturing a graph"):
                fresh.setup(B["dval"], smoother="chebyshev", stream=s)
            refused = S.lib().sblas_hip_amg_plan_setup_ex(fresh.handle, s.cuda_stream, B["dval"].data_ptr(), 2, 0.0, 1, 8, 1.0, 2, 10, 1.1, 30.0)
            fresh.apply(dr, out=z, stream=s)                                 # something to capture
    assert refused != 0                                                      # the C entry refuses by itself, before it allocates
    torch.cuda.synchronize()
    info = fresh.info()
    assert info["smoother"] == "jacobi" and info["ready"] and same(fresh.apply(dr).cpu().numpy(), want)   # the plan is as it was
    E = S.SblasError
    for kw in (dict(omega=0.5), dict(degree=0), dict(degree=65), dict(eig_steps=0), dict(eig_boost=0.5), dict(eig_ratio=1.0),
               dict(eig_ratio=float("nan")), dict(coarse_sweeps=65), dict(nu=0)):
        with pytest.raises(E):
            fresh.setup(B["dval"], smoother="chebyshev", **kw)
    with pytest.raises(E):
        fresh.eig()                                                          # no Chebyshev setup yet
    with pytest.raises(E):
        fresh.setup(B["dval"], smoother="ssor")
    assert fresh.info()["bytes"] == plain_bytes(fresh)                       # the refusals allocated nothing
    L = S.lib()
    assert L.sblas_hip_amg_plan_setup_ex(fresh.handle, None, B["dval"].data_ptr(), 2, 0.5, 1, 8, 1.0, 2, 10, 1.1, 30.0) != 0   # omega set
    assert L.sblas_hip_amg_plan_setup_ex(fresh.handle, None, B["dval"].data_ptr(), 3, 0.0, 1, 8, 1.0, 2, 10, 1.1, 30.0) != 0
    assert same(fresh.apply(dr).cpu().numpy(), want)
    fresh.destroy()


class Parts(SC.Parts):
    """solver_compose's parts with an AmgPlan whose smoother is the polynomial"""

    def __init__(self, env, n, rp, ci, val, kind, degree):
        self.kind, self.degree = kind, degree
        super().__init__(env, n, rp, ci, val, "amg_smoothed" if kind == "smoothed" else "amg", planned=False)

    def revalue(self, val):
        S, torch, cuda = self.env
        self.val = val
        self.dval, = up(torch, cuda, val)
        self.lu = self.dinv = self.ddinv = None
        self.amg.setup(self.dval, smoother="chebyshev", degree=self.degree)


@pytest.mark.parametrize("kind", ["plain", "smoothed"])
def test_pcg_with_the_smoother_equals_its_composition_and_the_host_count(env, kind):
    S, torch, cuda = env
    n, rp, ci, val = KN.laplacian(32)
    b = np.random.default_rng(30).standard_normal(n)
    P = Parts(env, n, rp, ci, val, kind, 2)
    x0 = 0.1 * np.random.default_rng(31).standard_normal(n)
    want_x, want_it, want_rnorm, want_status = SC.composed_pcg(P.matvec, P.apply, P.dot, b, x0, RTOL, 1000)
    plan = S.KrylovPlan(n, P.drp, P.dci, precond=P.amg)
    db, = up(torch, cuda, b)
    runs = []
    for every in (1, 7, 50):
        dx, = up(torch, cuda, x0)
        x, st = plan.solve(P.dval, db, x=dx, rtol=RTOL, max_iter=1000, check_every=every)
        runs.append((x.cpu().numpy(), st))
    x, st = runs[0]
    assert want_status == "converged" and (st["status"], st["iterations"]) == (want_status, want_it), st
    assert same(st["rnorm"], want_rnorm) and same(x, want_x)
    for x2, st2 in runs[1:]:
        assert st2 == st and same(x2, x)
    assert plan.info()["launches"] == S.krylov_launches("pcg", "amg", P.amg.info()["launches"])
    # from zero: the host float64 loop with the reference cycle takes the same count
    _, st0 = plan.solve(P.dval, db, rtol=RTOL, max_iter=1000)
    W = host_levels(S, download(P.amg), 2, 8)
    host_it, _ = AN.host_pcg(n, rp, ci, val, b, lambda r: reference(S, W, r, kind, degree=2), RTOL)
    print("PCG on 32^2 with %s aggregation and the Chebyshev smoother of degree 2: device %d iterations, host loop %d"
          % (kind, st0["iterations"], host_it))
    assert st0["status"] == "converged" and st0["iterations"] == host_it
    plan.destroy()
    P.destroy()
