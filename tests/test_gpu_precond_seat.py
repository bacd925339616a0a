"""The preconditioner seat under PCG, BiCGStab and GMRES (precond.h) on the 6 x 6 five-point Laplacian
(n = 36: ILU(0) has more than one level, the AMG plan two): every create-time refusal under every solver, through the C
entry points, and one accepted create per kind and solver whose info() names the kind and counts what the host rule
counts from the seated plan's own info().  No plan is ever passed under another kind's code."""
import ctypes as C

import numpy as np
import pytest

import krylov_numerics as KN

pytestmark = pytest.mark.gpu

INVALID = 1                                                                  # SBLAS_E_INVALID
NONE, JACOBI, ILU0, AMG, CHEBYSHEV = range(5)                                # SBLAS_PRECOND_*
SOLVERS = ["pcg", "bicgstab", "gmres"]
RESTART = 5


class Seats:
    def __init__(self, S, torch, cuda):
        self.n, rp, ci, val = KN.laplacian(6)
        self.drp, self.dci, self.dval = [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in (rp, ci, val)]
        self.nnz = len(ci)
        self.ilu = S.Ilu0Plan(self.n, self.drp, self.dci)
        self.lower, self.upper = self.ilu.solvers()
        self.amg = S.AmgPlan(self.n, self.drp, self.dci, coarse_max=8)
        self.amg.setup(self.dval)
        self.cheb = S.ChebyshevPlan(self.n, self.drp, self.dci)
        self.cheb.setup(self.dval)
        self.x = torch.full((self.n,), -7.0, dtype=torch.float64, device=cuda)   # the sentinel: no refusal launches anything


@pytest.fixture(scope="module")
def seats(sblas, cuda):
    import torch
    P = Seats(sblas, torch, cuda)
    assert P.lower.info()["levels"] > 1 and P.upper.info()["levels"] > 1 and P.amg.info()["levels"] >= 2
    yield P
    for plan in (P.cheb, P.amg, P.ilu):
        plan.destroy()


def raw_create(S, P, solver, precond, lower, upper, h):
    L = S.lib()
    tail = (None, precond, lower, upper, C.byref(h))
    if solver == "gmres":
        return L.sblas_hip_gmres_plan_create(-1, None, P.n, P.nnz, P.drp.data_ptr(), P.dci.data_ptr(), RESTART, *tail)
    method = {"pcg": 0, "bicgstab": 1}[solver]
    return L.sblas_hip_krylov_plan_create(-1, None, method, P.n, P.nnz, P.drp.data_ptr(), P.dci.data_ptr(), *tail)


@pytest.mark.parametrize("solver", SOLVERS)
def test_create_refuses_a_seat_that_does_not_fit_its_kind(sblas, seats, solver):
    import torch
    P = seats
    lo, up, amg, cheb = (q.handle for q in (P.lower, P.upper, P.amg, P.cheb))
    bad = [(AMG, amg, amg), (CHEBYSHEV, cheb, cheb),                         # a cycle or a polynomial with an upper plan
           (AMG, None, None), (CHEBYSHEV, None, None),                       # ... without its handle
           (ILU0, None, up), (ILU0, lo, None), (ILU0, None, None),           # ILU(0) without either solve
           (NONE, lo, None), (NONE, None, up), (NONE, lo, up),               # a plan where none is taken
           (JACOBI, lo, None), (JACOBI, None, up), (JACOBI, lo, up),
           (5, None, None), (-1, None, None)]                                # no such kind
    for precond, lower, upper in bad:
        h = C.c_void_p(0xdead)                                               # create writes NULL first
        rc = raw_create(sblas, P, solver, precond, lower, upper, h)
        assert rc == INVALID and not h.value, (solver, precond, lower is not None, upper is not None, rc, h.value)
    torch.cuda.synchronize()
    assert bool((P.x == -7.0).all())


@pytest.mark.parametrize("solver", SOLVERS)
def test_an_accepted_seat_names_its_kind_and_counts_as_the_host_rule(sblas, seats, solver):
    S, P = sblas, seats
    lower, upper = P.lower.info()["launches"], P.upper.info()["launches"]
    kinds = [(None, NONE, None, 0, 0), ("jacobi", JACOBI, "jacobi", 0, 0), (P.ilu, ILU0, "ilu0", lower, upper),
             ((P.lower, P.upper), ILU0, "ilu0", lower, upper), (P.amg, AMG, "amg", P.amg.info()["launches"], 0),
             (P.cheb, CHEBYSHEV, "chebyshev", P.cheb.info()["launches"], 0)]
    assert P.cheb.info()["launches"] == P.cheb.info()["degree"]
    for precond, code, name, lo, up in kinds:
        if solver == "gmres":
            plan = S.GmresPlan(P.n, P.drp, P.dci, restart=RESTART, precond=precond)
        else:
            plan = S.KrylovPlan(P.n, P.drp, P.dci, method=solver, precond=precond)
        try:
            info = plan.info()
            assert info["precond"] == name and plan.precond_kind == code and plan.precond is precond, (solver, name, info)
            if solver == "gmres":
                want = S.gmres_launches(RESTART, name, lo, up)
                got = dict(step=info["step_launches"], close=info["close_launches"], restart=info["restart_launches"], cycle=info["cycle_launches"])
                assert got == {k: want[k] for k in got}, (solver, name, got, want)
                assert info["vectors"] == RESTART + S.gmres_limits()["vectors_fixed"] + (name in ("ilu0", "amg", "chebyshev"))
            else:
                assert info["launches"] == S.krylov_launches(solver, name, lo, up), (solver, name, info)
                assert info["vectors"] == S.krylov_limits()[solver + "_vectors"] + (name in ("ilu0", "amg", "chebyshev"))
        finally:
            plan.destroy()
