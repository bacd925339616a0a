"""The host half of tools/fuzz_solvers.py, without a GPU: the generators of the seed that tests/test_gpu_fuzz_solvers.py
commits to are run as they are there, and

- every draw is sound: a pcg matrix is symmetric and strictly dominant (the doubled entries summed), the others strictly
  dominant by rows, a preconditioned pattern passes ilu0_numerics.check, the planted row has exactly the drawn length, the
  planted n is exact, an exact guess leaves b - A x0 = 0;
- the host loop converges in under HOST_LIMIT iterations on every drawn problem that is expected to converge, and on every
  drawn matrix once it has Jacobi (GMRES(1) apart): "converged" is a statement about the inputs;
- the host half of the census holds, and with the loops composed from host parts the cases that carry the residual bar
  are at least the census's share;
- every planted breakdown reaches its literal (status, name, iterations) under the host composition;
- every judge refuses a spoiled answer: x with one value moved by one ulp or two neighbours swapped, iterations +- 1,
  another status, rnorm one ulp off, and for the residual bar an x whose residual is twice the bound;
- the composed loops with host parts reproduce the literal counts the existing GPU tests record."""
import math

import numpy as np
import pytest

import ilu0_numerics as IN
import krylov_numerics as KN
import numerics as NM
import solver_compose as SC
import test_gpu_fuzz_solvers as G

OPS = ["pcg", "bicgstab", "gmres"]


@pytest.fixture(scope="module")
def fuzz(sblas):
    return G.load()


def problems(fuzz, op):
    for case in range(G.CASES):
        yield case, fuzz.DRAW[op](case, fuzz.case_rng(G.SEED, op, case), G.max_rows(op))


def summed(n, rp, ci, val):
    """the matrix with doubled entries added -> (keys row * n + col ascending, values)"""
    key = NM.row_of_entries(rp) * n + ci.astype(np.int64)
    uniq, inv = np.unique(key, return_inverse=True)
    return uniq, np.bincount(inv, val, minlength=len(uniq))


def assert_sound(fuzz, op, P):
    n, rp, ci, st = P["n"], P["rp"], P["ci"], P["st"]
    assert len(rp) == n + 1 and rp[0] == 0 and rp[-1] == len(ci) and (np.diff(rp) >= 0).all(), P["params"]
    assert len(ci) == 0 or (0 <= ci.min() and ci.max() < n), P["params"]
    assert all(len(v) == len(ci) for v in P["val"]) and len(P["b"]) == n, P["params"]
    if P["size"] is not None:
        assert n == P["size"] and st["plant"] is None, P["params"]
    if st["degenerate"]:
        assert P["precond"] is None, P["params"]
        return
    row = NM.row_of_entries(rp)
    assert (np.bincount(row[ci == row], minlength=n) == 1).all(), P["params"]          # one stored diagonal a row
    if st["plant"]:
        assert np.diff(rp.astype(np.int64))[P["planted_row"]] == st["plant"]["L"], P["params"]
        split = fuzz.S.SPMV_SPLIT_MIN
        assert st["plant"]["L"] == dict(below=split - 1, at=split, above=split + 1, far=2 * split + 3)[st["plant"]["rel"]], P["params"]
    if P["precond"] is not None:
        assert IN.check(n, rp, ci)[1] is None, P["params"]
    for val in P["val"]:
        assert np.isfinite(val).all()
        key, v = summed(n, rp, ci, val)
        r, c = key // n, key % n
        off = np.bincount(r, np.where(r == c, 0.0, np.abs(v)), minlength=n)
        assert (v[r == c] > off).all(), P["params"]                                    # strictly dominant, a positive diagonal
        if op == "pcg":
            mirror = np.searchsorted(key, c * n + r)
            assert (mirror < len(key)).all() and np.array_equal(key[mirror], c * n + r) and np.array_equal(v[mirror], v), P["params"]
    if P["x0_kind"] == "exact":
        assert not np.any(P["b"] - KN.matvec(n, rp, ci, P["val"][0], P["x0"])), P["params"]


def host_answer(fuzz, P, val, precond):
    """the case under the host composition: precond None or "jacobi" -> (the answer, rtol, atol, max_iter, expected)"""
    n, rp, ci = P["n"], P["rp"], P["ci"]
    dinv = 1.0 / val[ci == NM.row_of_entries(rp)] if precond == "jacobi" else None
    parts = fuzz.host_parts(n, rp, ci, val, dinv)
    loop = lambda rtol, atol, max_iter: fuzz.compose(P["op"], parts, P["b"], P["x0"], P["restart"], rtol, atol, max_iter)
    rtol, atol, max_iter, expected = fuzz.stopping(P, loop)
    return loop(rtol, atol, max_iter), rtol, atol, max_iter, expected


def refused(judge, *args):
    try:
        judge(*args)
    except AssertionError:
        return True
    return False


def one_ulp(a):
    a = np.array(a, np.float64)
    live = np.flatnonzero(np.isfinite(a.reshape(-1)))
    if len(live) == 0:
        return None
    i = live[len(live) // 2]
    a.reshape(-1)[i] = np.nextafter(a.reshape(-1)[i], np.inf)
    return a if a.ndim else float(a)


def neighbours_swapped(a):
    a = np.array(a)
    differ = np.flatnonzero((a[1:] != a[:-1]) & ~(np.isnan(a[1:]) & np.isnan(a[:-1])))       # two NaNs swapped are no change
    if len(differ) == 0:
        return None
    i = differ[len(differ) // 2]
    a[[i, i + 1]] = a[[i + 1, i]]
    return a


def spoiled_answers(want):
    """(what, answer) for every way of spoiling that applies"""
    for what, bad in (("ulp", one_ulp(want["x"])), ("swap", neighbours_swapped(want["x"]))):
        if bad is not None:
            yield what, dict(want, x=bad)
    yield "iterations", dict(want, iterations=want["iterations"] + 1)
    if want["iterations"] > 0:
        yield "iterations", dict(want, iterations=want["iterations"] - 1)
    yield "status", dict(want, status="limit" if want["status"] != "limit" else "converged")
    if np.isfinite(want["rnorm"]):
        yield "rnorm", dict(want, rnorm=one_ulp(want["rnorm"]))
    else:
        yield "rnorm", dict(want, rnorm=1.0)


@pytest.mark.parametrize("op", OPS)
def test_generated_cases_are_sound_and_spoiled_answers_refused(fuzz, op):
    seen, spoiled, bars, endings = [], {}, 0, set()
    for case, P in problems(fuzz, op):
        assert_sound(fuzz, op, P)
        seen.append(fuzz.census_of(P))
        if P["st"]["degenerate"] is None and not (op == "gmres" and P["restart"] == 1):
            # once it has Jacobi every drawn matrix is solved by the host loop in a few dozen iterations, both values
            for val in P["val"]:
                its, _ = fuzz.host_solution(dict(P, precond="jacobi"), val, fuzz.RTOL, 0.0)
                assert its < fuzz.HOST_LIMIT, (its, P["params"])
        if fuzz.expects_convergence(P):
            for val in P["val"]:                                             # inside the solver's allowance, with room
                its, _ = fuzz.host_solution(P, val, P["rtol"], P["atol"])
                assert its <= fuzz.MAX_ITER - 10 < fuzz.HOST_LIMIT, (its, P["params"])
        if P["precond"] not in (None, "jacobi"):
            continue
        # what the device meets, with host parts: the expectation of the regime, the bar, the judges
        want, rtol, atol, max_iter, expected = host_answer(fuzz, P, P["val"][0], P["precond"])
        fuzz.judge_expectation(P, want, expected)
        endings.add(want["status"])
        fuzz.JUDGE[op](P, want, want)
        for what, bad in spoiled_answers(want):
            assert refused(fuzz.JUDGE[op], P, bad, want), "a spoiled answer (%s) is accepted: %s" % (what, P["params"])
            spoiled[what] = spoiled.get(what, 0) + 1
        if fuzz.carries_the_bar(P, want):
            bars += 1
            val = P["val"][0]
            host_x = fuzz.host_solution(P, val, rtol, atol)[1]
            fuzz.judge_residual(P, val, want["x"], host_x, rtol, atol)
            # an x whose residual is twice the bound (and the rounding of x + s u): |A (s u)| = 2 bound + the residual x has
            bound = fuzz.residual_bound(P, val, host_x, rtol, atol)
            u = np.zeros(P["n"])
            u[P["n"] // 2] = 1.0
            Au = float(np.linalg.norm(KN.matvec(P["n"], P["rp"], P["ci"], val, u)))
            if bound > 0.0:
                bad = want["x"] + (2.0 * bound * (1.0 + 1e-6) + fuzz.true_residual(P, val, want["x"])) / Au * u
                assert 2.0 * bound <= fuzz.true_residual(P, val, bad) <= 2.0 * bound * (1.0 + 1e-5) + 2.0 * fuzz.true_residual(P, val, want["x"])
                assert refused(fuzz.judge_residual, P, val, bad, host_x, rtol, atol), "twice the residual bound is accepted: %s" % (P["params"],)
                spoiled["bound"] = spoiled.get("bound", 0) + 1
    G.host_census(fuzz, seen, op)
    assert bars >= G.BAR_CASES, bars
    assert endings == {"converged", "limit", "breakdown"}, endings
    for what in ("ulp", "swap", "iterations", "status", "rnorm", "bound"):
        assert spoiled.get(what, 0) >= 10, (what, spoiled)


def test_the_turns_have_no_common_factor_and_fit_a_run(fuzz):
    lengths = sorted(len(v) for v in fuzz.TURNS.values())
    assert all(math.gcd(a, b) == 1 for i, a in enumerate(lengths) for b in lengths[i + 1:]), lengths
    assert max(lengths) <= fuzz.RUN == G.CASES
    for start in (0, 17, 1000):                                              # any RUN consecutive cases meet every value
        met = [fuzz.turn(k) for k in range(start, start + fuzz.RUN)]
        assert {t["precond"] for t in met} == set(fuzz.PRECONDS) and {t["planned"] for t in met} == {True, False}
        assert {t["size"] for t in met} == set(fuzz.SIZES) | {None} and {t["restart"] for t in met} == set(fuzz.RESTARTS)
        assert {t["regime"] for t in met} == set(fuzz.REGIMES) and {t["check_every"] for t in met} == set(fuzz.CHECK_EVERY)
        assert {t["x0"] for t in met} == set(fuzz.X0_KINDS) and {t["b"] for t in met} == set(fuzz.B_KINDS)
    lim = fuzz.S.gmres_limits()
    assert {lim["dot_group"] - 1, lim["dot_group"], lim["dot_group"] + 1, 1, lim["max_restart"] - 1, lim["max_restart"]} <= set(fuzz.RESTARTS)
    assert fuzz.SIZES == [KN.CELL - 1, KN.CELL, KN.CELL + 1, 2 * KN.CELL + 5]


def test_case_k_is_a_function_of_seed_operation_and_k_alone(fuzz):
    for op in OPS:
        first = [fuzz.DRAW[op](case, fuzz.case_rng(G.SEED, op, case), G.max_rows(op))["params"] for case in range(4, 8)]
        again = fuzz.DRAW[op](6, fuzz.case_rng(G.SEED, op, 6), G.max_rows(op))["params"]
        assert again == first[2]
        assert fuzz.DRAW[op](6, fuzz.case_rng(G.SEED + 1, op, 6), G.max_rows(op))["params"] != first[2]


def test_every_planted_breakdown_reaches_its_literal(fuzz):
    named = set()
    for plant in fuzz.PLANTS:
        want = fuzz.host_plant(plant)
        fuzz.judge_plant(plant, want)
        assert (want["status"], want["breakdown"], want["iterations"]) == plant["expect"]
        named.add((plant["op"], want["breakdown"]))
        assert refused(fuzz.judge_plant, plant, dict(want, iterations=want["iterations"] + 1))
        assert refused(fuzz.judge_plant, plant, dict(want, breakdown="(p, q)" if want["breakdown"] != "(p, q)" else "rho"))
    assert named >= {("pcg", "(p, q)"), ("pcg", "rho"), ("bicgstab", "(r^, v)"), ("bicgstab", "(t, t)"), ("bicgstab", "omega"),
                     ("bicgstab", "rho"), ("bicgstab", None), ("gmres", "givens"), ("gmres", "beta")}
    assert set(n for _, n in named if n) == {v for v in fuzz.S.GMRES_DENOM.values() if v}       # every denominator either solver names
    both = fuzz.host_plant(next(p for p in fuzz.PLANTS if p["name"] == "bicgstab rho before omega"))
    assert both["breakdown"] == "rho" and both["omega"] == 0.0              # omega is bad too: the name shows which test comes first
    clause = fuzz.host_plant(next(p for p in fuzz.PLANTS if p["name"] == "bicgstab omega = 0"))
    assert clause["omega"] == 0.0 and clause["alpha"] == 1.0 and np.array_equal(clause["x"], [1.0, 1.0])


def diagonal(d):
    n = len(d)
    return n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.asarray(d, np.float64)


def test_the_composed_loops_with_host_parts_reproduce_the_recorded_counts(fuzz):
    """the literals tests/test_gpu_krylov.py and tests/test_gpu_gmres.py hold the device to, where every operation is exact"""
    parts = lambda A: fuzz.host_parts(*A)
    # diag(1, 0, 1, 0) x = 1: PCG breaks down on (p, q) after one iteration with x = 2, |r| = 2, alpha = 2, beta = 1
    A = diagonal([1.0, 0.0, 1.0, 0.0])
    r = SC.composed_pcg(*parts(A)[:3], np.ones(4), np.zeros(4), 1e-8, 50)
    assert (r.status, r.breakdown, r.iterations, r.rnorm, r.alpha, r.beta) == ("breakdown", "(p, q)", 1, 2.0, 2.0, 1.0)
    assert np.array_equal(r.x, np.full(4, 2.0)) and tuple(r) [1:] == (1, 2.0, "breakdown")
    # ... and GMRES on (givens) after one column
    g = SC.composed_gmres(*parts(A), np.ones(4), np.zeros(4), 30, 1e-8, 50)
    assert (g["status"], g["breakdown"], g["iterations"], g["columns"]) == ("breakdown", "givens", 1, 1)
    # A = 0: BiCGStab's first (r^, v) is 0
    A0 = diagonal([0.0, 0.0, 0.0])
    r = SC.composed_bicgstab(*parts(A0)[:3], np.ones(3), np.zeros(3), 1e-8, 50)
    assert (r.status, r.breakdown, r.iterations) == ("breakdown", "(r^, v)", 0) and not r.x.any()
    # n == 1: 2 x = 3 in one iteration, x = 1.5; GMRES by the lucky breakdown, |r| = 0
    A1 = diagonal([2.0])
    for loop in (SC.composed_pcg, SC.composed_bicgstab):
        r = loop(*parts(A1)[:3], np.array([3.0]), np.zeros(1), 1e-8, 1000)
        assert (r.status, r.iterations, r.x[0]) == ("converged", 1, 1.5)
    g = SC.composed_gmres(*parts(A1), np.array([3.0]), np.zeros(1), 30, 1e-8, 1000)
    assert (g["status"], g["iterations"], g["rnorm"], g["x"][0]) == ("converged", 1, 0.0, 1.5)
    # b == 0: x = 0 at iteration 0 whatever the guess; max_iter == 0 with work to do: the limit at 0 and x untouched
    n, rp, ci, val = KN.laplacian(8)
    L = fuzz.host_parts(n, rp, ci, val)
    x0 = np.full(n, -7.0)
    for loop in (SC.composed_pcg, SC.composed_bicgstab):
        r = loop(*L[:3], np.zeros(n), x0, 1e-8, 1000)
        assert (r.status, r.iterations, r.rnorm, r.bnorm, r.alpha, r.beta) == ("converged", 0, 0.0, 0.0, 0.0, 0.0) and not r.x.any()
        r = loop(*L[:3], np.ones(n), x0, 1e-8, 0)
        assert (r.status, r.iterations) == ("limit", 0) and np.array_equal(r.x, x0)
    g = SC.composed_gmres(*L, np.ones(n), x0, 5, 1e-8, 0)
    assert (g["status"], g["iterations"], g["restarts"], g["columns"]) == ("limit", 0, 0, 0) and np.array_equal(g["x"], x0)
    # the guess is the solution: small integers, b = A x exact, converged at iteration 0 with |r| = 0
    xs = np.random.default_rng(5).integers(-8, 9, n).astype(np.float64)
    for loop in (SC.composed_pcg, SC.composed_bicgstab):
        r = loop(*L[:3], KN.matvec(n, rp, ci, val, xs), xs, 1e-8, 1000)
        assert (r.status, r.iterations, r.rnorm) == ("converged", 0, 0.0) and np.array_equal(r.x, xs)
    # GMRES(5) on the 24 x 24 convection-diffusion grid stopped at 7 steps: a full cycle, a restart, two columns
    n, rp, ci, val = KN.convection_diffusion(24)
    rng = np.random.default_rng(30)
    b, x0 = rng.standard_normal(n), 0.1 * rng.standard_normal(n)
    g = SC.composed_gmres(*fuzz.host_parts(n, rp, ci, val), b, x0, 5, 1e-10, 7)
    assert (g["status"], g["iterations"], g["restarts"], g["columns"]) == ("limit", 7, 1, 2)


def test_the_tolerance_follows_the_fold(fuzz):
    """tol = t if t >= atol else atol with t = rtol |b|: atol governs when it is the larger, alone when rtol = 0, and a
    NaN t (a non-finite b) leaves atol"""
    assert SC.tolerance(1e-10, 0.0, 2.0) == 2e-10 and SC.tolerance(1e-10, 1e-6, 2.0) == 1e-6 and SC.tolerance(0.0, 1e-8, 2.0) == 1e-8
    assert SC.tolerance(1e-10, 0.5, float("nan")) == 0.5 and SC.tolerance(0.0, 0.0, 5.0) == 0.0
    n, rp, ci, val = KN.laplacian(8)
    L = fuzz.host_parts(n, rp, ci, val)
    b = np.random.default_rng(1).standard_normal(n)
    tight = SC.composed_pcg(*L[:3], b, np.zeros(n), 1e-10, 1000)
    loose = SC.composed_pcg(*L[:3], b, np.zeros(n), 1e-10, 1000, atol=1e-3 * tight.bnorm)
    alone = SC.composed_pcg(*L[:3], b, np.zeros(n), 0.0, 1000, atol=1e-3 * tight.bnorm)
    assert loose.status == alone.status == "converged" and loose.iterations == alone.iterations < tight.iterations
    assert loose.rnorm > 1e-10 * loose.bnorm and KN.same_bits(loose.x, alone.x)
