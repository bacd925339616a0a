"""The host side of the Chebyshev plan (cheby_rule.cpp through the C ABI): the start vector, the Lanczos
recurrence, the tridiagonal and its Ritz value, the row bound, lambda_max, the coefficient table and the polynomial against
the Python restatements of cheby_numerics with ==; the Ritz value against numpy's eigenvalues, lambda_max against the true
one, the polynomial's symmetry, the iteration counts of a host float64 PCG, the launch counts and the refusals.  No GPU."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import amg_numerics as AN
import cheby_numerics as CN
import krylov_numerics as KN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(a, b):
    return KN.same_bits(a, b)


@pytest.fixture(scope="module")
def restated():
    """every case's estimate by the Python restatement, computed once"""
    made = {}

    def get(name, seed=0):
        if (name, seed) not in made:
            made[name, seed] = CN.estimate(CN.case(name), seed=seed)
        return made[name, seed]
    return get


def test_the_library_exports_what_the_new_header_declares(sblas):
    hdr = open(os.path.join(ROOT, "include", "sblas_hip_cheby.h")).read()
    declared = set(re.findall(r"\b(sblas_[A-Za-z0-9_]+)\s*\(", hdr))
    others = set(sblas.EXPORTS + sblas.EXPORTS_AMG_SA + sblas.EXPORTS_AMG_DEV)
    assert declared == set(sblas.EXPORTS_CHEBY) and not declared & others, declared ^ set(sblas.EXPORTS_CHEBY)
    assert '#include "sblas_hip_cheby.h"' in open(os.path.join(ROOT, "include", "sblas_hip.h")).read()
    for name in declared:
        assert hasattr(sblas.lib(), name), name
    lim = sblas.cheby_limits()
    assert (lim["max_degree"], lim["max_steps"], lim["degree"], lim["eig_steps"], lim["bisections"]) == (64, 64, CN.DEGREE, CN.STEPS, CN.BISECTIONS)
    assert sblas.PRECOND_CHEBYSHEV == 4


@pytest.mark.parametrize("name", CN.CASES)
def test_the_estimate_equals_the_restatement(sblas, restated, name):
    c = CN.case(name)
    n, rp, ci, val = c["n"], c["rp"], c["ci"], c["val"]
    for seed in (0, 5) if name in ("grid24", "tridiagonal3000", "indefinite2") else (0,):
        W = restated(name, seed)
        assert same(sblas.cheby_start_ref(n, seed=seed), CN.start(n, seed)) and same(sblas.cheby_start_ref(n, seed=seed - 2, level=2), CN.start(n, seed))
        b0 = CN.start(n, seed)
        assert n == 0 or (np.abs(b0).max() < 1.0 and np.abs(b0).min() > 0.0)
        got = sblas.cheby_lanczos_ref(n, rp, ci, val, seed=seed)
        assert got["m"] == W["m"] and same(got["alpha"], W["alpha"]) and same(got["beta"], W["beta"]) and got["bad_row"] is None, (name, seed)
        g = sblas.cheby_rowbound_ref(n, rp, ci, val)
        assert same(g, W["g"])
        ritz = 0.0
        if W["m"]:
            T = sblas.cheby_ritz_ref(got["alpha"], got["beta"])
            assert same(T["t"], W["t"]) and same(T["e2"], W["e2"]) and same(T["ritz"], W["ritz"]), (name, seed)
            ritz = T["ritz"]
            dense = np.diag(W["t"]) + np.diag(np.sqrt(W["e2"]), 1) + np.diag(np.sqrt(W["e2"]), -1)
            top = float(np.linalg.eigvalsh(dense)[-1])
            assert abs(ritz - top) <= 4.0 * np.spacing(top), (name, ritz, top)  # the bisection against numpy's eigenvalues of the same T
        lam = sblas.cheby_lambda_ref(got["m"], ritz, g)
        assert same(lam, W["lambda_max"])
        print("%s seed %d: m %d, Ritz %.6g, g %.6g, lambda_max %.6g" % (name, seed, W["m"], W["ritz"], W["g"], W["lambda_max"]))
    if name == "n0":
        assert W["m"] == 0 and W["g"] == 0.0
    if name == "n1":
        assert W["m"] == 1 and W["ritz"] == 1.0 and W["g"] == 1.0 and W["lambda_max"] == 1.0
    if name == "indefinite2":                                                # (p, q) < 0 at the first step or the second: the recurrence stops early
        assert W["m"] < CN.STEPS and W["g"] == 3.0
    if name == "random4000":                                                 # unsymmetric: the Ritz value overshoots and the row bound caps it
        assert W["lambda_max"] == W["g"] and CN.BOOST * W["ritz"] > W["g"]
    if c["symmetric"] and 0 < n <= 1024 and name != "indefinite2":
        true = CN.true_lambda_max(n, rp, ci, val)
        print("%s: boost * Ritz / true = %.3f, lambda_max / true = %.3f" % (name, CN.BOOST * W["ritz"] / true, W["lambda_max"] / true))
        assert W["lambda_max"] >= true, (name, W["lambda_max"], true)


@pytest.mark.parametrize("name", CN.CASES)
def test_the_table_and_the_polynomial_equal_the_restatement(sblas, restated, name):
    c = CN.case(name)
    n, rp, ci, val = c["n"], c["rp"], c["ci"], c["val"]
    lam = restated(name)["lambda_max"] if n else 2.0
    rng = np.random.default_rng(12)
    b, x = rng.standard_normal(n), rng.standard_normal(n)
    for degree in (1, 2, 3, 8):
        got = sblas.cheby_coef_ref(lam, degree=degree)
        table, low = CN.coefficients(lam, degree)
        assert same(got["table"], table) and same(got["lambda_min"], low), (name, degree)
        if name in ("star5000", "random4000", "tridiagonal3000") and degree == 3:   # the long Python loops once
            continue
        assert same(sblas.cheby_apply_ref(n, rp, ci, val, table, b), CN.apply(n, rp, ci, val, table, b)), (name, degree)
        assert same(sblas.cheby_apply_ref(n, rp, ci, val, table, b, x), CN.apply(n, rp, ci, val, table, b, x)), (name, degree)
    got = sblas.cheby_coef_ref(lam, degree=4, eig_ratio=10.0)
    table, low = CN.coefficients(lam, 4, 10.0)
    assert same(got["table"], table) and same(got["lambda_min"], low)


def grid(side):
    n, rp, ci, val = KN.laplacian(side)
    return n, rp.astype(np.int32), ci.astype(np.int32), val


def host_table(sblas, n, rp, ci, val, degree):
    L = sblas.cheby_lanczos_ref(n, rp, ci, val)
    lam = sblas.cheby_lambda_ref(L["m"], sblas.cheby_ritz_ref(L["alpha"], L["beta"])["ritz"], sblas.cheby_rowbound_ref(n, rp, ci, val))
    return sblas.cheby_coef_ref(lam, degree=degree)["table"]


def test_the_polynomial_is_symmetric_on_the_grid(sblas):
    """e_i' M^-1 e_j against e_j' M^-1 e_i over nine pairs, as the AMG tests do.  M^-1 = p(D^-1 A) D^-1 of degree 4 reaches
    three steps on the grid, so the pairs lie within three steps of each other: every entry compared is non-zero.  The two
    sides round in different orders; the bound is 2 ulps of the larger entry."""
    n, rp, ci, val = grid(24)
    table = host_table(sblas, n, rp, ci, val, 4)
    col = {}

    def column(j):
        if j not in col:
            e = np.zeros(n)
            e[j] = 1.0
            col[j] = sblas.cheby_apply_ref(n, rp, ci, val, table, e)
        return col[j]
    worst = 0.0
    for i, j in [(0, 1), (0, 24), (5, 7), (17, 18), (100, 124), (287, 263), (575, 574), (250, 253), (333, 358)]:
        a, b = column(j)[i], column(i)[j]
        worst = max(worst, abs(a - b) / np.spacing(max(abs(a), abs(b))))
        assert a != 0.0
    print("largest asymmetry: %.1f ulps" % worst)
    assert worst <= 2.0


def test_host_pcg_counts_fall_with_the_degree(sblas):
    """Host float64 PCG to 1e-10 on the 32^2 Laplacian, b from default_rng(30), with the C reference polynomial on the
    host estimate: DESIGN.md 3.27 records the counts this prints."""
    n, rp, ci, val = grid(32)
    b = np.random.default_rng(30).standard_normal(n)
    dinv = 1.0 / CN.diagonal(n, rp, ci, val)
    jacobi, _ = AN.host_pcg(n, rp, ci, val, b, lambda r: dinv * r, 1e-10)
    counts = {}
    for degree in (2, 4, 8):
        table = host_table(sblas, n, rp, ci, val, degree)
        it, x = AN.host_pcg(n, rp, ci, val, b, lambda r: sblas.cheby_apply_ref(n, rp, ci, val, table, r), 1e-10)
        assert np.linalg.norm(b - KN.matvec(n, rp, ci, val, x)) <= 1e-9 * np.linalg.norm(b)
        counts[degree] = it
    print("32^2: Jacobi %d, Chebyshev degree 2 / 4 / 8: %d / %d / %d" % (jacobi, counts[2], counts[4], counts[8]))
    assert jacobi == 115
    assert counts[2] > counts[4] > counts[8]
    assert 2 * counts[4] <= 115


def test_launch_counts_equal_a_hand_count(sblas):
    for degree in (1, 4, 64):
        assert sblas.krylov_launches("pcg", "chebyshev", degree) == 8 + degree           # the ILU(0) formulas, a polynomial as the M^-1
        assert sblas.krylov_launches("bicgstab", "chebyshev", degree) == 10 + 2 * degree
        g = sblas.gmres_launches(30, "chebyshev", degree)
        assert (g["step"], g["close"], g["restart"], g["start"]) == (9 + degree, 3 + degree, 4, 6) and g["cycle"] == 30 * (9 + degree) + 3 + degree + 4
    L = sblas.lib()
    out = (C.c_int64 * 4)()
    assert L.sblas_krylov_launches(0, 4, None, None) == -1 and L.sblas_gmres_launches(30, 4, None, None, out) == -1   # no info
    assert L.sblas_krylov_launches(0, 5, None, None) == -1 and L.sblas_gmres_launches(30, 5, None, None, out) == -1
    info = (C.c_int64 * 12)()
    info[5] = -1
    assert L.sblas_krylov_launches(0, 4, info, None) == -1 and L.sblas_gmres_launches(30, 4, info, None, out) == -1


def test_the_rule_check_runs_clean_under_the_sanitizers(tmp_path):
    """tools/cheby_rule_check.cpp, host code only and a program of its own, under the address and undefined-behaviour
    sanitizers of every host compiler there is"""
    found = [p for p in (shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++", shutil.which("g++")) if p and os.path.exists(p)]
    assert found, "no host compiler"
    csrc = os.path.join(ROOT, "s-blas_amd", "csrc")
    src = [os.path.join(ROOT, "tools", "cheby_rule_check.cpp")] + [os.path.join(csrc, f) for f in ("cheby_rule.cpp", "krylov_rule.cpp", "ilu0_plan.cpp")]
    for k, cxx in enumerate(found):
        exe = str(tmp_path / ("cheby_rule_check_%d" % k))
        subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-w", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                              + src + ["-o", exe])
        done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        assert done.returncode == 0, done.stdout.decode()
        assert b"cheby_rule_check: ok" in done.stdout


def test_refusals(sblas):
    S, E = sblas, sblas.SblasError
    c = CN.case("grid24")
    n, rp, ci, val = c["n"], c["rp"], c["ci"], c["val"]
    table = CN.coefficients(2.0, 3)[0]
    b = np.ones(n)
    nan, inf = float("nan"), float("inf")
    bad = [lambda: S.cheby_lanczos_ref(n, rp, ci, val, eig_steps=0), lambda: S.cheby_lanczos_ref(n, rp, ci, val, eig_steps=65),
           lambda: S.cheby_lanczos_ref(n, rp, ci, val, eig_steps=2.0), lambda: S.cheby_lanczos_ref(n, rp, ci, val[:-1]),
           lambda: S.cheby_lanczos_ref(n, rp[:-1], ci, val),
           lambda: S.cheby_ritz_ref([], []), lambda: S.cheby_ritz_ref(np.ones(65), np.ones(64)), lambda: S.cheby_ritz_ref(np.ones(3), np.ones(1)),
           lambda: S.cheby_lambda_ref(1, 1.0, 2.0, 0.5), lambda: S.cheby_lambda_ref(1, 1.0, 2.0, nan), lambda: S.cheby_lambda_ref(1, 1.0, 2.0, inf),
           lambda: S.cheby_coef_ref(2.0, degree=0), lambda: S.cheby_coef_ref(2.0, degree=65), lambda: S.cheby_coef_ref(2.0, degree=True),
           lambda: S.cheby_coef_ref(2.0, eig_ratio=1.0), lambda: S.cheby_coef_ref(2.0, eig_ratio=nan), lambda: S.cheby_coef_ref(2.0, eig_ratio=inf),
           lambda: S.cheby_coef_ref(nan),
           lambda: S.cheby_apply_ref(n, rp, ci, val, table[:0], b), lambda: S.cheby_apply_ref(n, rp, ci, val, table.ravel(), b),
           lambda: S.cheby_apply_ref(n, rp, ci, val, table, b[:-1]), lambda: S.cheby_apply_ref(n, rp, ci, val, table, b, b[:-1])]
    for k, call in enumerate(bad):
        with pytest.raises(E):
            call()
            pytest.fail("call %d was accepted" % k)
    no_diag = ci.copy()
    no_diag[rp[9]:rp[10]][ci[rp[9]:rp[10]] == 9] = 8
    for call in (lambda: S.cheby_lanczos_ref(n, rp, no_diag, val), lambda: S.cheby_rowbound_ref(n, rp, no_diag, val),
                 lambda: S.cheby_apply_ref(n, rp, no_diag, val, table, b)):
        with pytest.raises(E) as err:
            call()
        assert err.value.bad_row == 9
    # a diagonal that is not finite and > 0 is reported, not refused
    planted = val.copy()
    planted[rp[40]:rp[41]][ci[rp[40]:rp[41]] == 40] = -4.0
    assert S.cheby_lanczos_ref(n, rp, ci, planted)["bad_row"] == 40
    L = S.lib()
    y = np.zeros(n)
    args = (n, rp.ctypes.data, ci.ctypes.data, val.ctypes.data, table.ctypes.data, 3)
    assert L.sblas_cheby_apply_ref(*args, b.ctypes.data, None, b.ctypes.data, None) != 0       # y is b
    assert L.sblas_cheby_apply_ref(*args, b.ctypes.data, y.ctypes.data, y.ctypes.data, None) != 0   # y is x
    assert L.sblas_cheby_apply_ref(*args, b.ctypes.data, None, y.ctypes.data, None) == 0
    assert L.sblas_cheby_coef_ref(2.0, 30.0, 3, None, None) != 0 and L.sblas_cheby_limits(None) != 0
    assert L.sblas_cheby_ritz_ref(1, None, None, None, None, None) != 0
    # the plans refuse what is not a plan of theirs before any launch: no GPU is touched here
    for kind in (S.KrylovPlan, S.GmresPlan):
        for pre in ("chebyshev", "ssor", 4, 3, (None, None)):
            with pytest.raises(E):
                kind(n, rp, ci, precond=pre)
    with pytest.raises(E):
        S.pcg((n, rp, ci, val), b, precond="ssor")
    for kw in (dict(degree=0), dict(degree=65), dict(degree=2.0), dict(eig_steps=0), dict(eig_steps=65), dict(eig_boost=0.99), dict(eig_boost=nan),
               dict(eig_boost=inf), dict(eig_ratio=1.0), dict(eig_ratio=nan), dict(eig_ratio=inf)):
        with pytest.raises(E, match="must be"):
            S.ChebyshevPlan(n, rp, ci, **kw)
    h, row = C.c_void_p(), C.c_int64()
    create = lambda *opt: L.sblas_hip_cheby_plan_create(-1, None, 0, 0, None, None, *opt, 0, C.byref(h), C.byref(row))
    for opt in ((0, 10, 1.1, 30.0), (65, 10, 1.1, 30.0), (4, 0, 1.1, 30.0), (4, 65, 1.1, 30.0), (4, 10, 0.5, 30.0), (4, 10, nan, 30.0),
                (4, 10, 1.1, 1.0), (4, 10, 1.1, nan), (4, 10, 1.1, inf)):
        assert create(*opt) != 0 and not h.value, opt
    assert L.sblas_hip_cheby_plan_create(-1, None, 0, 0, None, None, 4, 10, 1.1, 30.0, 0, None, None) != 0


# ---------------------------------------------------------------------------------------------------------------------
# the polynomial as AMG's smoother
# ---------------------------------------------------------------------------------------------------------------------
def c_estimate(sblas):
    """cheby_numerics.estimate's result by the C functions (they equal the restatement: tested above)"""
    def estimate_of(c, steps, boost, seed, level):
        L = sblas.cheby_lanczos_ref(c["n"], c["rp"], c["ci"], c["val"], eig_steps=steps, seed=seed, level=level)
        ritz = sblas.cheby_ritz_ref(L["alpha"], L["beta"])["ritz"] if L["m"] else 0.0
        g = sblas.cheby_rowbound_ref(c["n"], c["rp"], c["ci"], c["val"])
        return dict(m=L["m"], ritz=ritz, g=g, lambda_max=sblas.cheby_lambda_ref(L["m"], ritz, g, boost))
    return estimate_of


@pytest.mark.parametrize("kind", ["plain", "smoothed"])
def test_the_chebyshev_cycle_reference_equals_the_restatement(sblas, kind):
    import amg_sa_numerics as SA
    for name in ("grid24", "clique130", "n1"):
        c = AN.case(name)
        H = SA.hierarchy(c, sblas.amg_aggregate, kind)
        r = np.random.default_rng(7).standard_normal(c["n"])
        ref = sblas.amg_cycle_sa_ref if kind == "smoothed" else sblas.amg_cycle_ref
        for nu in (1, 2):
            for degree in (1, 2, 3):
                coarse, scale = (8, 1.0) if nu == 1 else (3, 1.5)
                W = CN.chebyshev_levels(H, degree, coarse, estimate_of=CN.estimate if (nu, degree) == (1, 2) else c_estimate(sblas))
                got = ref(W, r, nu=nu, coarse_sweeps=coarse, coarse_scale=scale, degree=degree)
                assert same(got, CN.cycle_py(W, r, nu, degree, coarse, scale)), (name, kind, nu, degree)
                assert np.isfinite(got).all()
                assert sblas.amg_launches(len(W), nu, coarse, degree) == CN.launches(len(W), nu, degree, coarse)
        assert same(ref(H, r), ref(H, r, degree=0))                          # degree 0 is the sweeps' cycle, untouched
    assert sblas.amg_launches(3, 1, 8, 2) == 2 * (2 * 2 + 3) + 8 and sblas.amg_launches(1, 2, 5, 3) == 5 and sblas.amg_launches(0, 1, 8, 2) == 0
    for bad in ((3, 1, 65, 2), (3, 1, 8, 65), (3, 0, 8, 2), (3, 1, 8, -1)):
        with pytest.raises(sblas.SblasError):
            sblas.amg_launches(*bad)
    H = CN.chebyshev_levels(SA.hierarchy(AN.case("grid24"), sblas.amg_aggregate, kind), 2, 8, estimate_of=c_estimate(sblas))
    r = np.ones(576)
    for kw in (dict(degree=65), dict(degree=2, coarse_sweeps=65), dict(degree=2, nu=0)):
        with pytest.raises(sblas.SblasError):
            ref(H, r, **kw)
    with pytest.raises((sblas.SblasError, KeyError)):                        # no table
        ref([{k: v for k, v in L.items() if k != "table"} for L in H], r, degree=2)


def test_host_pcg_counts_of_amg_with_the_chebyshev_smoother(sblas):
    """Host float64 PCG to 1e-10 with the reference cycle of plain aggregation, b from default_rng(30): the Chebyshev smoother
    at degree 2 and 3 (nu = 1, the coarsest level a degree-8 polynomial) against the Jacobi smoother at nu = 2 and 3.
    DESIGN.md 3.27 records the counts this prints; the anisotropic case is recorded without a condition."""
    found = {}
    for name in ("grid24", "grid32", "aniso32"):
        c = AN.case(name)
        n, rp, ci, val = c["n"], c["rp"], c["ci"], c["val"]
        b = np.random.default_rng(30).standard_normal(n)
        H = AN.hierarchy(c, sblas.amg_aggregate)
        counts = {}
        for nu in (1, 2, 3):
            counts["jacobi%d" % nu] = AN.host_pcg(n, rp, ci, val, b, lambda r: sblas.amg_cycle_ref(H, r, nu=nu), 1e-10)[0]
        for degree in (2, 3, 4):
            W = CN.chebyshev_levels(H, degree, 8, estimate_of=c_estimate(sblas))
            it, x = AN.host_pcg(n, rp, ci, val, b, lambda r: sblas.amg_cycle_ref(W, r, degree=degree), 1e-10)
            assert np.linalg.norm(b - KN.matvec(n, rp, ci, val, x)) <= 1e-9 * np.linalg.norm(b)
            counts["chebyshev%d" % degree] = it
        print(name, counts)
        found[name] = counts
    for name in ("grid24", "grid32"):
        assert found[name]["chebyshev2"] < found[name]["jacobi2"] and found[name]["chebyshev3"] < found[name]["jacobi3"], found[name]
