"""The host side of the aggregation AMG plan (amg_rule.cpp through the C ABI): the pinned aggregation against a scalar
loop, the level sizes, the cycle reference against the Python restatement, the operator's symmetry, the refusals, the
limits and the launch counts.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import amg_numerics as AN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return {name: AN.case(name) for name in AN.CASES}


def values(c):
    return c["val"] if c["theta"] > 0.0 else None


@pytest.mark.parametrize("name", AN.CASES)
def test_aggregate_equals_the_scalar_loop(sblas, cases, name):
    c = cases[name]
    n, rp, ci = c["n"], c["rp"], c["ci"]
    for seed in (0, 1, 2):
        agg, aggptr, members = sblas.amg_aggregate(n, rp, ci, values(c), c["theta"], seed=seed)
        want_agg, want_ptr, want_members, root = AN.aggregate_py(n, rp, ci, values(c), c["theta"], seed=seed)
        assert np.array_equal(agg, want_agg) and np.array_equal(aggptr, want_ptr) and np.array_equal(members, want_members), (name, seed)
        # every vertex in exactly one aggregate
        assert np.array_equal(np.sort(members), np.arange(n)) and aggptr[0] == 0 and aggptr[-1] == n
        assert np.array_equal(np.bincount(agg, minlength=len(aggptr) - 1), np.diff(aggptr))
        strong = AN.strong_lists(n, rp, ci, values(c), c["theta"])
        roots = np.flatnonzero(root)
        assert len(roots) == len(aggptr) - 1 and np.array_equal(agg[roots], np.arange(len(roots)))
        for v in range(n):
            if not root[v]:                                                   # a non-root shares a strong entry of its own row with its root
                assert roots[agg[v]] in strong[v], (name, seed, v)
            elif c["symmetric"]:                                              # no two roots are strong neighbours
                assert not any(root[u] for u in strong[v]), (name, seed, v)
    if name == "aniso32":                                                     # aggregates lie along the strong direction: one grid row each
        agg = sblas.amg_aggregate(n, rp, ci, c["val"], c["theta"])[0]
        for a in range(agg.max() + 1):
            assert len(set(np.flatnonzero(agg == a) // 32)) == 1, a
    if name == "clique130":
        assert np.diff(sblas.amg_aggregate(n, rp, ci)[1]).max() == 130
    if name == "diagonal300":
        assert len(sblas.amg_aggregate(n, rp, ci)[1]) - 1 == n                # singletons: no level is made of them


def test_level_sizes_of_the_grids(sblas, cases):
    """integer outcomes of the rule; the CPU prototype of the design gave the same"""
    sizes = lambda name: [L["n"] for L in AN.hierarchy(cases[name], sblas.amg_aggregate)]
    assert sizes("grid24") == [576, 212, 57]
    assert sizes("grid32") == [1024, 378, 93, 24]
    assert sizes("grid24") == [L["n"] for L in AN.hierarchy(cases["grid24"], AN.aggregate_py)]
    assert sizes("diagonal300") == [300] and sizes("n1") == [1] and sizes("n0") == []


COMBOS = [(nu, sm, sc) for nu in (1, 2) for sm in ("jacobi", "l1") for sc in (1.0, 1.5)]


@pytest.mark.parametrize("name", AN.CASES)
def test_cycle_ref_equals_the_restatement(sblas, cases, name):
    c = cases[name]
    r = np.random.default_rng(7).standard_normal(c["n"])
    for nu, smoother, scale in (COMBOS if name in ("grid24", "grid32", "aniso32") else COMBOS[:1] + COMBOS[-1:]):
        H = AN.hierarchy(c, sblas.amg_aggregate, smoother=smoother)
        for L in H:                                                           # the library's wd is the restatement's
            wd, bad = sblas.amg_wd_ref(L["n"], L["rowptr"], L["colidx"], L["val"], smoother)
            assert bad == -1 and np.array_equal(wd, L["wd"])
        got = sblas.amg_cycle_ref(H, r, nu=nu, coarse_sweeps=8, coarse_scale=scale)
        want = AN.cycle_py(H, r, nu, 8, scale) if H else np.zeros(0)
        assert np.array_equal(got, want), (name, nu, smoother, scale)
        assert np.isfinite(got).all()


def test_the_operator_is_symmetric_on_the_grid(sblas, cases):
    """e_i' M^-1 e_j against e_j' M^-1 e_i.  The two sides round in different orders; on the reference the largest
    difference over these pairs is 2 ulps of the larger entry (measured), and the bound is 4 x that."""
    c = cases["grid24"]
    H = AN.hierarchy(c, sblas.amg_aggregate)
    col = {}

    def column(j):
        if j not in col:
            e = np.zeros(c["n"])
            e[j] = 1.0
            col[j] = sblas.amg_cycle_ref(H, e)
        return col[j]
    worst = 0.0
    for i, j in [(0, 1), (0, 24), (5, 300), (17, 18), (100, 124), (287, 288), (575, 0), (250, 251), (333, 40)]:
        a, b = column(j)[i], column(i)[j]
        worst = max(worst, abs(a - b) / np.spacing(max(abs(a), abs(b))))
        assert a != 0.0
    print("largest asymmetry: %.1f ulps" % worst)
    assert worst <= 8.0


def test_refusals_name_their_row(sblas, cases):
    c = cases["grid24"]
    n, rp, ci, val = c["n"], c["rp"], c["ci"], c["val"]
    swapped = ci.copy()
    swapped[rp[5]], swapped[rp[5] + 1] = ci[rp[5] + 1], ci[rp[5]]
    no_diag = ci.copy()
    no_diag[rp[9]:rp[10]][ci[rp[9]:rp[10]] == 9] = 8
    outside = ci.copy()
    outside[rp[30]] = n
    short = rp.copy()
    short[12] = short[11] - 1
    for bad_rp, bad_ci, row in ((rp, swapped, 5), (rp, no_diag, 9), (rp, outside, 30), (short, ci, 11)):
        with pytest.raises(sblas.SblasError) as err:
            sblas.amg_aggregate(n, bad_rp, bad_ci)
        assert err.value.bad_row == row and "row %d" % row in str(err.value)
    for theta in (-0.1, 1.5, float("nan")):
        with pytest.raises(sblas.SblasError):
            sblas.amg_aggregate(n, rp, ci, val, theta)
    with pytest.raises(sblas.SblasError):
        sblas.amg_aggregate(n, rp, ci, None, 0.25)                           # theta > 0 without values
    with pytest.raises(sblas.SblasError):
        sblas.amg_aggregate(n + 1, rp, ci)
    L = sblas.lib()
    out = C.c_int64()
    assert L.sblas_amg_aggregate(2**31, rp.ctypes.data, ci.ctypes.data, None, 0.0, 0, 0, None, None, None, C.byref(out), None) != 0
    zero = val.copy()
    zero[rp[7]:rp[8]][ci[rp[7]:rp[8]] == 7] = 0.0
    assert sblas.amg_wd_ref(n, rp, ci, zero)[1] == 7
    nan = val.copy()
    nan[rp[3]:rp[4]][ci[rp[3]:rp[4]] == 3] = np.nan
    assert sblas.amg_wd_ref(n, rp, ci, nan, "l1")[1] == 3
    with pytest.raises(sblas.SblasError):
        sblas.amg_wd_ref(n, rp, ci, val, "ssor")
    H = AN.hierarchy(c, sblas.amg_aggregate)
    for kw in (dict(nu=0), dict(coarse_sweeps=0)):
        with pytest.raises(sblas.SblasError):
            sblas.amg_cycle_ref(H, np.ones(n), **kw)
    with pytest.raises(sblas.SblasError):
        sblas.amg_cycle_ref(H, np.ones(n + 1))


def test_limits_are_the_headers(sblas):
    lim = sblas.amg_limits()
    text = open(os.path.join(ROOT, "s-blas_amd", "csrc", "amg.h")).read()
    solves = sblas.sptrsv_limits()
    assert (lim["g4_max"], lim["g16_max"]) == (AN.G4_MAX, AN.G16_MAX) == (solves["g4_max"], solves["g16_max"])
    for key, name in (("threads", "AMG_THREADS"), ("coarse_max", "AMG_COARSE_MAX"), ("max_levels", "AMG_MAX_LEVELS"), ("nu", "AMG_NU"),
                      ("coarse_sweeps", "AMG_COARSE_SWEEPS"), ("level_cap", "AMG_LEVEL_CAP")):
        assert "%s = %d;" % (name, lim[key]) in text, name
    assert (lim["coarse_max"], lim["max_levels"], lim["nu"], lim["coarse_sweeps"]) == (64, 20, 1, 8)
    assert sblas.lib().sblas_amg_limits(None) != 0


def test_launches_against_a_hand_count(sblas):
    assert sblas.amg_launches(0) == 0 and sblas.amg_launches(1) == 8 and sblas.amg_launches(4) == 3 * 5 + 8 == 23
    for levels in (1, 2, 3, 6, 20):
        for nu in (1, 2, 3):
            for cs in (1, 2, 8):
                assert sblas.amg_launches(levels, nu, cs) == AN.launches(levels, nu, cs)
    for bad in ((-1, 1, 8), (65, 1, 8), (3, 0, 8), (3, 1, 0)):
        with pytest.raises(sblas.SblasError):
            sblas.amg_launches(*bad)


def test_solver_launch_counts_with_amg(sblas):
    L = sblas.lib()
    info = (C.c_int64 * 12)()
    info[5] = 23
    out = (C.c_int64 * 4)()
    assert L.sblas_krylov_launches(0, 3, None, None) == -1 and L.sblas_krylov_launches(1, 3, None, None) == -1
    assert L.sblas_gmres_launches(30, 3, None, None, out) == -1
    assert L.sblas_krylov_launches(0, 3, info, None) == 8 + 23                # the ILU(0) formulas, a cycle as the M^-1
    assert L.sblas_krylov_launches(1, 3, info, None) == 10 + 2 * 23
    assert L.sblas_gmres_launches(30, 3, info, None, out) == 30 * (9 + 23) + (3 + 23) + 4
    assert list(out) == [9 + 23, 3 + 23, 4, 6]
    info[5] = -1
    assert L.sblas_krylov_launches(0, 3, info, None) == -1 and L.sblas_gmres_launches(30, 3, info, None, out) == -1
    assert sblas.krylov_launches("pcg", "amg", 23) == 31 and sblas.gmres_launches(30, "amg", 23)["step"] == 32
    with pytest.raises(sblas.SblasError):
        sblas.krylov_launches("pcg", "ssor")


def test_exports_name_the_amg_entries(sblas):
    header = open(os.path.join(ROOT, "include", "sblas_hip.h")).read()
    names = [e for e in sblas.EXPORTS if "amg" in e]
    assert len(names) == 16
    for name in names:
        assert name + "(" in header and hasattr(sblas.lib(), name), name


def test_the_rule_check_runs_clean_under_the_sanitizers(tmp_path):
    cxx = next((p for p in (shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++", shutil.which("g++")) if p and os.path.exists(p)), None)
    if cxx is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "amg_rule_check")
    src = [os.path.join(ROOT, "tools", "amg_rule_check.cpp"), os.path.join(ROOT, "s-blas_amd", "csrc", "amg_rule.cpp"),
           os.path.join(ROOT, "s-blas_amd", "csrc", "ilu0_plan.cpp")]
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                          + src + ["-o", exe])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert done.returncode == 0, done.stdout.decode()
    assert b"amg_rule_check: ok" in done.stdout
