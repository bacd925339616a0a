"""GMRES's host rule (gmres_rule.cpp; no GPU): the scalar step and the back substitution -- the very functions the
device compiles -- against their restatements in Python floats (tests/gmres_numerics.py), the limits against gmres.h,
the launch counts against a list written by hand, and the refusals of the Python layer that need no GPU."""
import os
import re

import numpy as np
import pytest

import gmres_numerics as GN
import krylov_numerics as KN
from conftest import ROOT


def random_state(j, seed):
    """a state step j can meet: j rotations with c^2 + s^2 = 1 (as rounded), g so far, a new column h and eta"""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0.0, 2.0 * np.pi, j)
    scale = 10.0 ** rng.integers(-3, 4)
    return dict(j=j, h=rng.standard_normal(j + 1) * scale, eta=abs(rng.standard_normal()) * scale, c=np.cos(ang), s=np.sin(ang),
                g=rng.standard_normal(j + 1))


def same_step(got, want):
    assert (got["status"], got["iterations"], got["breakdown"]) == (want["status"], want["iterations"], want["breakdown"]), (got, want)
    for key in ("h", "c", "s", "g"):
        assert KN.same_bits(got[key], want[key]), (key, got[key], want[key])
    if want["rcol"] is None:
        assert got["rcol"] is None and got["rnorm"] is None
    else:
        assert KN.same_bits(got["rcol"], want["rcol"]) and KN.same_bits(got["rnorm"], want["rnorm"])


@pytest.mark.parametrize("j", [0, 1, 5, 63])
def test_step_ref_is_the_written_order(sblas, j):
    for seed in range(4):
        st = random_state(j, 10 * j + seed)
        for tol, it, limit in ((0.0, 3, 1000), (1e300, 3, 1000), (0.0, 6, 7)):
            got = sblas.gmres_step_ref(st["j"], st["h"], st["eta"], st["c"], st["s"], st["g"], tol, iterations=it, max_iter=limit)
            want = GN.step_py(st["j"], st["h"], st["eta"], st["c"], st["s"], st["g"], tol, it, limit)
            same_step(got, want)
            assert got["status"] == ("converged" if tol > 0 else "limit" if limit == 7 else "running")
            assert got["iterations"] == it + 1
        assert len(got["c"]) == j + 1 and len(got["g"]) == j + 2 and len(got["rcol"]) == j + 1
        assert got["rcol"][j] > 0.0 and abs(got["c"][j] ** 2 + got["s"][j] ** 2 - 1.0) < 1e-15


@pytest.mark.parametrize("j", [0, 1, 5, 63])
def test_step_ref_edges(sblas, j):
    st = random_state(j, 77 + j)
    # eta == 0 with d != 0, the lucky breakdown: g_{j+1} = 0 meets any tolerance, 0 included
    got = sblas.gmres_step_ref(j, st["h"], 0.0, st["c"], st["s"], st["g"], 0.0, iterations=j, max_iter=1000)
    same_step(got, GN.step_py(j, st["h"], 0.0, st["c"], st["s"], st["g"], 0.0, j, 1000))
    assert (got["status"], got["rnorm"], got["iterations"]) == ("converged", 0.0, j + 1) and got["s"][j] == 0.0
    # d == 0: h rotates to a column whose last entry is 0 when h is 0, and eta is 0
    got = sblas.gmres_step_ref(j, np.zeros(j + 1), 0.0, st["c"], st["s"], st["g"], 1e300, iterations=j, max_iter=1000)
    same_step(got, GN.step_py(j, np.zeros(j + 1), 0.0, st["c"], st["s"], st["g"], 1e300, j, 1000))
    assert (got["status"], got["breakdown"], got["iterations"]) == ("breakdown", "givens", j)      # not counted
    assert KN.same_bits(got["c"], st["c"]) and KN.same_bits(got["s"], st["s"]) and KN.same_bits(got["g"], st["g"])
    # a NaN never converges, whatever the tolerance: in eta, in h, and an overflow of h_j h_j (d = inf)
    for h, eta in ((st["h"], float("nan")), (np.where(np.arange(j + 1) == j, np.nan, st["h"]), 1.0),
                   (np.where(np.arange(j + 1) == j, 1e200, st["h"]), 1.0)):
        got = sblas.gmres_step_ref(j, h, eta, st["c"], st["s"], st["g"], float("inf"), iterations=j, max_iter=1000)
        same_step(got, GN.step_py(j, h, eta, st["c"], st["s"], st["g"], float("inf"), j, 1000))
        assert (got["status"], got["breakdown"]) == ("breakdown", "givens")
    # a NaN that reaches g but not d: the step goes on, not converged
    g = st["g"].copy()
    g[j] = float("nan")
    got = sblas.gmres_step_ref(j, st["h"], st["eta"], st["c"], st["s"], g, float("inf"), iterations=0, max_iter=1000)
    same_step(got, GN.step_py(j, st["h"], st["eta"], st["c"], st["s"], g, float("inf"), 0, 1000))
    assert got["status"] == "running" and np.isnan(got["rnorm"])
    with pytest.raises(sblas.SblasError):
        sblas.gmres_step_ref(64, np.zeros(65), 1.0, np.zeros(64), np.zeros(64), np.zeros(65), 0.0)
    with pytest.raises(sblas.SblasError):
        sblas.gmres_step_ref(j, np.zeros(j + 2), 1.0, st["c"], st["s"], st["g"], 0.0)


def test_a_whole_cycle_of_steps_then_the_solve(sblas):
    """steps 0 .. m - 1 chained through the library and through Python, then R y = g: what a device cycle does in scalars"""
    m = 12
    rng = np.random.default_rng(4)
    lib_c, lib_s, lib_g = np.zeros(0), np.zeros(0), np.array([2.5])
    py_c, py_s, py_g = [], [], [2.5]
    R = np.zeros((m, m))
    for j in range(m):
        h, eta = rng.standard_normal(j + 1), abs(rng.standard_normal())
        got = sblas.gmres_step_ref(j, h, eta, lib_c, lib_s, lib_g, 0.0, iterations=j)
        want = GN.step_py(j, h, eta, py_c, py_s, py_g, 0.0, j, 1000)
        same_step(got, want)
        lib_c, lib_s, lib_g = got["c"], got["s"], got["g"]
        py_c, py_s, py_g = want["c"], want["s"], want["g"]
        R[:j + 1, j] = got["rcol"]
    for k in (1, 5, m):
        assert KN.same_bits(sblas.gmres_solve_ref(R[:k, :k], lib_g), GN.solve_py(R[:k, :k].tolist(), py_g)), k
    y = sblas.gmres_solve_ref(R, lib_g)
    assert np.allclose(R @ y, lib_g[:m], rtol=1e-9, atol=1e-12)              # and it is a solution


def test_solve_ref_edges(sblas):
    assert sblas.gmres_solve_ref(np.zeros((0, 0)), np.zeros(1)).shape == (0,)
    assert sblas.gmres_solve_ref([[4.0]], [3.0, 9.0])[0] == 0.75
    rng = np.random.default_rng(9)
    R = np.triu(rng.standard_normal((64, 64))) + 3.0 * np.eye(64)
    g = rng.standard_normal(65)
    assert KN.same_bits(sblas.gmres_solve_ref(R, g), GN.solve_py(R.tolist(), g))
    R[5, 5] = 0.0                                                            # a zero pivot: inf / nan as written, no trap
    assert KN.same_bits(sblas.gmres_solve_ref(R, g), GN.solve_py(R.tolist(), g))
    with pytest.raises(sblas.SblasError):
        sblas.gmres_solve_ref(np.zeros((65, 65)), np.zeros(65))
    with pytest.raises(sblas.SblasError):
        sblas.gmres_solve_ref(np.zeros((3, 4)), np.zeros(4))
    with pytest.raises(sblas.SblasError):
        sblas.gmres_solve_ref(np.eye(3), np.zeros(2))


def test_limits_agree_with_the_header(sblas):
    text = open(os.path.join(ROOT, "s-blas_amd", "csrc", "gmres.h")).read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    slots = int(re.search(r"GMRES_BLOCK_SLOTS = (\d+)", text).group(1))
    lim = sblas.gmres_limits()
    assert (lim["max_restart"], lim["default_restart"], lim["max_dots"]) == (const("GMRES_MAX_RESTART"), const("GMRES_DEFAULT_RESTART"),
                                                                             const("GMRES_MAX_DOTS")) == (64, 30, 65)
    assert lim["max_dots"] == lim["max_restart"] + 1
    assert (lim["vectors_per_restart"], lim["vectors_fixed"]) == (1, 1 + const("GMRES_EXTRA_VECTORS"))
    assert lim["scalar_bytes"] == 8 * slots and lim["dot_group"] == const("GMRES_DOT_GROUP")
    m = lim["max_restart"]
    assert lim["matrix_bytes"] >= 8 * (m * m + 2 * m + (m + 1) + m + (m + 1))   # R, c, s, g, y, h
    assert "constexpr int KRYLOV_CELL" not in text and "constexpr int KRYLOV_LANES" not in text   # krylov.h's, not redefined
    hdr = open(os.path.join(ROOT, "include", "sblas_hip.h")).read()
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, hdr).group(1))
    assert define("SBLAS_GMRES_MAX_RESTART") == m
    assert (define("SBLAS_GMRES_DENOM_GIVENS"), define("SBLAS_GMRES_DENOM_BETA")) == (const("GMRES_DENOM_GIVENS"), const("GMRES_DENOM_BETA")) == (6, 7)
    assert define("SBLAS_KRYLOV_DENOM_OMEGA") == 5                           # numbered after the existing five
    assert sblas.GMRES_DENOM[6] == "givens" and sblas.GMRES_DENOM[7] == "beta" and sblas.GMRES_DENOM[5] == sblas.KRYLOV_DENOM[5]


def test_launches_of_a_step_a_close_and_a_restart(sblas):
    """counted by hand from the sequences DESIGN.md 3.23 lists, with the solves' launches as SptrsvPlan.info() gives them"""
    for m in (1, 5, 30):
        for lower, upper in ((1, 1), (3, 7), (0, 0)):
            apply = ["solve"] * (lower + upper)                              # one M^-1: the lower solve, then the upper
            tail = ["multi-dot", "fold h", "project", "multi-dot", "fold h + c", "project with (w, w)", "fold and scalar step", "normalise"]
            start = ["dot (b, b)", "fold |b|", "spmv", "residual", "fold and test", "normalise"]
            restart = ["spmv", "residual", "fold and test", "normalise"]
            for precond in (None, "jacobi", "ilu0"):
                mine = apply if precond == "ilu0" else []
                step = mine + ["spmv"] + tail
                close = ["back substitution", "combine"] + mine + ["x update"]
                got = sblas.gmres_launches(m, precond, lower, upper)
                assert got == dict(step=len(step), close=len(close), restart=len(restart), start=len(start),
                                   cycle=m * len(step) + len(close) + len(restart)), (m, precond, lower, upper, got)
    L = sblas.lib()
    import ctypes as C
    out, info = (C.c_int64 * 4)(), (C.c_int64 * 12)()
    assert L.sblas_gmres_launches(0, 0, None, None, out) == -1
    assert L.sblas_gmres_launches(65, 0, None, None, out) == -1
    assert L.sblas_gmres_launches(30, 3, None, None, out) == -1
    assert L.sblas_gmres_launches(30, 2, None, None, out) == -1              # ILU(0) without the solves' info
    assert L.sblas_gmres_launches(30, 2, info, None, out) == -1
    assert L.sblas_gmres_launches(30, 0, None, None, None) == -1
    info[5] = -1
    assert L.sblas_gmres_launches(30, 2, info, info, out) == -1
    for bad in (dict(restart=0), dict(restart=65), dict(precond="ssor")):
        with pytest.raises(sblas.SblasError):
            sblas.gmres_launches(**bad)


def test_exports_are_present(sblas):
    L = sblas.lib()
    for name in ("sblas_gmres_limits", "sblas_gmres_step_ref", "sblas_gmres_solve_ref", "sblas_gmres_launches",
                 "sblas_hip_gmres_dots_workspace", "sblas_hip_gmres_dots_f64", "sblas_hip_gmres_project_f64", "sblas_hip_gmres_combine_f64",
                 "sblas_hip_gmres_plan_create", "sblas_hip_gmres_plan_info", "sblas_hip_gmres_plan_destroy", "sblas_hip_gmres_start",
                 "sblas_hip_gmres_iterate", "sblas_hip_gmres_status"):
        assert name in sblas.EXPORTS and hasattr(L, name), name
    assert L.sblas_hip_gmres_dots_workspace(5000, 65) == 65 * 3 * 8 and L.sblas_hip_gmres_dots_workspace(0, 1) == 8
    assert L.sblas_hip_gmres_dots_workspace(10, 0) == 0 and L.sblas_hip_gmres_dots_workspace(10, 66) == 0


def test_python_refusals_need_no_gpu(sblas):
    import torch
    E = sblas.SblasError
    x = torch.zeros(8, dtype=torch.float64)
    rp = torch.zeros(9, dtype=torch.int32)
    ci = torch.zeros(0, dtype=torch.int32)
    with pytest.raises(E, match="GPU tensor"):
        sblas.GmresPlan(8, rp, ci)
    with pytest.raises(E, match="GPU tensor"):
        sblas.gmres_dots(x.view(1, 8), x)
    with pytest.raises(E, match="GPU tensor"):
        sblas.gmres_project(x.view(1, 8), x[:1], x)
    with pytest.raises(E, match="GPU tensor"):
        sblas.gmres_combine(x.view(1, 8), x[:1])
    with pytest.raises(E, match="GPU tensor"):
        sblas.gmres((8, rp, ci, x[:0]), x)
    for restart in (0, 65, -1, 2.5, None):
        with pytest.raises(E, match="restart"):
            sblas.GmresPlan(8, rp, ci, restart=restart)
    # x is b is refused before any tensor is looked at, so a plan object without a handle shows it
    plan = object.__new__(sblas.GmresPlan)
    plan.handle = None
    with pytest.raises(E, match="x must not be b"):
        sblas.GmresPlan.start(plan, x, x, x)
    for precond in ("ssor", "ilu0", 3, (None, None)):                        # "ilu0" is the one-shot's word: a plan takes the Ilu0Plan
        with pytest.raises(E, match="precond"):
            sblas.GmresPlan(8, rp, ci, precond=precond)
    with pytest.raises(E, match="precond"):
        sblas.gmres((8, rp, ci, x[:0]), x, precond="ssor")
    with pytest.raises(E, match="spmv_plan"):
        sblas.GmresPlan(8, rp, ci, spmv_plan="plan")
    # the split is deliberate: GMRES is a plan of its own, and KrylovPlan goes on refusing it as a method
    with pytest.raises(E, match="method"):
        sblas.KrylovPlan(8, rp, ci, method="gmres")
    with pytest.raises(E):
        sblas.krylov_launches("gmres")
    assert set(sblas.krylov_limits()) == {"cell", "width", "pcg_vectors", "bicgstab_vectors", "max_dots"}


KINDS = (None, "jacobi", "ilu0", "amg", "chebyshev")                         # by code: SBLAS_PRECOND_*


def test_the_two_launch_rules_agree_on_one_application(sblas):
    """one M^-1 costs the same launches under PCG, BiCGStab and GMRES: the kind rule is written once (precond_rule.h)"""
    for precond in KINDS:
        for lower in (0, 1, 7):
            for upper in (0, 1, 7):
                pcg = sblas.krylov_launches("pcg", precond, lower, upper)
                bicg = sblas.krylov_launches("bicgstab", precond, lower, upper)
                g = sblas.gmres_launches(5, precond, lower, upper)
                apply = g["close"] - 3
                if precond in ("ilu0", "amg", "chebyshev"):                  # applied by launches of their own
                    assert apply == (lower + upper if precond == "ilu0" else lower), (precond, lower, upper)
                    assert g["step"] - 9 == pcg - 8, (precond, lower, upper)
                else:
                    assert apply == 0 and pcg == 6, (precond, lower, upper)
                assert g["step"] - 9 == apply, (precond, lower, upper)
                assert bicg - 10 == 2 * apply, (precond, lower, upper)


def test_the_raw_launch_rules_refuse_the_same_arguments(sblas):
    import ctypes as C
    L = sblas.lib()

    def info(v):
        if v is None:
            return None
        a = (C.c_int64 * 12)()
        a[5] = v
        return a

    refused = 0
    for precond in range(-1, 6):
        for lower in (None, -1, 3):
            for upper in (None, -1, 3):
                out = (C.c_int64 * 4)()
                k = [L.sblas_krylov_launches(method, precond, info(lower), info(upper)) for method in (0, 1)]
                g = L.sblas_gmres_launches(30, precond, info(lower), info(upper), out)
                assert (k[0] == -1) == (k[1] == -1) == (g == -1), (precond, lower, upper, k, g)
                # what is refused, said once more: an unknown kind; ILU(0) without both infos; a cycle or a polynomial
                # without the lower one
                want = precond not in range(5) or (precond == 2 and (lower != 3 or upper != 3)) or (precond in (3, 4) and lower != 3)
                assert (g == -1) == want, (precond, lower, upper, g)
                refused += g == -1
    assert refused == 2 * 9 + 8 + 2 * 6
