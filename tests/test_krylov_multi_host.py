"""The multi-right-hand-side Krylov solvers' host side (krylov_multi_rule.cpp, krylov_scalar.h; no GPU): the new header
against its export list, the limits and the launch rule, the shared scalar step compiled for the host against the Python
floats of tests/solver_compose.py, and the lockstep loops of tests/multi_compose.py against s independent single loops."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import krylov_numerics as KN
import multi_compose as MC
import solver_compose as SC
from conftest import ROOT

RTOL = 1e-10


def test_the_library_exports_what_the_new_header_declares(sblas):
    hdr = open(os.path.join(ROOT, "include", "sblas_hip_krylov_multi.h")).read()
    declared = set(re.findall(r"\b(sblas_[A-Za-z0-9_]+)\s*\(", hdr))
    others = set(sblas.EXPORTS + sblas.EXPORTS_AMG_SA + sblas.EXPORTS_AMG_DEV + sblas.EXPORTS_CHEBY)
    assert declared == set(sblas.EXPORTS_KRYLOV_MULTI) and not declared & others, declared ^ set(sblas.EXPORTS_KRYLOV_MULTI)
    assert len(set(sblas.EXPORTS_KRYLOV_MULTI)) == len(sblas.EXPORTS_KRYLOV_MULTI)
    assert '#include "sblas_hip_krylov_multi.h"' in open(os.path.join(ROOT, "include", "sblas_hip.h")).read()
    for name in declared:
        assert hasattr(sblas.lib(), name), name


def test_limits_agree_with_the_headers(sblas):
    text = open(os.path.join(ROOT, "s-blas_amd", "csrc", "krylov.h")).read()
    const = lambda name: int(re.search(r"%s = (\d+)" % name, text).group(1))
    public = open(os.path.join(ROOT, "include", "sblas_hip_krylov_multi.h")).read()
    macro = lambda name: int(re.search(r"#define %s (\d+)" % name, public).group(1))
    lim = sblas.krylov_multi_limits()
    assert lim == dict(max_rhs=macro("SBLAS_KRYLOV_MULTI_MAX_RHS"), tile=macro("SBLAS_KRYLOV_MULTI_TILE"), cell=const("KRYLOV_CELL"),
                       width=const("KRYLOV_LANES"), pcg_blocks=const("KRYLOV_PCG_VECTORS"), bicgstab_blocks=const("KRYLOV_BICGSTAB_VECTORS"),
                       max_dots=const("KRYLOV_MAX_DOTS"), block_slots=const("KRYLOV_BLOCK_SLOTS"))
    assert (lim["max_rhs"], lim["tile"], lim["cell"], lim["width"]) == (64, 8, KN.CELL, KN.WIDTH)
    single = sblas.krylov_limits()
    assert (lim["cell"], lim["width"], lim["max_dots"]) == (single["cell"], single["width"], single["max_dots"])
    assert sblas.lib().sblas_krylov_multi_limits(None) != 0
    for name, code in sblas.KRYLOV_STEPS.items():
        assert macro("SBLAS_KRYLOV_STEP_" + name.upper()) == code


def test_launches_grid_and_the_kinds_a_batch_takes(sblas):
    """counted by hand from the sequence DESIGN.md 3.29 lists"""
    L = sblas.lib()
    for spmm in (0, 1, 3, 17):
        pcg = ["spmm"] * spmm + ["dots", "fold alpha", "x r update", "fold residual and beta", "p update"]
        bicg = ["p update"] + ["spmm"] * spmm + ["dots", "fold alpha", "s update"] + ["spmm"] * spmm + \
               ["dots", "fold omega", "x r update", "fold residual and beta"]
        for precond in (None, "jacobi"):
            assert sblas.krylov_multi_launches("pcg", precond, spmm) == len(pcg)
            assert sblas.krylov_multi_launches("bicgstab", precond, spmm) == len(bicg)
    assert L.sblas_krylov_multi_launches(2, 0, 1) == -1 and L.sblas_krylov_multi_launches(0, 0, -1) == -1
    # the kinds: decided by precond_rule.h, where every kind is listed
    rule = open(os.path.join(ROOT, "s-blas_amd", "csrc", "precond_rule.h")).read()
    assert "precond_multi" in rule
    takes = {kind: L.sblas_krylov_multi_precond_ok(kind) == 0 for kind in range(-1, 7)}
    assert takes == {-1: False, sblas.PRECOND_NONE: True, sblas.PRECOND_JACOBI: True, sblas.PRECOND_ILU0: False, sblas.PRECOND_AMG: False,
                     sblas.PRECOND_CHEBYSHEV: False, 5: False, 6: False}
    for kind in (sblas.PRECOND_ILU0, sblas.PRECOND_AMG, sblas.PRECOND_CHEBYSHEV, 9):
        assert L.sblas_krylov_multi_launches(0, kind, 1) == -1
    for name in ("ilu0", "amg", "chebyshev"):
        with pytest.raises(sblas.SblasError, match="no multi-column apply"):
            sblas.krylov_multi_launches("pcg", name)
    with pytest.raises(sblas.SblasError, match="method"):
        sblas.krylov_multi_launches("gmres")
    # the grid: cells x ceil(s / 8), the last tile ragged
    for n in (0, 1, KN.CELL, KN.CELL + 1, 5 * KN.CELL):
        for s in (1, 7, 8, 9, 11, 16, 63, 64):
            g = sblas.krylov_multi_grid(n, s)
            assert g == dict(cells=-(-n // KN.CELL), tiles=-(-s // 8), grid=-(-n // KN.CELL) * -(-s // 8), last_tile=(s - 1) % 8 + 1)
    for n, s in ((-1, 1), (1, 0), (1, 65)):
        with pytest.raises(sblas.SblasError):
            sblas.krylov_multi_grid(n, s)
    assert L.sblas_hip_krylov_multi_dot_workspace(KN.CELL + 1, 11, 3) == 3 * 11 * 2 * 8
    assert L.sblas_hip_krylov_multi_dot_workspace(0, 1, 1) == 8 and L.sblas_hip_krylov_multi_dot_workspace(5, 65, 1) == 0
    assert L.sblas_hip_krylov_multi_dot_workspace(5, 1, 4) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the shared scalar step, compiled for the host, against the Python floats of the composed loops
# ---------------------------------------------------------------------------------------------------------------------
STATUS, ITER, RNORM, BNORM, ALPHA, BETA, OMEGA, WHICH, RHO, TOL, MAX_ITER, ZERO_X = range(12)      # krylov.h's KrylovSlot


def ints(block):
    return block.view(np.int64)


def test_the_scalar_step_is_the_composed_loops_step(sblas):
    step = sblas.krylov_scalar_step_ref
    blk = np.full(16, -7.0)
    step("start_b", [9.0], blk, flag=1, rtol=0.5, atol=1.0, max_iter=3)
    assert (blk[BNORM], blk[TOL], blk[OMEGA], blk[ALPHA], blk[BETA], blk[RHO], blk[RNORM]) == (3.0, 1.5, 1.0, 0.0, 0.0, 0.0, 0.0)
    assert list(ints(blk)[[STATUS, ITER, WHICH, MAX_ITER, ZERO_X]]) == [0, 0, 0, 3, 0]
    step("start_b", [9.0], blk, flag=0, rtol=0.1, atol=1.0, max_iter=3)
    assert (blk[TOL], blk[OMEGA]) == (SC.tolerance(0.1, 1.0, 3.0), 0.0) and blk[TOL] == 1.0
    step("start_r", [16.0, 5.0], blk)
    assert (blk[RNORM], blk[RHO]) == (4.0, 5.0) and ints(blk)[STATUS] == sblas.KRYLOV_RUNNING and ints(blk)[ITER] == 0
    step("pcg_alpha", [2.5], blk)
    assert blk[ALPHA] == 5.0 / 2.5
    step("pcg_res", [4.0, 0.3], blk, flag=1)
    assert (blk[RNORM], blk[BETA], blk[RHO]) == (2.0, 0.3 / 5.0, 0.3) and ints(blk)[ITER] == 1
    for bad in (0.0, math.inf, math.nan):
        b2 = blk.copy()
        step("pcg_alpha", [bad], b2)
        assert (ints(b2)[STATUS], ints(b2)[WHICH]) == (sblas.KRYLOV_BREAKDOWN, 1) and b2[ALPHA] == blk[ALPHA]
        frozen = b2.copy()
        step("pcg_res", [1e-30, 1.0], b2, flag=1)                            # frozen: nothing changes
        assert KN.same_bits(b2, frozen)
    b2 = blk.copy()
    step("pcg_res", [0.25, 1.0], b2, flag=1)                                 # |r| = 0.5 <= tol = 1: converged, beta untouched
    assert (ints(b2)[STATUS], ints(b2)[ITER], b2[RNORM], b2[BETA]) == (sblas.KRYLOV_CONVERGED, 2, 0.5, blk[BETA])
    b2 = blk.copy()
    step("pcg_res", [4.0, 1.0], b2, flag=1), step("pcg_res", [4.0, 1.0], b2, flag=1)
    assert (ints(b2)[STATUS], ints(b2)[ITER]) == (sblas.KRYLOV_LIMIT, 3)
    # BiCGStab: the half step, and beta's two denominators in order
    blk = np.zeros(16)
    step("start_b", [4.0], blk, flag=1, rtol=0.25, max_iter=9)
    step("start_r", [3.0], blk)
    assert blk[RHO] == 3.0 and blk[TOL] == 0.5
    step("bicg_alpha", [1.5], blk)
    step("bicg_omega", [0.0, 0.0, 0.2], blk)
    assert blk[OMEGA] == 0.0 and ints(blk)[STATUS] == 0                      # sqrt(0.2) <= 0.5: omega = 0 takes the half step
    b2 = blk.copy()
    step("bicg_omega", [0.0, 0.0, 0.3], b2)
    assert (ints(b2)[STATUS], ints(b2)[WHICH]) == (sblas.KRYLOV_BREAKDOWN, 4)
    step("bicg_omega", [0.6, 0.8, 1.0], blk)
    assert blk[OMEGA] == 0.6 / 0.8
    step("bicg_res", [2.0, 0.7], blk)
    assert blk[BETA] == (0.7 / 3.0) * (2.0 / (0.6 / 0.8)) and blk[RHO] == 0.7 and ints(blk)[ITER] == 1
    blk[OMEGA] = 0.0
    step("bicg_res", [2.0, 0.7], blk)
    assert (ints(blk)[STATUS], ints(blk)[WHICH]) == (sblas.KRYLOV_BREAKDOWN, 5)
    # b == 0
    blk = np.full(16, -7.0)
    step("start_b", [0.0], blk, rtol=0.5)
    assert list(ints(blk)[[STATUS, ZERO_X]]) == [sblas.KRYLOV_CONVERGED, 1]
    L = sblas.lib()
    d = np.zeros(3)
    assert L.sblas_krylov_scalar_step_ref(0, 1, 0, d.ctypes.data, blk.ctypes.data, 0.0, 0.0, 0) != 0
    assert L.sblas_krylov_scalar_step_ref(10, 1, 0, d.ctypes.data, blk.ctypes.data, 0.0, 0.0, 0) != 0
    assert L.sblas_krylov_scalar_step_ref(8, 2, 0, d.ctypes.data, blk.ctypes.data, 0.0, 0.0, 0) != 0
    assert L.sblas_krylov_scalar_step_ref(4, 4, 0, d.ctypes.data, blk.ctypes.data, 0.0, 0.0, 0) != 0
    with pytest.raises(sblas.SblasError):
        step("axpy", [1.0], blk)


def test_one_text_of_the_scalar_step():
    """krylov.hip and krylov_multi.hip run krylov_scalar.h's step; neither keeps a switch of its own"""
    src = lambda name: open(os.path.join(ROOT, "s-blas_amd", "csrc", name)).read()
    for name in ("krylov.hip", "krylov_multi.hip", "krylov_multi_rule.cpp"):
        text = src(name)
        assert '#include "krylov_scalar.h"' in text and "krylov_scalar_step(" in text, name
        assert "switch (op)" not in text.split("// ---- launches")[0] and "KS_BETA] =" not in text, name
    assert src("krylov_scalar.h").count("switch (op)") == 1
    assert "contract(off)" in src("krylov_multi.hip").split("__global__")[0]      # at file scope, ahead of every kernel


def test_one_text_of_the_plan_plumbing(sblas):
    """krylov_multi.hip and gmres_multi.hip keep their plans on multi_plan.h's base, and the two Python classes on
    _MultiSolverPlan: neither side holds a copy of what the base holds"""
    src = lambda name: open(os.path.join(ROOT, "s-blas_amd", "csrc", name)).read()
    base = src("multi_plan.h")
    for name in ("krylov_multi.hip", "gmres_multi.hip"):
        text = src(name)
        assert '#include "multi_plan.h"' in text, name
        assert "span_bytes" not in text and not re.search(r"^\w[\w \*]*\bproduct\(", text, re.M), name
        for call in ("sblas_hip_spmm_plan_create", "sblas_hip_amg_plan_reserve_multi", "hipMemcpyDeviceToHost"):
            assert call not in text and call in base, (name, call)
    assert "span_bytes" in src("krylov_multi.h") and re.search(r"^inline int product\(", base, re.M)
    for name in ("start", "solve", "iterate", "destroy", "status"):
        assert getattr(sblas.KrylovMultiPlan, name) is getattr(sblas.GmresMultiPlan, name), name


def overlap_cases():
    """the rows of tools/krylov_multi_rule_check.cpp's table: (n, s, x0, ldx, b0, ldb, overlap)"""
    text = open(os.path.join(ROOT, "tools", "krylov_multi_rule_check.cpp")).read()
    table = text.split("OVERLAP_CASES[] = {")[1].split("};")[0]
    rows = re.findall(r"\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (true|false)\}", table)
    return [tuple(int(v) for v in r[:6]) + (r[6] == "true",) for r in rows]


def test_the_overlap_table_is_pythons_answer_too(sblas):
    """the literals the rule check holds the C predicate to are what _blocks_overlap answers, either way round"""
    class At:
        def __init__(self, ptr):
            self.ptr = ptr

        def data_ptr(self):
            return self.ptr

    cases = overlap_cases()
    assert len(cases) >= 8 and {c[6] for c in cases} == {True, False} and {c[0] for c in cases} >= {0, 1, 5}
    for n, s, x0, ldx, b0, ldb, want in cases:
        assert bool(sblas._blocks_overlap(At(x0), ldx, At(b0), ldb, n, s)) == want, (n, s, x0, ldx, b0, ldb)
        assert bool(sblas._blocks_overlap(At(b0), ldb, At(x0), ldx, n, s)) == want, (n, s, x0, ldx, b0, ldb)


def test_the_rule_check_runs_clean_under_the_sanitizers(tmp_path):
    """tools/krylov_multi_rule_check.cpp, host code only and a program of its own, under the address and
    undefined-behaviour sanitizers (as test_gmres_multi_host.py runs its rule check)"""
    cxx = next((p for p in (shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++", shutil.which("g++")) if p and os.path.exists(p)), None)
    if cxx is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "krylov_multi_rule_check")
    src = [os.path.join(ROOT, "tools", "krylov_multi_rule_check.cpp"), os.path.join(ROOT, "s-blas_amd", "csrc", "krylov_multi_rule.cpp")]
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                          + src + ["-o", exe])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert done.returncode == 0, done.stdout.decode()
    assert b"krylov_multi_rule_check: ok" in done.stdout


# ---------------------------------------------------------------------------------------------------------------------
# the lockstep loop against s independent loops
# ---------------------------------------------------------------------------------------------------------------------
def host_parts(A):
    n, rp, ci, val = A
    mv1 = lambda v: KN.matvec(n, rp, ci, val, v)
    mvs = lambda V: np.stack([mv1(V[:, j]) for j in range(V.shape[1])], axis=1)
    return mv1, mvs


def same_solved(got, want):
    ok = KN.same_bits(got.x, want.x) and got.iterations == want.iterations and got.status == want.status
    ok = ok and got.breakdown == want.breakdown
    for name in ("rnorm", "bnorm", "alpha", "beta", "omega"):
        ok = ok and KN.same_bits(getattr(got, name), getattr(want, name))
    return ok


@pytest.fixture(scope="module")
def spd():
    return KN.spd_perturbed(48)


@pytest.fixture(scope="module")
def convection():
    return KN.convection_diffusion(48)


@pytest.mark.parametrize("jacobi", [False, True])
def test_lockstep_pcg_equals_independent_solves(spd, jacobi):
    n, rp, ci, val = spd
    mv1, mvs = host_parts(spd)
    B, X0, names = MC.columns(n, mv1)
    dinv = 1.0 / val[SC.stored_diagonal(rp, ci)]
    apply = (lambda v: dinv * v) if jacobi else (lambda v: v)
    got = MC.composed_pcg_multi(mvs, apply, KN.dot_np, B, X0, RTOL, 1000)
    for j, name in enumerate(names):
        want = SC.composed_pcg(mv1, apply, KN.dot_np, B[:, j], X0[:, j], RTOL, 1000)
        assert same_solved(got[j], want), (name, got[j].asdict(), want.asdict())
    by = dict(zip(names, got))
    print("PCG%s on spd_perturbed(48): %s" % (" with Jacobi" if jacobi else "", {k: (v.status, v.iterations) for k, v in by.items()}))
    assert (by["zero"].status, by["zero"].iterations) == ("converged", 0) and not by["zero"].x.any()
    assert (by["nan"].status, by["nan"].iterations, by["nan"].breakdown) == ("breakdown", 0, SC.DENOM_PQ)
    assert all(v.status == "converged" for k, v in by.items() if k != "nan")
    assert by["warm 0.001"].iterations > by["warm 1e-06"].iterations > by["warm 1e-09"].iterations > 0
    assert MC.spread_ok([v.iterations for v in got])


def test_lockstep_bicgstab_equals_independent_solves(convection):
    n, rp, ci, val = convection
    mv1, mvs = host_parts(convection)
    B, X0, names = MC.columns(n, mv1)
    for jacobi in (False, True):
        dinv = 1.0 / val[SC.stored_diagonal(rp, ci)]
        apply = (lambda v: dinv * v) if jacobi else (lambda v: v)
        got = MC.composed_bicgstab_multi(mvs, apply, KN.dot_np, B, X0, RTOL, 1000)
        for j, name in enumerate(names):
            want = SC.composed_bicgstab(mv1, apply, KN.dot_np, B[:, j], X0[:, j], RTOL, 1000)
            assert same_solved(got[j], want), (name, jacobi, got[j].asdict(), want.asdict())
        by = dict(zip(names, got))
        print("BiCGStab on convection_diffusion(48), Jacobi %s: %s" % (jacobi, {k: (v.status, v.iterations) for k, v in by.items()}))
        assert (by["nan"].status, by["nan"].iterations, by["nan"].breakdown) == ("breakdown", 0, SC.DENOM_RV)
        assert (by["zero"].status, by["zero"].iterations) == ("converged", 0)
        assert all(v.status == "converged" for k, v in by.items() if k != "nan")
        assert MC.spread_ok([v.iterations for v in got])


def test_lockstep_limits_and_empty_systems(spd):
    n, rp, ci, val = spd
    mv1, mvs = host_parts(spd)
    B, X0, names = MC.columns(n, mv1)
    ident = lambda v: v
    for loop, single in ((MC.composed_pcg_multi, SC.composed_pcg), (MC.composed_bicgstab_multi, SC.composed_bicgstab)):
        for max_iter in (0, 5):                                              # the limit, per column: a warm start still converges
            got = loop(mvs, ident, KN.dot_np, B, X0, RTOL, max_iter)
            for j, name in enumerate(names):
                assert same_solved(got[j], single(mv1, ident, KN.dot_np, B[:, j], X0[:, j], RTOL, max_iter)), (name, max_iter)
        got = loop(mvs, ident, KN.dot_np, B, X0, RTOL, 5)
        assert {g.status for g in got} == {"converged", "limit", "breakdown"}
        empty = loop(lambda V: V, ident, KN.dot_np, np.zeros((0, 3)), np.zeros((0, 3)), RTOL, 10)
        assert [(e.status, e.iterations) for e in empty] == [("converged", 0)] * 3
    assert not MC.spread_ok([0, 3, 3, 5, 5]) and not MC.spread_ok([0, 4, 5, 6, 7]) and MC.spread_ok([0, 3, 15, 27, 41])


def test_python_refusals_need_no_gpu(sblas):
    import torch
    E = sblas.SblasError
    rp = torch.zeros(9, dtype=torch.int32)
    ci = torch.zeros(0, dtype=torch.int32)
    X = torch.zeros(8, 3, dtype=torch.float64)
    with pytest.raises(E, match="GPU tensor"):
        sblas.KrylovMultiPlan(8, rp, ci, 3)
    with pytest.raises(E, match="method"):
        sblas.KrylovMultiPlan(8, rp, ci, 3, method="gmres")
    for s in (0, 65):
        with pytest.raises(E, match="right-hand sides"):
            sblas.KrylovMultiPlan(8, rp, ci, s)
    for name in ("ilu0", "amg", "chebyshev"):
        with pytest.raises(E, match="no multi-column apply"):
            sblas.KrylovMultiPlan(8, rp, ci, 3, precond=name)
    with pytest.raises(E, match="None or 'jacobi'"):
        sblas.KrylovMultiPlan(8, rp, ci, 3, precond="ssor")
    with pytest.raises(E, match="GPU tensor"):
        sblas.krylov_multi_dots([(X, X)])
    with pytest.raises(E, match="one to three"):
        sblas.krylov_multi_dots([])
    with pytest.raises(E, match="op must be"):
        sblas.krylov_multi_update("axpy", X, [X])
    with pytest.raises(E, match="no multi-column apply"):
        sblas.pcg_multi((8, rp, ci, X), X, precond="ilu0")
