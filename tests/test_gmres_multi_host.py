"""Multi-right-hand-side GMRES's host side (gmres_multi_rule.cpp, precond_rule.h; no GPU): the new header against its
export list, the limits, the grid, the launches against the single solver's, the kinds the plan takes through each door,
and the lockstep loop of tests/gmres_multi_compose.py with column-separable host parts against independent
solver_compose.composed_gmres loops."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gmres_multi_compose as GMC
import gmres_numerics as GN
import ilu0_numerics as IN
import krylov_numerics as KN
import multi_compose as MC
import solver_compose as SC
from conftest import ROOT

RTOL = 1e-10


def test_the_library_exports_what_the_new_header_declares(sblas):
    hdr = open(os.path.join(ROOT, "include", "sblas_hip_gmres_multi.h")).read()
    declared = set(re.findall(r"\b(sblas_[A-Za-z0-9_]+)\s*\(", hdr))
    others = set(sblas.EXPORTS + sblas.EXPORTS_AMG_SA + sblas.EXPORTS_AMG_DEV + sblas.EXPORTS_CHEBY + sblas.EXPORTS_KRYLOV_MULTI +
                 sblas.EXPORTS_AMG_MULTI + sblas.EXPORTS_SPTRSM_TILE)
    assert declared == set(sblas.EXPORTS_GMRES_MULTI) and not declared & others, declared ^ set(sblas.EXPORTS_GMRES_MULTI)
    assert len(set(sblas.EXPORTS_GMRES_MULTI)) == len(sblas.EXPORTS_GMRES_MULTI)
    assert '#include "sblas_hip_gmres_multi.h"' in open(os.path.join(ROOT, "include", "sblas_hip.h")).read()
    for name in declared:
        assert hasattr(sblas.lib(), name), name


def test_limits_agree_with_the_header_and_the_two_plans_it_combines(sblas):
    public = open(os.path.join(ROOT, "include", "sblas_hip_gmres_multi.h")).read()
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, public).group(1))
    lim, single, multi = sblas.gmres_multi_limits(), sblas.gmres_limits(), sblas.krylov_multi_limits()
    assert lim["max_rhs"] == define("SBLAS_GMRES_MULTI_MAX_RHS") == multi["max_rhs"] == 64
    assert lim["tile"] == define("SBLAS_GMRES_MULTI_TILE") == multi["tile"] == 8
    assert lim["max_restart"] == define("SBLAS_GMRES_MULTI_MAX_RESTART") == single["max_restart"] == 64
    assert lim["cell"] == multi["cell"] == 2048 and lim["width"] == multi["width"] == 256
    assert lim["fixed_blocks"] == single["vectors_fixed"] - 1 == 3            # W, U, Z beside the m + 1 of the basis
    assert lim["block_slots"] * 8 == single["scalar_bytes"] == 128 and lim["matrix_doubles"] * 8 == single["matrix_bytes"]
    out = (C.c_int64 * 8)(*([-7] * 8))
    assert sblas.lib().sblas_gmres_multi_limits(out) == 0 and list(out)[:7] == [64, 8, 2048, 256, 64, 3, 16]
    assert sblas.lib().sblas_gmres_multi_limits(None) != 0


def test_the_grid_of_a_pass(sblas):
    """counted by hand: a workgroup is a cell of 2048 rows and a tile of 8 columns"""
    for n in (0, 1, 2048, 2049):
        for s in (1, 7, 8, 9, 64):
            cells = {0: 0, 1: 1, 2048: 1, 2049: 2}[n]
            tiles = {1: 1, 7: 1, 8: 1, 9: 2, 64: 8}[s]
            last = {1: 1, 7: 7, 8: 8, 9: 1, 64: 8}[s]
            assert sblas.gmres_multi_grid(n, s) == dict(cells=cells, tiles=tiles, grid=cells * tiles, last_tile=last), (n, s)
            assert sblas.gmres_multi_grid(n, s) == sblas.krylov_multi_grid(n, s)
    for n, s in ((-1, 1), (1, 0), (1, -1), (1, 65), (2048, 2 ** 31)):
        with pytest.raises(sblas.SblasError):
            sblas.gmres_multi_grid(n, s)


DOORS = ((0, 0, 0), (1, 0, 0), (3, 17, 0), (2, 11, 7))                        # (kind, lower or cycle launches, upper launches)


def test_launches_are_the_single_solvers_with_the_product_in_the_spmvs_place(sblas):
    L = sblas.lib()
    names = {0: None, 1: "jacobi", 2: "ilu0", 3: "amg"}
    for restart in (1, 30, 64):
        for kind, lo, up in DOORS:
            want = sblas.gmres_launches(restart, names[kind], lo, up)
            for spmm in (0, 1, 3):
                out = (C.c_int64 * 4)(-7, -7, -7, -7)
                cycle = L.sblas_gmres_multi_launches(restart, kind, spmm, lo, up, out)
                got = dict(step=out[0], close=out[1], restart=out[2], start=out[3], cycle=cycle)
                assert got == dict(step=want["step"] - 1 + spmm, close=want["close"], restart=want["restart"] - 1 + spmm,
                                   start=want["start"] - 1 + spmm, cycle=want["cycle"] + (restart + 1) * (spmm - 1)), (restart, kind, spmm)
    out = (C.c_int64 * 4)(-7, -7, -7, -7)
    for kind in (sblas.PRECOND_CHEBYSHEV, -1, 5, 9):                         # the refused kinds
        for lo, up in ((0, 0), (3, 0), (3, 3)):
            assert L.sblas_gmres_multi_launches(30, kind, 1, lo, up, out) == -1
    for bad in ((0, 0, 1, 0, 0), (65, 0, 1, 0, 0), (30, 0, -1, 0, 0), (30, 0, 1, 1, 0), (30, 1, 1, 0, 1), (30, 3, 1, 5, 1), (30, 3, 1, -1, 0),
                (30, 2, 1, 1, -1)):
        assert L.sblas_gmres_multi_launches(*bad, out) == -1, bad
    assert list(out) == [-7, -7, -7, -7]                                      # a refusal writes nothing
    assert L.sblas_gmres_multi_launches(30, 0, 1, 0, 0, None) == -1
    # the Python door: the names without a multi-column apply keep _multi_precond's answers
    assert sblas.gmres_multi_launches(30, None, 2) == dict(step=10, close=3, restart=5, start=7, cycle=308)
    assert sblas.gmres_multi_launches(5, "jacobi", 1)["cycle"] == 5 * 9 + 3 + 4
    for name in ("ilu0", "amg", "chebyshev"):
        with pytest.raises(sblas.SblasError, match="the %s preconditioner has no multi-column apply" % name):
            sblas.gmres_multi_launches(30, name)


def test_the_kinds_the_plan_takes_through_each_door(sblas):
    L = sblas.lib()
    kinds = (0, 1, 2, 3, 4, -1, 5, 9)
    alone = {kind: L.sblas_gmres_multi_precond_ok(kind) == 0 for kind in kinds}
    assert alone == {kind: kind in (sblas.PRECOND_NONE, sblas.PRECOND_JACOBI) for kind in kinds}
    with_plan = {kind: L.sblas_gmres_multi_precond_plan_ok(kind) == 0 for kind in kinds}
    assert with_plan == {kind: kind == sblas.PRECOND_AMG for kind in kinds}
    with_pair = {kind: L.sblas_gmres_multi_precond_pair_ok(kind) == 0 for kind in kinds}
    assert with_pair == {kind: kind == sblas.PRECOND_ILU0 for kind in kinds}
    for kind in kinds:                                                       # one rule under both multi-right-hand-side plans
        assert L.sblas_gmres_multi_precond_ok(kind) == L.sblas_krylov_multi_precond_ok(kind)
        assert L.sblas_gmres_multi_precond_plan_ok(kind) == L.sblas_krylov_multi_precond_plan_ok(kind)
        assert L.sblas_gmres_multi_precond_pair_ok(kind) == L.sblas_krylov_multi_precond_pair_ok(kind)
    rule = open(os.path.join(ROOT, "s-blas_amd", "csrc", "gmres_multi_rule.cpp")).read()
    assert "precond_multi(" in rule and "precond_multi_applied(" in rule and "precond_multi_pair(" in rule


# ---------------------------------------------------------------------------------------------------------------------
# the lockstep loop against independent loops: with host parts the composition is separable by column
# ---------------------------------------------------------------------------------------------------------------------
def host_ilu_apply(n, rp, ci, lu):
    """v -> U^-1 (L^-1 v) by numpy substitutions with ilu0_numerics.ilu0_ref's factor, one column at a time"""
    rp = np.asarray(rp, np.int64)
    rows = [(ci[rp[i]:rp[i + 1]], lu[rp[i]:rp[i + 1]]) for i in range(n)]
    low = [(c[c < i], v[c < i]) for i, (c, v) in enumerate(rows)]
    upp = [(c[c > i], v[c > i], v[c == i][0]) for i, (c, v) in enumerate(rows)]

    def apply(r):
        with np.errstate(all="ignore"):
            y = np.zeros(n)
            for i, (c, v) in enumerate(low):
                y[i] = r[i] - np.dot(v, y[c])
            z = np.zeros(n)
            for i in range(n - 1, -1, -1):
                c, v, d = upp[i]
                z[i] = (y[i] - np.dot(v, z[c])) / d
        return z
    return apply


def same_result(got, want):
    ok = KN.same_bits(got["x"], want["x"]) and KN.same_bits(got["rnorm"], want["rnorm"]) and KN.same_bits(got["bnorm"], want["bnorm"])
    return ok and all(got[k] == want[k] for k in ("status", "iterations", "restarts", "columns", "breakdown"))


@pytest.fixture(scope="module")
def case():
    A = n, rp, ci, val = KN.convection_diffusion(24)
    mv1 = lambda v: KN.matvec(*A, v)
    mvs = lambda V: np.stack([mv1(V[:, j]) for j in range(V.shape[1])], axis=1)
    dinv = 1.0 / val[SC.stored_diagonal(rp, ci)]
    applies = dict(none=lambda v: v, jacobi=lambda v: dinv * v, ilu0=host_ilu_apply(n, rp, ci, IN.ilu0_ref(n, rp, ci, val)))
    B, X0, names = MC.columns(n, mv1)
    return dict(mv1=mv1, mvs=mvs, applies=applies, B=B, X0=X0, names=names)


@pytest.mark.parametrize("precond", ["none", "jacobi", "ilu0"])
@pytest.mark.parametrize("restart,max_iter", [(1, 60), (5, 1000), (30, 1000), (5, 7)])
def test_the_lockstep_loop_equals_independent_loops(case, restart, max_iter, precond):
    g = case
    apply = g["applies"][precond]
    got = GMC.composed_gmres_multi(g["mvs"], apply, KN.dot_np, g["B"], g["X0"], restart, RTOL, max_iter)
    assert len(got) == 9
    dots = lambda V, w: [KN.dot_np(v, w) for v in V]
    for c, name in enumerate(g["names"]):
        want = SC.composed_gmres(g["mv1"], apply, KN.dot_np, dots, g["B"][:, c], g["X0"][:, c], restart, RTOL, max_iter)
        assert same_result(got[c], want), (name, got[c], want)
    by = dict(zip(g["names"], got))
    print("GMRES(%d) %s, max_iter %d: %s" % (restart, precond, max_iter, {k: (v["status"], v["iterations"], v["restarts"]) for k, v in by.items()}))
    assert (by["zero"]["status"], by["zero"]["iterations"]) == (GN.CONVERGED, 0) and not by["zero"]["x"].any()
    assert (by["nan"]["status"], by["nan"]["breakdown"], by["nan"]["iterations"]) == (GN.BREAKDOWN, "beta", 0)
    if max_iter == 7:                                                        # every column that runs stops at exactly 7
        limited = [v for v in got if v["status"] == GN.LIMIT]
        assert len(limited) >= 5 and all(v["iterations"] == 7 and v["restarts"] == 1 and v["columns"] == 2 for v in limited), by
        assert all(v["iterations"] < 7 for v in got if v["status"] != GN.LIMIT)
    else:
        assert all(v["status"] in (GN.CONVERGED, GN.LIMIT) for k, v in by.items() if k != "nan")
    if restart == 30:                                                        # the cycle is long enough for every column to get there
        assert all(v["status"] == GN.CONVERGED for k, v in by.items() if k != "nan")
        assert MC.spread_ok([v["iterations"] for v in got])


def test_an_empty_block_and_the_empty_system():
    got = GMC.composed_gmres_multi(None, None, None, np.zeros((0, 3)), np.zeros((0, 3)), 5, RTOL, 10)
    assert [(v["status"], v["iterations"], v["rnorm"], v["columns"]) for v in got] == [(GN.CONVERGED, 0, 0.0, 0)] * 3


def test_python_refusals_need_no_gpu(sblas):
    import torch
    E = sblas.SblasError
    rp = torch.zeros(9, dtype=torch.int32)
    ci = torch.zeros(0, dtype=torch.int32)
    for s in (0, 65):
        with pytest.raises(E, match="right-hand sides"):
            sblas.GmresMultiPlan(8, rp, ci, s)
    for restart in (0, 65, 2.5, True):
        with pytest.raises(E, match="restart must be an integer"):
            sblas.GmresMultiPlan(8, rp, ci, 3, restart=restart)
    for name in ("ilu0", "amg", "chebyshev"):                                # _multi_precond's answers, reused
        with pytest.raises(E, match="the %s preconditioner has no multi-column apply" % name):
            sblas.GmresMultiPlan(8, rp, ci, 3, precond=name)
    with pytest.raises(E, match="precond must be None or 'jacobi'"):
        sblas.GmresMultiPlan(8, rp, ci, 3, precond="ssor")
    for pair in ((None, None), ("lower", "upper"), (1, 2, 3)):
        with pytest.raises(E):
            sblas.GmresMultiPlan(8, rp, ci, 3, precond=pair)
    with pytest.raises(E):                                                   # gmres keeps refusing a block
        sblas.gmres((8, rp, ci, torch.zeros(0, dtype=torch.float64)), torch.zeros(8, 3, dtype=torch.float64))
    with pytest.raises(E, match="GPU tensor"):
        sblas.gmres_multi_dots(torch.zeros(2, 8, 3, dtype=torch.float64), torch.zeros(8, 3, dtype=torch.float64))


def test_the_rule_check_runs_clean_under_the_sanitizers(tmp_path):
    """tools/gmres_multi_rule_check.cpp, host code only and a program of its own, under the address and
    undefined-behaviour sanitizers"""
    cxx = next((p for p in (shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++", shutil.which("g++")) if p and os.path.exists(p)), None)
    if cxx is None:
        pytest.skip("no host compiler")
    csrc = os.path.join(ROOT, "s-blas_amd", "csrc")
    exe = str(tmp_path / "gmres_multi_rule_check")
    src = [os.path.join(ROOT, "tools", "gmres_multi_rule_check.cpp")] + \
          [os.path.join(csrc, f) for f in ("gmres_multi_rule.cpp", "gmres_rule.cpp", "krylov_multi_rule.cpp")]
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                          + src + ["-o", exe])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert done.returncode == 0, done.stdout.decode()
    assert b"gmres_multi_rule_check: ok" in done.stdout
