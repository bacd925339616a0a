"""The block AMG cycle's host side and its seat's rule (amg_rule.cpp, krylov_multi_rule.cpp, precond_rule.h; no GPU): the
new header against its export list, the limits and the grid of a multi-column row kernel, which preconditioner kinds a
multi-right-hand-side plan takes WITH a plan, the launches of an iteration with a block cycle in it, and the lockstep loops
of tests/multi_compose.py with a cycle as `apply` against independent single loops."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import amg_numerics as AN
import krylov_numerics as KN
import multi_compose as MC
import solver_compose as SC
from conftest import ROOT

RTOL = 1e-10


def test_the_library_exports_what_the_new_header_declares(sblas):
    hdr = open(os.path.join(ROOT, "include", "sblas_hip_amg_multi.h")).read()
    declared = set(re.findall(r"\b(sblas_[A-Za-z0-9_]+)\s*\(", hdr))
    others = set(sblas.EXPORTS + sblas.EXPORTS_AMG_SA + sblas.EXPORTS_AMG_DEV + sblas.EXPORTS_CHEBY + sblas.EXPORTS_KRYLOV_MULTI)
    assert declared == set(sblas.EXPORTS_AMG_MULTI) and not declared & others, declared ^ set(sblas.EXPORTS_AMG_MULTI)
    assert len(set(sblas.EXPORTS_AMG_MULTI)) == len(sblas.EXPORTS_AMG_MULTI)
    assert '#include "sblas_hip_amg_multi.h"' in open(os.path.join(ROOT, "include", "sblas_hip.h")).read()
    for name in declared:
        assert hasattr(sblas.lib(), name), name


def test_limits_agree_with_the_header_and_the_solvers(sblas):
    public = open(os.path.join(ROOT, "include", "sblas_hip_amg_multi.h")).read()
    macro = lambda name: int(re.search(r"#define %s (\d+)" % name, public).group(1))
    lim = sblas.amg_multi_limits()
    assert lim == dict(max_rhs=macro("SBLAS_AMG_MULTI_MAX_RHS"), tile=macro("SBLAS_AMG_MULTI_TILE"), threads=sblas.amg_limits()["threads"])
    multi = sblas.krylov_multi_limits()
    assert (lim["max_rhs"], lim["tile"]) == (multi["max_rhs"], multi["tile"]) == (64, 8)
    out = (C.c_int64 * 4)(-7, -7, -7, -7)
    assert sblas.lib().sblas_amg_multi_limits(out) == 0
    assert list(out) == [64, 8, 256, 0]                                      # [3] is reserved
    assert sblas.lib().sblas_amg_multi_limits(None) != 0


def test_the_grid_of_a_row_kernel(sblas):
    """counted by hand: a workgroup of 256 threads holds 64 four-lane units and a tile of 8 columns"""
    for units in (0, 1, 63, 64, 65):
        for s in (1, 7, 8, 9, 64):
            blocks = {0: 0, 1: 1, 63: 1, 64: 1, 65: 2}[units]
            tiles = {1: 1, 7: 1, 8: 1, 9: 2, 64: 8}[s]
            last = {1: 1, 7: 7, 8: 8, 9: 1, 64: 8}[s]
            assert sblas.amg_multi_grid(units, s) == dict(unit_blocks=blocks, tiles=tiles, grid=blocks * tiles, last_tile=last), (units, s)
    for units, s in ((-1, 1), (1, 0), (1, 65), (1, -1)):
        with pytest.raises(sblas.SblasError):
            sblas.amg_multi_grid(units, s)


def test_the_kinds_a_batch_takes_with_a_plan(sblas):
    L = sblas.lib()
    with_plan = {kind: L.sblas_krylov_multi_precond_plan_ok(kind) == 0 for kind in range(-1, 7)}
    assert with_plan == {kind: kind == sblas.PRECOND_AMG for kind in range(-1, 7)}
    # what a batch takes without a plan is what it was
    alone = {kind: L.sblas_krylov_multi_precond_ok(kind) == 0 for kind in range(-1, 7)}
    assert alone == {kind: kind in (sblas.PRECOND_NONE, sblas.PRECOND_JACOBI) for kind in range(-1, 7)}
    rule = open(os.path.join(ROOT, "s-blas_amd", "csrc", "precond_rule.h")).read()
    assert "precond_multi_applied" in rule and "sptrsm" in rule            # the one place, with what the other kinds wait on


def test_launches_with_a_block_cycle(sblas):
    """counted by hand from the sequences DESIGN.md 3.30 lists"""
    L = sblas.lib()
    ex = L.sblas_krylov_multi_launches_ex
    PCG, BICG = 0, 1
    for spmm in (0, 1, 3):
        for cycle in (1, 11, 48):
            pcg = ["spmm"] * spmm + ["dots (p, q)", "fold alpha", "x r update", "fold residual"] + ["cycle"] * cycle + \
                  ["dots (r, z)", "fold beta", "p update"]
            bicg = ["p update"] + ["cycle"] * cycle + ["spmm"] * spmm + ["dots", "fold alpha", "s update"] + ["cycle"] * cycle + \
                   ["spmm"] * spmm + ["dots", "fold omega", "x r update", "fold residual and beta"]
            assert ex(PCG, sblas.PRECOND_AMG, spmm, cycle) == len(pcg) == spmm + 5 + cycle + 2
            assert ex(BICG, sblas.PRECOND_AMG, spmm, cycle) == len(bicg) == 2 * spmm + 8 + 2 * cycle
            for kind in (sblas.PRECOND_ILU0, sblas.PRECOND_CHEBYSHEV, -1, 5, 9):
                assert ex(PCG, kind, spmm, cycle) == -1 and ex(BICG, kind, spmm, cycle) == -1
            for kind in (sblas.PRECOND_NONE, sblas.PRECOND_JACOBI):          # a kind that rides in the kernels has no launches of its own
                assert ex(PCG, kind, spmm, cycle) == -1
        for kind, name in ((sblas.PRECOND_NONE, None), (sblas.PRECOND_JACOBI, "jacobi")):
            for method, code in (("pcg", PCG), ("bicgstab", BICG)):
                assert ex(code, kind, spmm, 0) == L.sblas_krylov_multi_launches(code, kind, spmm) == sblas.krylov_multi_launches(method, name, spmm)
    assert ex(PCG, sblas.PRECOND_AMG, 0, 0) == 7 and ex(BICG, sblas.PRECOND_AMG, 0, 0) == 8
    for bad in ((2, sblas.PRECOND_AMG, 1, 1), (-1, sblas.PRECOND_AMG, 1, 1), (PCG, sblas.PRECOND_AMG, -1, 1), (PCG, sblas.PRECOND_AMG, 1, -1),
                (PCG, sblas.PRECOND_NONE, 1, -1), (BICG, sblas.PRECOND_JACOBI, -1, 0)):
        assert ex(*bad) == -1, bad
    # the old function gives what it gave
    for kind in (sblas.PRECOND_ILU0, sblas.PRECOND_AMG, sblas.PRECOND_CHEBYSHEV):
        assert L.sblas_krylov_multi_launches(PCG, kind, 1) == -1
    for name in ("ilu0", "amg", "chebyshev"):                                # a name carries no plan
        with pytest.raises(sblas.SblasError, match="no multi-column apply"):
            sblas.krylov_multi_launches("pcg", name)


# ---------------------------------------------------------------------------------------------------------------------
# the lockstep loops with a cycle as M^-1 against independent loops: the composition is separable by column
# ---------------------------------------------------------------------------------------------------------------------
def same_solved(got, want):
    ok = KN.same_bits(got.x, want.x) and got.iterations == want.iterations and got.status == want.status
    ok = ok and got.breakdown == want.breakdown
    for name in ("rnorm", "bnorm", "alpha", "beta", "omega"):
        ok = ok and KN.same_bits(getattr(got, name), getattr(want, name))
    return ok


@pytest.fixture(scope="module")
def grid24(sblas):
    c = AN.case("grid24")
    H = AN.hierarchy(c, sblas.amg_aggregate)
    assert [L["n"] for L in H] == [576, 212, 57]
    A = (c["n"], c["rp"], c["ci"], c["val"])
    mv1 = lambda v: KN.matvec(*A, v)
    mvs = lambda V: np.stack([mv1(V[:, j]) for j in range(V.shape[1])], axis=1)
    apply = lambda v: sblas.amg_cycle_ref(H, v).copy()
    B, X0, names = MC.columns(c["n"], mv1)
    return dict(A=A, mv1=mv1, mvs=mvs, apply=apply, B=B, X0=X0, names=names)


@pytest.mark.parametrize("method", ["pcg", "bicgstab"])
def test_lockstep_loops_with_a_cycle_equal_independent_solves(grid24, method):
    g = grid24
    multi, single = (MC.composed_pcg_multi, SC.composed_pcg) if method == "pcg" else (MC.composed_bicgstab_multi, SC.composed_bicgstab)
    got = multi(g["mvs"], g["apply"], KN.dot_np, g["B"], g["X0"], RTOL, 1000)
    assert len(got) == 9
    for j, name in enumerate(g["names"]):
        want = single(g["mv1"], g["apply"], KN.dot_np, g["B"][:, j], g["X0"][:, j], RTOL, 1000)
        assert same_solved(got[j], want), (name, got[j].asdict(), want.asdict())
    by = dict(zip(g["names"], got))
    print("%s with a V-cycle on grid24: %s" % (method, {k: (v.status, v.iterations) for k, v in by.items()}))
    assert (by["zero"].status, by["zero"].iterations) == ("converged", 0) and not by["zero"].x.any()
    assert (by["nan"].status, by["nan"].iterations) == ("breakdown", 0)
    assert by["nan"].breakdown == (SC.DENOM_PQ if method == "pcg" else SC.DENOM_RV)
    assert all(v.status == "converged" for k, v in by.items() if k != "nan")
    assert by["warm 0.001"].iterations >= by["warm 1e-06"].iterations >= by["warm 1e-09"].iterations > 0


def test_python_refusals_need_no_gpu(sblas):
    import torch
    E = sblas.SblasError
    rp = torch.zeros(9, dtype=torch.int32)
    ci = torch.zeros(0, dtype=torch.int32)
    X = torch.zeros(8, 3, dtype=torch.float64)
    for name in ("ilu0", "amg", "chebyshev"):                                # the names stay refused with today's message
        with pytest.raises(E, match="the %s preconditioner has no multi-column apply" % name):
            sblas.KrylovMultiPlan(8, rp, ci, 3, precond=name)
    with pytest.raises(E, match="None or 'jacobi'"):
        sblas.KrylovMultiPlan(8, rp, ci, 3, precond="amg_smoothed")          # the one-shots' word, not a plan's
    for s in (0, 65):
        with pytest.raises(E, match="columns"):
            sblas.amg_sweep_multi(None, 0, torch.zeros(8, s, dtype=torch.float64), None, None)
    with pytest.raises(E, match="GPU tensor"):
        sblas.pcg_multi((8, rp, ci, X), X, precond="amg")
    with pytest.raises(E, match="2-D"):
        sblas.amg_restrict_multi(None, 0, torch.zeros(8), None)


def test_the_rule_check_runs_clean_under_the_sanitizers(tmp_path):
    """tools/amg_multi_rule_check.cpp, host code only and a program of its own, under the address and undefined-behaviour
    sanitizers"""
    cxx = next((p for p in (shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++", shutil.which("g++")) if p and os.path.exists(p)), None)
    if cxx is None:
        pytest.skip("no host compiler")
    csrc = os.path.join(ROOT, "s-blas_amd", "csrc")
    exe = str(tmp_path / "amg_multi_rule_check")
    src = [os.path.join(ROOT, "tools", "amg_multi_rule_check.cpp")] + [os.path.join(csrc, f) for f in ("amg_rule.cpp", "ilu0_plan.cpp",
                                                                                                      "krylov_multi_rule.cpp")]
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                          + src + ["-o", exe])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert done.returncode == 0, done.stdout.decode()
    assert b"amg_multi_rule_check: ok" in done.stdout
