"""The tiled triangular solve's host side and the rule of ILU(0)'s seat under the multi-right-hand-side solvers
(sptrsv_plan.cpp, krylov_multi_rule.cpp, precond_rule.h; no GPU): the new header against its export list, the limits and
the grid of a wide launch, which preconditioner kinds a multi-right-hand-side plan takes WITH a pair of solve plans, the
launches of an iteration with the two solves in it, and the lockstep loops of tests/multi_compose.py with a column-wise
host U^-1 L^-1 as `apply` against independent single loops."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

import ilu0_numerics as IN
import krylov_numerics as KN
import multi_compose as MC
import solver_compose as SC
from conftest import ROOT

RTOL = 1e-10


def test_the_library_exports_what_the_new_header_declares(sblas):
    hdr = open(os.path.join(ROOT, "include", "sblas_hip_sptrsm_tile.h")).read()
    declared = set(re.findall(r"\b(sblas_[A-Za-z0-9_]+)\s*\(", hdr))
    others = set(sblas.EXPORTS + sblas.EXPORTS_AMG_SA + sblas.EXPORTS_AMG_DEV + sblas.EXPORTS_CHEBY + sblas.EXPORTS_KRYLOV_MULTI +
                 sblas.EXPORTS_AMG_MULTI)
    assert declared == set(sblas.EXPORTS_SPTRSM_TILE) and not declared & others, declared ^ set(sblas.EXPORTS_SPTRSM_TILE)
    assert len(set(sblas.EXPORTS_SPTRSM_TILE)) == len(sblas.EXPORTS_SPTRSM_TILE)
    assert '#include "sblas_hip_sptrsm_tile.h"' in open(os.path.join(ROOT, "include", "sblas_hip.h")).read()
    for name in declared:
        assert hasattr(sblas.lib(), name), name


def test_limits_agree_with_the_header_and_the_single_solve(sblas):
    public = open(os.path.join(ROOT, "include", "sblas_hip_sptrsm_tile.h")).read()
    tile = int(re.search(r"#define SBLAS_SPTRSM_TILE (\d+)", public).group(1))
    lim = sblas.sptrsm_tile_limits()
    assert lim == dict(tile=tile, wide_threads=256, chain_threads=sblas.sptrsv_limits()["chain_threads"], max_grid=2 ** 31 - 1)
    assert lim["tile"] == sblas.krylov_multi_limits()["tile"] == sblas.amg_multi_limits()["tile"] == 8
    out = (C.c_int64 * 4)(-7, -7, -7, -7)
    assert sblas.lib().sblas_sptrsm_tile_limits(out) == 0
    assert list(out) == [8, 256, 1024, 2 ** 31 - 1]
    assert sblas.lib().sblas_sptrsm_tile_limits(None) != 0


def test_the_grid_of_a_wide_launch(sblas):
    """counted by hand: a workgroup of 256 threads holds 64 four-lane units and a tile of 8 columns"""
    for units in (0, 1, 63, 64, 65):
        for s in (1, 7, 8, 9, 64):
            blocks = {0: 0, 1: 1, 63: 1, 64: 1, 65: 2}[units]
            tiles = {1: 1, 7: 1, 8: 1, 9: 2, 64: 8}[s]
            last = {1: 1, 7: 7, 8: 8, 9: 1, 64: 8}[s]
            assert sblas.sptrsm_tile_grid(units, s) == dict(unit_blocks=blocks, tiles=tiles, grid=blocks * tiles, last_tile=last), (units, s)
    # no cap at 64 columns: the grid is the limit
    assert sblas.sptrsm_tile_grid(65, 65) == dict(unit_blocks=2, tiles=9, grid=18, last_tile=1)
    assert sblas.sptrsm_tile_grid(64, 8 * (2 ** 31 - 1))["grid"] == 2 ** 31 - 1
    for units, s in ((-1, 1), (1, 0), (1, -1), (64, 8 * (2 ** 31 - 1) + 1), (65, 8 * 2 ** 30 + 1), (2 ** 40, 2 ** 40)):
        with pytest.raises(sblas.SblasError):
            sblas.sptrsm_tile_grid(units, s)


def test_the_kinds_a_batch_takes_with_a_pair(sblas):
    L = sblas.lib()
    with_pair = {kind: L.sblas_krylov_multi_precond_pair_ok(kind) == 0 for kind in range(-1, 7)}
    assert with_pair == {kind: kind == sblas.PRECOND_ILU0 for kind in range(-1, 7)}
    # what a batch takes with one plan, and without one, is what it was
    with_plan = {kind: L.sblas_krylov_multi_precond_plan_ok(kind) == 0 for kind in range(-1, 7)}
    assert with_plan == {kind: kind == sblas.PRECOND_AMG for kind in range(-1, 7)}
    alone = {kind: L.sblas_krylov_multi_precond_ok(kind) == 0 for kind in range(-1, 7)}
    assert alone == {kind: kind in (sblas.PRECOND_NONE, sblas.PRECOND_JACOBI) for kind in range(-1, 7)}
    rule = open(os.path.join(ROOT, "s-blas_amd", "csrc", "precond_rule.h")).read()
    assert "precond_multi_pair" in rule and "sptrsm" in rule


def test_launches_with_a_pair(sblas):
    """counted by hand: the sequences of DESIGN.md 3.30 with the two solves in the cycle's place"""
    L = sblas.lib()
    pair = L.sblas_krylov_multi_launches_pair
    PCG, BICG, ILU = 0, 1, sblas.PRECOND_ILU0
    for spmm in (0, 1, 3):
        for lo in (1, 11, 48):
            for hi in (1, 11, 48):
                pcg = ["spmm"] * spmm + ["dots (p, q)", "fold alpha", "x r update", "fold residual"] + ["L solve"] * lo + ["U solve"] * hi + \
                      ["dots (r, z)", "fold beta", "p update"]
                bicg = ["p update"] + ["L solve"] * lo + ["U solve"] * hi + ["spmm"] * spmm + ["dots", "fold alpha", "s update"] + \
                       ["L solve"] * lo + ["U solve"] * hi + ["spmm"] * spmm + ["dots", "fold omega", "x r update", "fold residual and beta"]
                assert pair(PCG, ILU, spmm, lo, hi) == len(pcg) == spmm + 5 + lo + hi + 2
                assert pair(BICG, ILU, spmm, lo, hi) == len(bicg) == 2 * spmm + 8 + 2 * (lo + hi)
                assert pair(PCG, ILU, spmm, lo, hi) == L.sblas_krylov_multi_launches_ex(PCG, sblas.PRECOND_AMG, spmm, lo + hi)
                for kind in (sblas.PRECOND_NONE, sblas.PRECOND_JACOBI, sblas.PRECOND_AMG, sblas.PRECOND_CHEBYSHEV, -1, 5, 9):
                    assert pair(PCG, kind, spmm, lo, hi) == -1 and pair(BICG, kind, spmm, lo, hi) == -1
    assert pair(PCG, ILU, 0, 0, 0) == 7 and pair(BICG, ILU, 0, 0, 0) == 8
    for bad in ((2, ILU, 1, 1, 1), (-1, ILU, 1, 1, 1), (PCG, ILU, -1, 1, 1), (PCG, ILU, 1, -1, 1), (BICG, ILU, 1, 1, -1)):
        assert pair(*bad) == -1, bad
    # the older functions give what they gave
    for method in (PCG, BICG):
        assert L.sblas_krylov_multi_launches(method, ILU, 1) == -1
        assert L.sblas_krylov_multi_launches_ex(method, ILU, 1, 2) == -1 and L.sblas_krylov_multi_launches_ex(method, ILU, 1, 0) == -1


# ---------------------------------------------------------------------------------------------------------------------
# the lockstep loops with U^-1 L^-1 as M^-1 against independent loops: the composition is separable by column
# ---------------------------------------------------------------------------------------------------------------------
def same_solved(got, want):
    ok = KN.same_bits(got.x, want.x) and got.iterations == want.iterations and got.status == want.status
    ok = ok and got.breakdown == want.breakdown
    for name in ("rnorm", "bnorm", "alpha", "beta", "omega"):
        ok = ok and KN.same_bits(getattr(got, name), getattr(want, name))
    return ok


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


@pytest.fixture(scope="module")
def cases():
    made = {}
    for method, A in (("pcg", KN.laplacian(16)), ("bicgstab", KN.convection_diffusion(14))):
        n, rp, ci, val = A
        mv1 = lambda v, A=A: KN.matvec(*A, v)
        mvs = lambda V, mv1=mv1: np.stack([mv1(V[:, j]) for j in range(V.shape[1])], axis=1)
        apply = host_ilu_apply(n, rp, ci, IN.ilu0_ref(n, rp, ci, val))
        B, X0, names = MC.columns(n, mv1)
        made[method] = dict(mv1=mv1, mvs=mvs, apply=apply, B=B, X0=X0, names=names)
    return made


@pytest.mark.parametrize("method", ["pcg", "bicgstab"])
def test_lockstep_loops_with_the_two_solves_equal_independent_solves(cases, method):
    g = cases[method]
    multi, single = (MC.composed_pcg_multi, SC.composed_pcg) if method == "pcg" else (MC.composed_bicgstab_multi, SC.composed_bicgstab)
    got = multi(g["mvs"], g["apply"], KN.dot_np, g["B"], g["X0"], RTOL, 1000)
    assert len(got) == 9
    for j, name in enumerate(g["names"]):
        want = single(g["mv1"], g["apply"], KN.dot_np, g["B"][:, j], g["X0"][:, j], RTOL, 1000)
        assert same_solved(got[j], want), (name, got[j].asdict(), want.asdict())
    by = dict(zip(g["names"], got))
    print("%s with ILU(0): %s" % (method, {k: (v.status, v.iterations) for k, v in by.items()}))
    assert (by["zero"].status, by["zero"].iterations) == ("converged", 0) and not by["zero"].x.any()
    assert by["nan"].status != "converged"
    assert all(v.status == "converged" for k, v in by.items() if k != "nan")


def test_python_refusals_need_no_gpu(sblas):
    import torch
    E = sblas.SblasError
    rp = torch.zeros(9, dtype=torch.int32)
    ci = torch.zeros(0, dtype=torch.int32)
    X = torch.zeros(8, 3, dtype=torch.float64)
    # the name stays refused with the message the older suites match, which now points at the pair
    with pytest.raises(E, match=r"the ilu0 preconditioner has no multi-column apply.*ilu\.solvers\(\)"):
        sblas.KrylovMultiPlan(8, rp, ci, 3, precond="ilu0")
    with pytest.raises(E, match="the ilu0 preconditioner has no multi-column apply"):
        sblas.krylov_multi_launches("pcg", "ilu0")
    for name in ("amg", "chebyshev"):                                       # the other names say what they said
        with pytest.raises(E, match="the %s preconditioner has no multi-column apply: several right-hand sides take None or 'jacobi'$" % name):
            sblas.KrylovMultiPlan(8, rp, ci, 3, precond=name)
    for pair in ((None, None), ("lower", "upper"), (1, 2, 3)):               # a pair is two SptrsvPlans
        with pytest.raises(E):
            sblas.KrylovMultiPlan(8, rp, ci, 3, precond=pair)
    # solve_multi's checks come before anything touches the device
    fake = types.SimpleNamespace(n=8, nnz=0, device=torch.device("cpu"))
    with pytest.raises(E, match="GPU tensor"):
        sblas.SptrsvPlan.solve_multi(fake, torch.zeros(0, dtype=torch.float64), X)
    for units, s in ((-1, 1), (1, 0)):
        with pytest.raises(E):
            sblas.sptrsm_tile_grid(units, s)


def test_the_rule_check_runs_clean_under_the_sanitizers(tmp_path):
    """tools/sptrsm_tile_rule_check.cpp, host code only and a program of its own, under the address and
    undefined-behaviour sanitizers"""
    cxx = next((p for p in (shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++", shutil.which("g++")) if p and os.path.exists(p)), None)
    if cxx is None:
        pytest.skip("no host compiler")
    csrc = os.path.join(ROOT, "s-blas_amd", "csrc")
    exe = str(tmp_path / "sptrsm_tile_rule_check")
    src = [os.path.join(ROOT, "tools", "sptrsm_tile_rule_check.cpp")] + [os.path.join(csrc, f) for f in ("sptrsv_plan.cpp", "krylov_multi_rule.cpp")]
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                          + src + ["-o", exe])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert done.returncode == 0, done.stdout.decode()
    assert b"sptrsm_tile_rule_check: ok" in done.stdout
