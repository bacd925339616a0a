"""The host side of the FSAI plan (fsai_rule.cpp through the C ABI): G's pattern and G's values against the
Python restatements of fsai_numerics with ==, the unit diagonal of G A G^T, the failed-row classes, the kind's place in the
preconditioner rule, the iteration counts of a host float64 PCG and the rule check under the sanitizers.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import amg_numerics as AN
import fsai_numerics as FN
import krylov_numerics as KN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-10


def same(a, b):
    return KN.same_bits(a, b)


@pytest.fixture(scope="module")
def reference(sblas):
    """every case's G by the host reference, computed once -> (rowptr_g, colidx_g, val_g, bad_row)"""
    made = {}

    def get(name):
        if name not in made:
            c = FN.case(name)
            grp, gci = sblas.fsai_pattern(c["n"], c["rp"], c["ci"], pattern=c["pattern"], max_row=c["max_row"])
            made[name] = (grp, gci) + sblas.fsai_ref(c["n"], c["rp"], c["ci"], c["val"], grp, gci)
        return made[name]
    return get


def test_the_library_exports_what_the_new_header_declares(sblas):
    hdr = open(os.path.join(ROOT, "include", "sblas_hip_fsai.h")).read()
    declared = set(re.findall(r"\b(sblas_[A-Za-z0-9_]+)\s*\(", hdr))
    others = set(sblas.EXPORTS + sblas.EXPORTS_AMG_SA + sblas.EXPORTS_AMG_DEV + sblas.EXPORTS_CHEBY + sblas.EXPORTS_KRYLOV_MULTI
                 + sblas.EXPORTS_AMG_MULTI + sblas.EXPORTS_SPTRSM_TILE + sblas.EXPORTS_GMRES_MULTI + sblas.EXPORTS_GEAM + sblas.EXPORTS_MSPGEMM
                 + sblas.EXPORTS_SDDMM_NARROW)
    assert declared == set(sblas.EXPORTS_FSAI) and not declared & others, declared ^ set(sblas.EXPORTS_FSAI)
    assert '#include "sblas_hip_fsai.h"' in open(os.path.join(ROOT, "include", "sblas_hip.h")).read()
    for name in declared:
        assert hasattr(sblas.lib(), name), name
    lim = sblas.fsai_limits()
    assert (lim["threads"], lim["row_max"], lim["g4_max"], lim["g16_max"]) == (256, FN.ROW_MAX, 4, 32)
    # every tier's triangle, columns and vector fit the LDS its lanes own
    for lanes, m in ((4, lim["g4_max"]), (16, lim["g16_max"]), (64, lim["row_max"])):
        assert m * (m + 1) // 2 <= lanes * lim["tri_per_lane"] and m <= lanes * lim["vec_per_lane"]
    assert lim["lds_bytes"] == lim["threads"] * (8 * lim["tri_per_lane"] + 12 * lim["vec_per_lane"]) and 2 * lim["lds_bytes"] <= 160 * 1024
    assert sblas.PRECOND_FSAI == 6 and re.search(r"#define SBLAS_PRECOND_FSAI 6\b", hdr)


@pytest.mark.parametrize("name", FN.CASES)
def test_the_pattern_and_the_values_equal_the_restatement(sblas, reference, name):
    c = FN.case(name)
    n, rp, ci, val = c["n"], c["rp"], c["ci"], c["val"]
    grp, gci, gval, bad = reference(name)
    wrp, wci = FN.pattern(n, rp, ci, c["pattern"], c["max_row"])
    assert np.array_equal(grp, wrp) and np.array_equal(gci, wci) and grp.dtype == gci.dtype == np.int32
    want, wbad = FN.values(n, rp, ci, val, grp, gci)
    assert same(gval, want) and bad is None and wbad is None
    rows = np.diff(grp)
    if n:
        assert rows.min() >= 1 and rows.max() <= (c["max_row"] or FN.ROW_MAX) and np.array_equal(gci[grp[1:] - 1], np.arange(n))
        G = FN.dense_g(n, grp, gci, gval)
        err = float(np.abs(np.diag(G @ c["dense"] @ G.T) - 1.0).max())
        print("%s: n %d, nnz(G) %d, longest row %d, |diag(G A G^T) - 1| <= %.3g" % (name, n, len(gci), rows.max(), err))
        assert err <= 1e-12
    if c["pattern"] is not None:                                            # positions A does not store gather +0.0: the pattern is wider than A's
        assert len(gci) > len(FN.pattern(n, rp, ci)[1])


def test_the_cases_reach_every_tier_and_the_thinning(sblas, reference):
    lim = sblas.fsai_limits()
    longest = {name: int(np.diff(reference(name)[0]).max()) for name in FN.CASES if FN.case(name)["n"]}
    assert longest["tridiagonal300"] == 2 and longest["grid24"] == 3 and longest["band6"] == 7 and longest["band20"] == 21
    assert longest["band20_max8"] == 8 and longest["band20_max1"] == 1 and longest["clique70_max64"] == 64
    assert longest["grid12_squared"] > longest["grid24"]
    rows = np.diff(reference("mixed70")[0])
    tier = np.where(rows <= lim["g4_max"], 0, np.where(rows <= lim["g16_max"], 1, 2))
    assert set(tier[:64]) == {0, 1, 2}                                      # all three inside one wave's worth of rows
    c = FN.case("clique70_max64")
    with pytest.raises(sblas.SblasError) as err:
        sblas.fsai_pattern(c["n"], c["rp"], c["ci"])
    assert err.value.bad_row == 64                                          # the first row with 65 entries up to its diagonal
    # max_row keeps the diagonal and the entries of largest column below it
    grp, gci = reference("band20_max8")[:2]
    assert [int(v) for v in gci[grp[100]:grp[101]]] == list(range(93, 101))


def test_the_pattern_function_refuses_by_row(sblas):
    S, E = sblas, sblas.SblasError
    c = FN.case("grid12_squared")
    n, rp, ci = c["n"], c["rp"], c["ci"]
    prp, pci = c["pattern"]
    full_rp, full_ci = FN.csr_of((np.abs(c["dense"]) @ np.abs(c["dense"])) != 0)[1:3]
    a, b = S.fsai_pattern(n, rp, ci, pattern=(full_rp, full_ci)), S.fsai_pattern(n, rp, ci, pattern=(prp, pci))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])        # entries above the diagonal are ignored
    strict = pci[pci != np.repeat(np.arange(n), np.diff(prp))]
    strict_rp = (prp - np.arange(n + 1)).astype(np.int32)
    swapped = pci.copy()
    swapped[prp[9]], swapped[prp[9] + 1] = pci[prp[9] + 1], pci[prp[9]]
    outside = pci.copy()
    outside[prp[5]] = -1
    unsorted = ci.copy()
    unsorted[rp[7]], unsorted[rp[7] + 1] = ci[rp[7] + 1], ci[rp[7]]
    for call, row in ((lambda: S.fsai_pattern(n, rp, ci, pattern=(strict_rp, strict)), 0),      # no row holds its diagonal
                      (lambda: S.fsai_pattern(n, rp, ci, pattern=(prp, swapped)), 9),
                      (lambda: S.fsai_pattern(n, rp, ci, pattern=(prp, outside)), 5),
                      (lambda: S.fsai_pattern(n, rp, unsorted), 7)):
        with pytest.raises(E) as err:
            call()
        assert err.value.bad_row == row
    for k in (0, 65, -1, 2.0, True):
        with pytest.raises(E):
            S.fsai_pattern(n, rp, ci, max_row=k)
    with pytest.raises(E):
        S.fsai_pattern(n, rp[:-1], ci)
    with pytest.raises(E):
        S.fsai_ref(n, rp, ci, c["val"][:-1], prp, pci)
    with pytest.raises(E):
        S.fsai_ref(n, rp, ci, c["val"], full_rp, full_ci)                  # not a pattern of G: rows must end on the diagonal


@pytest.mark.parametrize("name", sorted(FN.failures()))
def test_a_failed_row_is_its_diagonal_alone_and_the_least_is_named(sblas, name):
    n, rp, ci, val, row = FN.failures()[name]
    grp, gci = sblas.fsai_pattern(n, rp, ci)
    gval, bad = sblas.fsai_ref(n, rp, ci, val, grp, gci)
    want, wbad = FN.values(n, rp, ci, val, grp, gci)
    assert same(gval, want) and bad == wbad == row
    g = gval[grp[row]:grp[row + 1]]
    diag = val[rp[row]:rp[row + 1]][ci[rp[row]:rp[row + 1]] == row][0]
    fallback = 1.0 / np.sqrt(diag) if diag > 0.0 and np.isfinite(diag) else 1.0
    assert same(g[-1], fallback) and same(g[:-1], np.zeros(len(g) - 1))     # +0.0 beside the diagonal
    assert same(gval[grp[0]:grp[1]], want[grp[0]:grp[1]]) and np.isfinite(gval).all()


def test_the_kind_rule_holds(sblas):
    S, L = sblas, sblas.lib()
    info = (C.c_int64 * 12)()
    out = (C.c_int64 * 4)()
    info[5] = 2
    assert L.sblas_krylov_launches(0, 6, info, None) == S.krylov_launches("pcg", "fsai", 2) == 8 + 2       # known and applied
    assert L.sblas_krylov_launches(1, 6, info, None) == S.krylov_launches("bicgstab", "fsai", 2) == 10 + 2 * 2
    g = S.gmres_launches(30, "fsai", 2)
    assert (g["step"], g["close"], g["restart"], g["start"]) == (9 + 2, 3 + 2, 4, 6)
    assert L.sblas_krylov_launches(0, 6, None, None) == -1 and L.sblas_gmres_launches(30, 6, None, None, out) == -1   # an applied kind needs its info
    assert L.sblas_krylov_launches(0, 6, info, info) == 8 + 2                                          # not a pair: the upper info is not read
    assert L.sblas_krylov_launches(0, 5, info, None) == -1 and L.sblas_gmres_launches(30, 5, info, None, out) == -1   # 5 is still no kind
    assert L.sblas_krylov_launches(0, 7, info, None) == -1 and L.sblas_krylov_launches(0, 9, info, None) == -1
    for kind in (5, 6):                                                     # the multi-right-hand-side rules refuse both
        assert L.sblas_krylov_multi_precond_ok(kind) != 0 and L.sblas_krylov_multi_precond_plan_ok(kind) != 0
        assert L.sblas_krylov_multi_precond_pair_ok(kind) != 0
        assert L.sblas_gmres_multi_precond_ok(kind) != 0 and L.sblas_gmres_multi_precond_plan_ok(kind) != 0
        assert L.sblas_gmres_multi_precond_pair_ok(kind) != 0
        assert L.sblas_krylov_multi_launches(0, kind, 1) == -1 and L.sblas_krylov_multi_launches_ex(0, kind, 1, 2) == -1
    assert S._PRECOND_NAME[6] == "fsai" and S._PRECOND_NAME[5] is None and S._PRECOND_CODE["fsai"] == 6 and S._PRECOND_CODE[None] == 0
    assert 5 not in S._PRECOND_CODE.values()
    with pytest.raises(S.SblasError, match="the fsai preconditioner has no multi-column apply: several right-hand sides take None or 'jacobi'$"):
        S.krylov_multi_launches("pcg", "fsai")


@pytest.mark.parametrize("side", [24, 32])
def test_a_host_pcg_takes_fewer_iterations_with_g(sblas, side):
    """float64 PCG on the five-point Laplacian with the reference G; DESIGN.md 3.39 records the counts this prints"""
    n, rp, ci, val = KN.laplacian(side)
    rp, ci = rp.astype(np.int32), ci.astype(np.int32)
    b = np.random.default_rng(30).standard_normal(n)
    plain, _ = AN.host_pcg(n, rp, ci, val, b, lambda r: r.copy(), RTOL)
    counts = {}
    for what, pat in (("A", None), ("A^2", FN.lower_of_square(rp, ci))):
        grp, gci = sblas.fsai_pattern(n, rp, ci, pattern=pat)
        gval, bad = sblas.fsai_ref(n, rp, ci, val, grp, gci)
        G = FN.dense_g(n, grp, gci, gval)
        counts[what], x = AN.host_pcg(n, rp, ci, val, b, lambda r: G.T @ (G @ r), RTOL)
        assert bad is None and np.linalg.norm(b - KN.matvec(n, rp, ci, val, x)) <= 10 * RTOL * np.linalg.norm(b)
    print("%d^2 Laplacian: plain CG %d iterations, FSAI on A's lower pattern %d, on the lower pattern of A^2 %d" % (side, plain, counts["A"], counts["A^2"]))
    assert counts["A^2"] < counts["A"] < plain


def test_the_rule_check_runs_clean_under_the_sanitizers(tmp_path):
    """tools/fsai_rule_check.cpp, host code only and a program of its own, under the address and undefined-behaviour
    sanitizers of every host compiler there is"""
    found = [p for p in (shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++", shutil.which("g++")) if p and os.path.exists(p)]
    assert found, "no host compiler"
    csrc = os.path.join(ROOT, "s-blas_amd", "csrc")
    src = [os.path.join(ROOT, "tools", "fsai_rule_check.cpp")] + [os.path.join(csrc, f) for f in ("fsai_rule.cpp", "ilu0_plan.cpp")]
    for k, cxx in enumerate(found):
        exe = str(tmp_path / ("fsai_rule_check_%d" % k))
        subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-w", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                              + src + ["-o", exe])
        done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        assert done.returncode == 0, done.stdout.decode()
        assert b"fsai_rule_check: ok" in done.stdout
