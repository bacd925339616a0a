"""The host side of smoothed aggregation (amg_rule.cpp through the C ABI): the coarsening guard, the
prolongator, the transfers' row product and the cycle with general P and R against the numpy restatements with ==, the
level sizes, the refusals and the iteration counts of a host float64 PCG.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

import amg_numerics as AN
import amg_sa_numerics as SA
import krylov_numerics as KN


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(a, b):
    return KN.same_bits(a, b)


def test_the_library_exports_what_the_new_header_declares(sblas):
    hdr = open(os.path.join(ROOT, "include", "sblas_hip_amg_sa.h")).read()
    declared = set(re.findall(r"\b(sblas_[A-Za-z0-9_]+)\s*\(", hdr))
    assert declared == set(sblas.EXPORTS_AMG_SA) and not declared & set(sblas.EXPORTS), declared ^ set(sblas.EXPORTS_AMG_SA)
    assert '#include "sblas_hip_amg_sa.h"' in open(os.path.join(ROOT, "include", "sblas_hip.h")).read()
    for name in declared:
        assert hasattr(sblas.lib(), name), name


def test_keep_level_is_the_python_expression(sblas):
    assert sblas.lib().sblas_amg_keep_level                                 # the symbol this file is about
    for m in (0.0, 0.2, 1.0 / 3.0, 0.5, 0.999, math.nextafter(1.0, 0.0)):
        for n in (0, 1, 2, 3, 5, 10, 64, 65, 1000, 5000, 16384, 2 ** 31 - 65):
            edge = int(math.floor((1.0 - m) * n))
            for n_next in {0, 1, max(edge - 1, 0), edge, edge + 1, max(n - 1, 0), n, n + 1}:
                assert sblas.amg_keep_level(n, n_next, m) == SA.keep_level(n, n_next, m), (n, n_next, m)
            if 0 < edge < n:                                                   # the boundary: the floor is kept, one more is not
                assert sblas.amg_keep_level(n, edge, m) and not sblas.amg_keep_level(n, edge + 1, m)
    for n in (1, 7, 5000):                                                    # with 0 the rule is "any reduction"
        assert sblas.amg_keep_level(n, n - 1, 0.0) and not sblas.amg_keep_level(n, n, 0.0)
    assert not sblas.amg_keep_level(5000, 4999, 0.2) and sblas.amg_keep_level(5000, 4000, 0.2) and not sblas.amg_keep_level(5000, 4001, 0.2)
    for bad in ((-1, 0, 0.0), (1, -1, 0.0), (4, 2, 1.0), (4, 2, -0.1), (4, 2, float("nan")), (4, 2, float("inf"))):
        with pytest.raises(sblas.SblasError):
            sblas.amg_keep_level(*bad)


@pytest.mark.parametrize("name", SA.CASES)
def test_prolongator_ref_equals_the_restatement(sblas, name):
    c = SA.case(name)
    n, rp, ci, val = c["n"], c["rp"], c["ci"], c["val"]
    agg, aggptr, _ = sblas.amg_aggregate(n, rp, ci, val if c["theta"] > 0.0 else None, c["theta"])
    nc = len(aggptr) - 1
    for omega_p in (SA.OMEGA_P, 0.5, 1.0):
        for values in (val, val * (1.0 + 0.25 * np.sin(np.arange(len(val))))):
            prp, pci, pv = sblas.amg_prolongator_ref(n, rp, ci, values, agg, nc, omega_p)
            wrp, wci, wv = SA.prolongator(n, rp, ci, values, agg, nc, omega_p)
            assert np.array_equal(prp, wrp) and np.array_equal(pci, wci) and same(pv, wv), (name, omega_p)
    row = SA.rows_of(n, prp)
    assert all(np.all(np.diff(pci[prp[i]:prp[i + 1]]) > 0) for i in range(n))   # strictly ascending rows
    if n:                                                                         # every row i stores agg[i]
        assert all(agg[i] in pci[prp[i]:prp[i + 1]] for i in range(n)) and len(row) == len(pci)
    if name == "diagonal300":                                                    # omega_P = 1 on a diagonal matrix: 1 - a_ii / a_ii, stored
        assert np.array_equal(pci, agg) and np.abs(pv).max() <= 2.0 ** -52


# The restatement is the authority.  The design's CPU prototype formed the products with a library whose rows are not in the
# pinned (ascending) order, and "the first root in stored order" reads that order: it had 29 and 50 rows on the grids' third
# level where the rule gives 27 and 46; the tridiagonal's sizes are the prototype's.
LEVEL_SIZES = {"grid24": [576, 212, 27], "grid32": [1024, 378, 46], "tridiagonal3000": [3000, 1292, 413, 116, 33]}


def test_level_sizes_of_the_smoothed_hierarchies(sblas):
    """integer outcomes of the rule (theta = 0: structure only); DESIGN.md 3.25 records them"""
    for name in SA.CASES:
        c, H = SA.built(name, sblas.amg_aggregate)
        print("%s: levels %s, operator complexity %.3f" % (name, SA.sizes(H), SA.operator_complexity(H) if H else 1.0))
        if name in LEVEL_SIZES:
            assert SA.sizes(H) == LEVEL_SIZES[name], name
        for L in H:                                                             # ILU(0)'s structure contract on every level
            for i in range(L["n"]):
                cols = L["colidx"][L["rowptr"][i]:L["rowptr"][i + 1]]
                assert np.all(np.diff(cols) > 0) and i in cols, (name, i)
    assert SA.sizes(SA.built("star5000", sblas.amg_aggregate)[1]) == [5000]        # the guard: 4999 of 5000 is no coarsening
    assert SA.sizes(SA.built("diagonal300", sblas.amg_aggregate)[1]) == [300]
    assert len(SA.hierarchy(SA.case("star5000"), sblas.amg_aggregate, "plain")) == 20   # unguarded and plain: as before
    assert SA.sizes(SA.hierarchy(SA.case("star5000"), sblas.amg_aggregate, "plain", min_reduction=0.2)) == [5000]
    assert SA.sizes(SA.hierarchy(AN.case("grid24"), sblas.amg_aggregate, "plain")) == [576, 212, 57]
    groups = set()
    for name in ("random600", "clique130", "grid24"):
        for L in SA.built(name, sblas.amg_aggregate)[1][:-1]:
            for key in ("rowptr", "p_rowptr", "r_rowptr"):
                groups |= set(AN.group(int(p)) for p in np.diff(L[key]))
    assert groups == {4, 16, 64}                                                 # all three lane groups occur
    assert np.diff(SA.built("clique130", sblas.amg_aggregate)[1][0]["r_rowptr"]).max() == 130


@pytest.mark.parametrize("name", SA.CASES)
def test_transfer_and_cycle_refs_equal_the_restatements(sblas, name):
    c, H = SA.built(name, sblas.amg_aggregate)
    rng = np.random.default_rng(7)
    for L in H[:-1]:
        n, nc = L["n"], len(L["r_rowptr"]) - 1
        res, e, x = rng.standard_normal(n), rng.standard_normal(nc), rng.standard_normal(n)
        assert same(sblas.amg_transfer_ref("restrict", L["r_rowptr"], L["r_colidx"], L["r_val"], res),
                    SA.transfer(L["r_rowptr"], L["r_colidx"], L["r_val"], res))
        for scale in (1.0, 1.5):
            assert same(sblas.amg_transfer_ref("prolong", L["p_rowptr"], L["p_colidx"], L["p_val"], e, out=x, scale=scale),
                        x + np.float64(scale) * SA.transfer(L["p_rowptr"], L["p_colidx"], L["p_val"], e))
    r = rng.standard_normal(c["n"])
    for smoother in ("jacobi", "l1"):
        Hs = [dict(L, wd=AN.weights(L["n"], L["rowptr"], L["colidx"], L["val"], smoother)) for L in H]
        for nu in (1, 2):
            for scale in (1.0, 1.5):
                got = sblas.amg_cycle_sa_ref(Hs, r, nu=nu, coarse_sweeps=8 if nu == 1 else 3, coarse_scale=scale)
                want = SA.cycle_py(Hs, r, nu, 8 if nu == 1 else 3, scale) if c["n"] else np.zeros(0)
                assert same(got, want), (name, smoother, nu, scale)


def test_refusals(sblas):
    S, E = sblas, sblas.SblasError
    c, H = SA.built("grid24", S.amg_aggregate)
    n, rp, ci, val = c["n"], c["rp"], c["ci"], c["val"]
    L = H[0]
    nc = len(L["aggptr"]) - 1
    r = np.ones(n)
    no_diag_ci = ci.copy()
    no_diag_ci[rp[3]:rp[4]][ci[rp[3]:rp[4]] == 3] = 2                           # row 3 loses its diagonal
    bad = [lambda: S.amg_prolongator_ref(n, rp, ci, val, L["agg"], nc, 0.0), lambda: S.amg_prolongator_ref(n, rp, ci, val, L["agg"], nc, -1.0),
           lambda: S.amg_prolongator_ref(n, rp, ci, val, L["agg"], nc, float("nan")),
           lambda: S.amg_prolongator_ref(n, rp, ci, val, L["agg"], nc, float("inf")),
           lambda: S.amg_prolongator_ref(n, rp, ci, val, L["agg"], nc - 1),      # an aggregate beyond n_agg
           lambda: S.amg_prolongator_ref(n, rp, ci, val, L["agg"][:-1], nc), lambda: S.amg_prolongator_ref(n, rp, ci, val[:-1], L["agg"], nc),
           lambda: S.amg_transfer_ref("inject", L["r_rowptr"], L["r_colidx"], L["r_val"], r),
           lambda: S.amg_transfer_ref("prolong", L["p_rowptr"], L["p_colidx"], L["p_val"], np.ones(nc)),   # no out
           lambda: S.amg_transfer_ref("restrict", L["r_rowptr"], L["r_colidx"], L["r_val"], r[:-1]),
           lambda: S.amg_cycle_sa_ref(H, r, nu=0), lambda: S.amg_cycle_sa_ref(H, r, coarse_sweeps=0), lambda: S.amg_cycle_sa_ref(H, r[:-1])]
    for k, call in enumerate(bad):
        with pytest.raises(E):
            call()
            pytest.fail("call %d was accepted" % k)
    with pytest.raises(E) as err:
        S.amg_prolongator_ref(n, rp, no_diag_ci, val, L["agg"], nc)
    assert err.value.bad_row == 3
    lib = S.lib()
    z = np.zeros(n)
    assert lib.sblas_amg_transfer_ref(0, n, rp.ctypes.data, ci.ctypes.data, val.ctypes.data, 1.0, z.ctypes.data, z.ctypes.data) != 0   # out is in
    assert lib.sblas_amg_transfer_ref(2, n, rp.ctypes.data, ci.ctypes.data, val.ctypes.data, 1.0, r.ctypes.data, z.ctypes.data) != 0
    assert lib.sblas_amg_cycle_sa_ref(1, None, None, None, None, None, None, None, None, None, None, None, 1, 8, 1.0, None, None) != 0
    assert lib.sblas_amg_cycle_sa_ref(0, None, None, None, None, None, None, None, None, None, None, None, 1, 8, 1.0, None, None) == 0
    assert np.array_equal(z, np.zeros(n))
    assert len(S.amg_cycle_sa_ref([], np.zeros(0))) == 0


def test_host_pcg_counts_stop_growing_with_the_grid(sblas):
    """Host float64 PCG to 1e-10 with the C reference cycle, b from default_rng(30): DESIGN.md 3.25 records the counts this
    prints.  The bar is the issue's: smoothed at 64^2 takes at most what plain aggregation takes at 24^2."""
    counts = {}
    for side in (24, 32, 64):
        n, rp, ci, val = KN.laplacian(side)
        c = dict(n=n, rp=rp.astype(np.int32), ci=ci.astype(np.int32), val=val, theta=0.0)
        b = np.random.default_rng(30).standard_normal(n)
        H = SA.hierarchy(c, sblas.amg_aggregate)
        plain = AN.hierarchy(c, sblas.amg_aggregate)
        it, x = AN.host_pcg(n, rp, ci, val, b, lambda r: sblas.amg_cycle_sa_ref(H, r), 1e-10)
        it_plain, _ = AN.host_pcg(n, rp, ci, val, b, lambda r: sblas.amg_cycle_ref(plain, r), 1e-10)
        assert np.linalg.norm(b - KN.matvec(n, rp, ci, val, x)) <= 1e-9 * np.linalg.norm(b)
        counts[side] = (it, it_plain)
        print("%d^2: smoothed %s in %d iterations (operator complexity %.2f), plain %s in %d"
              % (side, SA.sizes(H), it, SA.operator_complexity(H), SA.sizes(plain), it_plain))
    assert counts[64][0] <= counts[24][1]
