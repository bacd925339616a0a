"""The host side of the device aggregation (amg_rule.cpp through the C ABI): the rule in synchronous rounds
against the greedy walk and against its Python restatement, the pinned round counts, the priority path, one-way edges, the
NaN / Inf / zero classes of the strength bound and the refusals.  Every comparison is ==.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import amg_dev_numerics as DN
import amg_numerics as AN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return {name: AN.case(name) for name in AN.CASES}


def agree(sblas, c, seed=0, level=0, rounds=None):
    """the library's rounds form, the library's greedy walk, the scalar loop and the Python rounds give the same roots"""
    n, rp, ci, val, theta = c["n"], c["rp"], c["ci"], DN.values(c), c["theta"]
    root, got_rounds = sblas.amg_roots_rounds_ref(n, rp, ci, val, theta, seed=seed, level=level)
    agg, aggptr, members = sblas.amg_aggregate(n, rp, ci, val, theta, seed=seed, level=level)
    want_agg, want_ptr, want_members, want_root = AN.aggregate_py(n, rp, ci, val, theta, seed=seed, level=level)
    py_root, py_rounds = DN.rounds_py(n, rp, ci, val, theta, seed=seed, level=level)
    what = (c["name"], seed, level)
    assert root.dtype == bool and len(root) == n
    assert np.array_equal(root, want_root) and np.array_equal(root, py_root) and DN.roots_are_numbered(root, agg, aggptr), what
    assert np.array_equal(agg, want_agg) and np.array_equal(aggptr, want_ptr) and np.array_equal(members, want_members), what
    assert got_rounds == py_rounds, what
    if rounds is not None:
        assert got_rounds == rounds, what
    return root, got_rounds


def test_the_rounds_reference_exists(sblas):
    assert sblas.lib().sblas_amg_roots_rounds_ref                           # fails on the parent commit
    hdr = open(os.path.join(ROOT, "include", "sblas_hip_amg_dev.h")).read()
    declared = set(re.findall(r"\b(sblas_[A-Za-z0-9_]+)\s*\(", hdr))
    assert declared == set(sblas.EXPORTS_AMG_DEV) and not declared & set(sblas.EXPORTS + sblas.EXPORTS_AMG_SA)
    assert '#include "sblas_hip_amg_dev.h"' in open(os.path.join(ROOT, "include", "sblas_hip.h")).read()
    for name in declared:
        assert hasattr(sblas.lib(), name), name


@pytest.mark.parametrize("name", AN.CASES)
def test_rounds_reach_the_greedy_walks_roots(sblas, cases, name):
    c = cases[name]
    root, rounds = agree(sblas, c, rounds=DN.ROUNDS[name])
    print("%s: %d roots of %d in %d rounds" % (name, int(root.sum()), c["n"], rounds))
    if name in ("grid24", "random4000", "aniso32"):                         # other salts: the same equivalence
        agree(sblas, c, seed=7), agree(sblas, c, level=3)


def test_the_priority_path_takes_a_round_a_vertex(sblas):
    c = DN.priority_path(300)
    root, rounds = agree(sblas, c, rounds=300)
    assert int(root.sum()) == 150
    assert len(sblas.amg_aggregate(c["n"], c["rp"], c["ci"])[1]) - 1 == 150
    agree(sblas, c, seed=7)                                                  # under another salt it is just a path


def test_one_way_edges_consult_the_own_row_only(sblas):
    c, pairs = DN.one_way()
    root, _ = agree(sblas, c)
    h = lambda v: AN.priority(v, 0, 0)
    for v, u in pairs:                                                       # u names nobody: always a root
        assert root[u]
    for v in set(v for v, _ in pairs):                                       # v is a root exactly when every vertex it names has the lower h
        assert root[v] == all(h(u) < h(v) for w, u in pairs if w == v), v
    assert any(root[v] for v, _ in pairs) and not all(root[v] for v, _ in pairs)
    assert any(h(u) > h(v) for v, u in pairs) and any(h(u) < h(v) for v, u in pairs)
    agree(sblas, c, seed=7), agree(sblas, c, level=3)


@pytest.mark.parametrize("theta", [0.25, 1.0])
@pytest.mark.parametrize("kind", DN.BOUND_CLASSES)
def test_bound_classes_agree_with_strong_lists(sblas, kind, theta):
    c = DN.bound_class(kind, theta)
    n, rp, ci, val = c["n"], c["rp"], c["ci"], c["val"]
    agree(sblas, c)
    strong = AN.strong_lists(n, rp, ci, val, theta)
    for i in range(0, n, 4):                                                 # what the class means for its rows
        cols = [int(x) for x in ci[rp[i]:rp[i + 1]] if x != i]
        vals = {int(x): v for x, v in zip(ci[rp[i]:rp[i + 1]], val[rp[i]:rp[i + 1]])}
        if kind in ("zeros", "equal"):
            assert strong[i] == cols
        elif kind == "nan":
            assert all(not np.isnan(vals[u]) for u in strong[i]) and len(strong[i]) < len(cols)
        else:
            assert strong[i] == [u for u in cols if np.isinf(vals[u])] and len(strong[i]) == 1


def test_widths_and_the_sweep_agree(sblas):
    for theta in (0.0, 0.3):
        agree(sblas, DN.widths(theta))
    for k in range(DN.SWEEP):
        agree(sblas, DN.sweep_case(k), seed=k)


def test_refusals(sblas, cases):
    c = cases["grid24"]
    n, rp, ci, val = c["n"], c["rp"], c["ci"], c["val"]
    E = sblas.SblasError
    for theta in (float("nan"), -0.1, 1.5):
        with pytest.raises(E):
            sblas.amg_roots_rounds_ref(n, rp, ci, val, theta)
    with pytest.raises(E):
        sblas.amg_roots_rounds_ref(n, rp, ci, None, 0.25)                    # theta > 0 without values
    swapped = ci.copy()
    swapped[rp[5]], swapped[rp[5] + 1] = ci[rp[5] + 1], ci[rp[5]]
    no_diag = ci.copy()
    no_diag[rp[9]:rp[10]][ci[rp[9]:rp[10]] == 9] = 8
    outside = ci.copy()
    outside[rp[30]] = n
    for bad_ci, row in ((swapped, 5), (no_diag, 9), (outside, 30)):
        with pytest.raises(E) as err:
            sblas.amg_roots_rounds_ref(n, rp, bad_ci)
        assert err.value.bad_row == row and "row %d" % row in str(err.value)
        with pytest.raises(E) as err:                                         # the same refusal as the greedy walk's
            sblas.amg_aggregate(n, rp, bad_ci)
        assert err.value.bad_row == row
    L = sblas.lib()
    rounds = C.c_int64(5)
    assert L.sblas_amg_roots_rounds_ref(2 ** 31, rp.ctypes.data, ci.ctypes.data, None, 0.0, 0, 0, None, C.byref(rounds), None) != 0
    assert rounds.value == 0
    assert L.sblas_amg_roots_rounds_ref(n, rp.ctypes.data, ci.ctypes.data, None, 0.0, 0, 0, None, C.byref(rounds), None) != 0   # no root_out
    assert L.sblas_amg_roots_rounds_ref(n, rp.ctypes.data, ci.ctypes.data, None, 0.0, 0, 0, None, None, None) != 0
    assert sblas.amg_roots_rounds_ref(0, np.zeros(1, np.int32), np.zeros(0, np.int32))[1] == 0
    # the device entry points refuse on the host, before anything is launched (no GPU is touched here)
    assert L.sblas_hip_amg_aggregate_workspace(0, 0) == 0 and L.sblas_hip_amg_aggregate_workspace(-1, 0) == 0
    assert L.sblas_hip_amg_aggregate_workspace(2 ** 31, 0) == 0 and L.sblas_hip_amg_aggregate_workspace(1000, 5000) > 1000 * 28
