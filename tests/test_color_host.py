"""The colouring rule without a GPU: color_ref (sblas_csr_color) against the restatement in tests/color_numerics.py with
==, the colour and round counts of the CPU prototype, every refusal with its row, the limits against csrc/color.h, and
what the order promises the level-scheduled solves."""
import functools
import os
import re

import numpy as np
import pytest

import color_numerics as CN
import ilu0_numerics as IN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = CN.cases()


@functools.lru_cache(maxsize=None)
def reference(name, seed):
    n, rp, ci, _ = CASES[name]
    color = CN.color_scalar(n, rp, ci, seed)
    par, rounds = CN.color_rounds(n, rp, ci, seed)
    assert np.array_equal(color, par), "%s: the parallel form disagrees with the scalar loop" % name
    return color, rounds


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_color_ref_equals_the_numpy_rule(sblas, name, seed):
    n, rp, ci, _ = CASES[name]
    want, rounds = reference(name, seed)
    color, k, sync = sblas.color_ref(n, rp, ci, seed)
    assert color.dtype == np.int32 and np.array_equal(color, want)
    assert k == (int(want.max()) + 1 if n else 0)
    assert sync == rounds
    CN.check_coloring(n, rp, ci, color, k)


def test_counts_of_the_prototype(sblas):
    got = {}
    for name in ("grid48", "tridiagonal3000", "band600", "block_diagonal"):
        n, rp, ci, _ = CASES[name]
        _, k, sync = sblas.color_ref(n, rp, ci, 0)
        got[name] = (k, sync)
    assert got == dict(grid48=(5, 9), tridiagonal3000=(3, 6), band600=(31, 52), block_diagonal=(70, 70))
    assert sblas.color_ref(*CASES["diagonal"][:3])[1:] == (1, 1)
    assert sblas.color_ref(*CASES["n0"][:3])[1:] == (0, 0)
    assert sblas.color_ref(*CASES["n1"][:3])[1:] == (1, 1)
    assert sblas.color_ref(*CASES["clique130"][:3])[1:] == (130, 130)
    assert sblas.color_ref(*CASES["star5000"][:3])[1] == 2
    assert sblas.color_ref(*CASES["random4000"][:3])[1] == 8                # the unsymmetric case of the issue's table


def test_seeds_give_different_colourings(sblas):
    for name in ("grid48", "band600", "random4000"):
        n, rp, ci, _ = CASES[name]
        c = [sblas.color_ref(n, rp, ci, seed)[0] for seed in (0, 1, 2)]
        assert not np.array_equal(c[0], c[1]) and not np.array_equal(c[1], c[2]) and not np.array_equal(c[0], c[2])
    n, rp, ci, _ = CASES["grid48"]
    assert np.array_equal(sblas.color_ref(n, rp, ci, -1)[0], sblas.color_ref(n, rp, ci, 0xffffffff)[0])   # seed + 1 wraps to 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_permuted_triangles_have_at_most_colours_levels(sblas, name):
    n, rp, ci, symmetric = CASES[name]
    color, k, _ = sblas.color_ref(n, rp, ci, 0)
    perm, inv, ptr, kk = CN.order(color)
    assert kk == k and np.array_equal(np.sort(perm), np.arange(n))
    rpb, cib, src = CN.permute(n, rp, ci, perm)
    assert np.array_equal(np.asarray(ci)[src], perm[cib])                   # the entry, relabelled
    for lower in (True, False):
        _, levels = sblas.sptrsv_levels(n, rpb, cib, lower=lower, unit_diag=True)
        assert levels <= k
        if symmetric:
            assert levels == k, (name, lower, levels, k)
    for c in range(k):                                                      # every class is an independent set
        cls = set(perm[ptr[c]:ptr[c + 1]].tolist())
        for v in cls:
            assert not (set(ci[rp[v]:rp[v + 1]].tolist()) - {v}) & cls


def refused(S, rp, ci, want):
    with pytest.raises(S.SblasError) as e:
        S.color_ref(len(rp) - 1, rp, ci)
    assert e.value.bad_row == want and "row %d" % want in str(e.value)


def test_bad_structures_name_their_row(sblas):
    rp, ci = IN.csr_of_rows([[0, 1], [0, 1, 3], [1, 2], [0, 3, 4], [2, 4]])
    sblas.color_ref(5, rp, ci)                                              # sound as it stands
    c = ci.copy()
    c[rp[3] + 2] = 5                                                        # row 3: a column == n
    refused(sblas, rp, c, 3)
    c = ci.copy()
    c[rp[1]] = -1                                                           # row 1: a negative column
    refused(sblas, rp, c, 1)
    r = rp.copy()
    r[3] = 4                                                                # row 2 ends before it starts
    refused(sblas, r, ci, 2)
    c = ci.copy()
    c[0] = 9                                                                # ... and rowptr comes before the columns
    refused(sblas, r, c, 2)
    r = rp.copy()
    r[0] = 1
    refused(sblas, r, ci, 0)
    with pytest.raises(sblas.SblasError):
        sblas.color_ref(4, rp, ci)                                          # rowptr of another length


def header_constants():
    """NAME = value of every integer constexpr in sptrsv.h and color.h, names resolved"""
    text = "".join(open(os.path.join(ROOT, "s-blas_amd", "csrc", f)).read() for f in ("sptrsv.h", "color.h"))
    env = {}
    for name, expr in re.findall(r"constexpr\s+(?:int64_t|int)\s+(\w+)\s*=\s*([^;]+);", text):
        env[name] = int(eval(expr, {"__builtins__": {}}, dict(env)))
    return env


def test_limits_are_the_header_s_constants(sblas):
    lim, h = sblas.color_limits(), header_constants()
    assert lim == dict(g4_max=h["COLOR_G4_MAX"], g16_max=h["COLOR_G16_MAX"], window=h["COLOR_WINDOW"], threads=h["COLOR_THREADS"])
    t = sblas.sptrsv_limits()
    assert (lim["g4_max"], lim["g16_max"]) == (t["g4_max"], t["g16_max"])   # the solves' lane groups
    assert lim["window"] == 64 and lim["threads"] % 64 == 0                 # one bit a colour in a 64-bit mask


def test_the_numpy_permutation_sorts_rows_and_keeps_duplicates_in_stored_order():
    rp, ci = IN.csr_of_rows([[2, 0, 2, 1], [1], [0, 0, 2]])
    rpb, cib, src = CN.permute(3, rp, ci, [2, 0, 1])                        # inv = [1, 2, 0]
    assert rpb.tolist() == [0, 3, 7, 8]
    assert cib.tolist() == [0, 1, 1, 0, 0, 1, 2, 2]
    assert src.tolist() == [7, 5, 6, 0, 2, 1, 3, 4]
