"""SpGEMM without a GPU: the numpy reference of tests/spgemm_numerics.py against a dense product on integer-valued data
(where every order of addition is exact) and against itself under a row permutation, and the plan's host rule
(sblas_hip_spgemm_classify, _group_width, _check_nnz), which decides each row's path and cuts the general rows into
chunks."""
import ctypes as C

import numpy as np
import pytest

import spgemm_numerics as GN

INVALID = 1
EMPTY, ROW, GENERAL = 0, 1, 2


def small_pair(rng, m, k, n, sort_b=True):
    rpa, cia, va = GN.random_csr(rng, m, k, 4, sort=False, empty_every=7, integer=True)
    rpb, cib, vb = GN.random_csr(rng, k, n, 5, sort=sort_b, empty_every=5, integer=True)
    return (rpa, cia, va), (rpb, cib, vb)


@pytest.mark.parametrize("m,k,n", [(37, 23, 41), (1, 9, 1), (16, 16, 16)])
def test_reference_equals_the_dense_product_on_integer_grids(m, k, n):
    rng = np.random.default_rng(m * 1000 + n)
    (rpa, cia, va), (rpb, cib, vb) = small_pair(rng, m, k, n)
    # duplicates in A: two steps on the same B row
    cia[1::9] = cia[0:-1:9][:len(cia[1::9])]
    rpc, cic, vc = GN.reference(m, n, rpa, cia, va, rpb, cib, vb)
    Ad, Bd = GN.to_dense(m, k, rpa, cia, va), GN.to_dense(k, n, rpb, cib, vb)
    Pa, Pb = GN.pattern_dense(m, k, rpa, cia), GN.pattern_dense(k, n, rpb, cib)
    want_pattern = (Pa.astype(np.int64) @ Pb.astype(np.int64)) > 0
    assert np.array_equal(GN.pattern_dense(m, n, rpc, cic), want_pattern)
    assert len(cic) == int(want_pattern.sum())                              # no column twice
    for i in range(m):
        row = cic[rpc[i]:rpc[i + 1]]
        assert np.all(np.diff(row) > 0)
    got = GN.to_dense(m, n, rpc, cic, vc)
    assert np.array_equal(got[want_pattern], (Ad @ Bd)[want_pattern])
    assert not got[~want_pattern].any()


def test_reference_keeps_a_cancelled_sum_as_a_stored_zero():
    rpa, cia, va = np.array([0, 2], np.int32), np.array([0, 1], np.int32), np.array([1.0, -1.0])
    rpb, cib, vb = np.array([0, 1, 2], np.int32), np.array([3, 3], np.int32), np.array([2.5, 2.5])
    rpc, cic, vc = GN.reference(1, 4, rpa, cia, va, rpb, cib, vb)
    assert rpc.tolist() == [0, 1] and cic.tolist() == [3]
    assert GN.bits(vc)[0] == GN.bits(np.array([0.0]))[0]


def test_reference_agrees_with_itself_under_a_row_permutation_of_a():
    rng = np.random.default_rng(5)
    m, k, n = 53, 31, 47
    rpa, cia, va = GN.random_csr(rng, m, k, 4, sort=False)
    rpb, cib, vb = GN.random_csr(rng, k, n, 6)
    rpc, cic, vc = GN.reference(m, n, rpa, cia, va, rpb, cib, vb)
    perm = rng.permutation(m)
    lens = np.diff(rpa)[perm]
    rpp = np.zeros(m + 1, np.int32)
    rpp[1:] = np.cumsum(lens)
    take = np.concatenate([np.arange(rpa[i], rpa[i + 1]) for i in perm]).astype(np.int64)
    rpc2, cic2, vc2 = GN.reference(m, n, rpp, cia[take], va[take], rpb, cib, vb)
    for new, old in enumerate(perm):
        a, b = slice(rpc[old], rpc[old + 1]), slice(rpc2[new], rpc2[new + 1])
        assert np.array_equal(cic[a], cic2[b])
        assert np.array_equal(GN.bits(vc[a]), GN.bits(vc2[b]))


# ---------------------------------------------------------------------------------------------------------------------
# the host rule
# ---------------------------------------------------------------------------------------------------------------------
def chunks_ok(path, products, chunk_first, cap):
    general = np.flatnonzero(path == GENERAL)
    assert chunk_first[0] == 0 and chunk_first[-1] == len(general)
    assert np.all(np.diff(chunk_first) > 0)                                 # consecutive, none empty, each row once
    for c in range(len(chunk_first) - 1):
        rows = general[chunk_first[c]:chunk_first[c + 1]]
        assert len(rows) == 1 or int(products[rows].sum()) <= cap


def test_limits_are_reported(sblas):
    lim = sblas.spgemm_limits()
    assert lim["s_max"] >= 64 and lim["s_max"] % 32 == 0
    assert lim["acc_cap"] >= 64 and lim["chunk_cap"] >= 1
    assert sblas.lib().sblas_hip_spgemm_limits(None) == INVALID


def test_a_row_goes_general_exactly_when_span_flag_or_b_say_so(sblas):
    s_max = sblas.spgemm_limits()["s_max"]
    products = np.array([5, 5, 5, 0, 5], np.int64)
    span = np.array([1, s_max, s_max + 1, 0, 17], np.int64)
    path, cf = sblas.spgemm_classify(products, span)
    assert path.tolist() == [ROW, ROW, GENERAL, EMPTY, ROW]
    assert cf.tolist() == [0, 1]
    path, cf = sblas.spgemm_classify(products, span, b_ascending=False)
    assert path.tolist() == [GENERAL, GENERAL, GENERAL, EMPTY, GENERAL]
    chunks_ok(path, products, cf, sblas.spgemm_limits()["chunk_cap"])
    path, cf = sblas.spgemm_classify(products, span, general=True)
    assert path.tolist() == [GENERAL, GENERAL, GENERAL, EMPTY, GENERAL]
    assert cf.tolist() == [0, 4]                                            # 20 products: one chunk


def test_a_row_with_no_product_has_a_path_of_its_own(sblas):
    for kw in (dict(), dict(general=True), dict(b_ascending=False)):
        path, cf = sblas.spgemm_classify(np.zeros(4, np.int64), np.zeros(4, np.int64), **kw)
        assert path.tolist() == [EMPTY] * 4 and cf.tolist() == [0]


@pytest.mark.parametrize("cap", [1, 7, 50, 1000])
def test_chunks_cover_the_general_rows_once_and_respect_the_cap(sblas, cap):
    rng = np.random.default_rng(cap)
    products = rng.integers(0, 30, 200).astype(np.int64)
    products[17] = 400                                                      # above every cap but the last
    span = rng.integers(1, 100, 200).astype(np.int64)
    span[products == 0] = 0
    path, cf = sblas.spgemm_classify(products, span, general=True, chunk_cap=cap)
    assert np.array_equal(path == GENERAL, products > 0)
    chunks_ok(path, products, cf, cap)
    if cap == 1:
        assert len(cf) - 1 == int((products > 0).sum())                     # one chunk per non-empty general row
    # greedy: a chunk could not have taken the next row as well
    general = np.flatnonzero(path == GENERAL)
    for c in range(len(cf) - 2):
        rows = general[cf[c]:cf[c + 1]]
        assert int(products[rows].sum()) + int(products[general[cf[c + 1]]]) > cap


def test_a_row_of_more_than_2_31_products_does_not_overflow(sblas):
    big = (1 << 31) + 12345
    products = np.array([3, big, 4, big, big, 2], np.int64)
    span = np.full(6, 10, np.int64)
    path, cf = sblas.spgemm_classify(products, span, general=True, chunk_cap=(5 << 30))
    assert path.tolist() == [GENERAL] * 6
    chunks_ok(path, products, cf, 5 << 30)
    assert cf.tolist() == [0, 4, 6]                                         # 3 + big + 4 + big <= 5 * 2^30 < that + big
    path, cf = sblas.spgemm_classify(products, span, general=True, chunk_cap=10)
    assert cf.tolist() == [0, 1, 2, 3, 4, 5, 6]
    path, cf = sblas.spgemm_classify(products, span)                        # the row path takes any count
    assert path.tolist() == [ROW] * 6 and cf.tolist() == [0]


def test_no_rows_and_bad_arguments(sblas):
    path, cf = sblas.spgemm_classify(np.zeros(0, np.int64), np.zeros(0, np.int64))
    assert len(path) == 0 and cf.tolist() == [0]
    L = sblas.lib()
    p, s = np.array([1], np.int64), np.array([1], np.int64)
    path, cf, n = np.zeros(1, np.uint8), np.zeros(2, np.int64), C.c_int64()
    args = lambda **kw: [kw.get("m", 1), kw.get("p", p.ctypes.data), kw.get("s", s.ctypes.data), 1, kw.get("flags", 0),
                         kw.get("cap", 0), kw.get("path", path.ctypes.data), kw.get("cf", cf.ctypes.data), kw.get("n", C.byref(n))]
    assert L.sblas_hip_spgemm_classify(*args()) == 0
    for bad in (dict(m=-1), dict(p=None), dict(s=None), dict(path=None), dict(cf=None), dict(n=None), dict(flags=2), dict(cap=-1)):
        assert L.sblas_hip_spgemm_classify(*args(**bad)) == INVALID, bad
    neg = np.array([-1], np.int64)
    assert L.sblas_hip_spgemm_classify(*args(p=neg.ctypes.data)) == INVALID


def test_group_width_follows_the_mean_b_row_length_and_the_span(sblas):
    s_max = sblas.spgemm_limits()["s_max"]
    assert sblas.spgemm_group_width(products=5 * 16, a_len=5, span=100) == 16
    assert sblas.spgemm_group_width(products=5 * 16 + 1, a_len=5, span=100) == 64
    assert sblas.spgemm_group_width(products=5, a_len=5, span=s_max // 4) == 16
    assert sblas.spgemm_group_width(products=5, a_len=5, span=s_max // 4 + 1) == 64


def test_nnz_of_c_must_stay_below_2_31(sblas):
    # the bound check of create, on the host: 65536 dense rows times 32768 dense columns is exactly 2^31 entries
    assert sblas.spgemm_check_nnz(65536 * 32768 - 1) == 0
    assert sblas.spgemm_check_nnz(65536 * 32768) == INVALID
    assert sblas.spgemm_check_nnz(0) == 0 and sblas.spgemm_check_nnz(-1) == INVALID
