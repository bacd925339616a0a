"""The lanes of a level plan without a GPU: sblas_sptrsv_pack -- the packer under the triangular solves' and ILU(0)'s
creates, with the neutral record (row, unit number) -- against the restatement in tests/sptrsv_numerics.py, and the layout
the kernels rely on checked directly: a row's units are consecutive and aligned to their count inside the level, pads
have row -1, rows ascend inside a level."""
import numpy as np
import pytest

import sptrsv_numerics as TN


def check_pack(S, n, rowptr, level, n_levels):
    lim = S.sptrsv_limits()
    g4, g16 = lim["g4_max"], lim["g16_max"]
    got = S.sptrsv_pack(n, rowptr, level, n_levels)
    want = TN.pack(n, rowptr, level, n_levels, g4, g16)
    for name, g, w in zip(("perm", "level_ptr", "level_unit_ptr", "unit_row", "unit_q"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), name
    perm, level_ptr, level_unit_ptr, unit_row, unit_q = got
    level = np.asarray(level, np.int64)
    length = np.diff(np.asarray(rowptr, np.int64))
    # the order
    assert np.array_equal(np.sort(perm), np.arange(n))
    assert np.array_equal(np.diff(level_ptr), TN.level_widths(level, n_levels))
    assert len(level_unit_ptr) == n_levels + 1 and level_unit_ptr[0] == 0 and level_unit_ptr[-1] == len(unit_row) == len(unit_q)
    assert np.all(np.diff(level_unit_ptr) >= 0)
    # the units, level by level
    for l in range(n_levels):
        rows, q = unit_row[level_unit_ptr[l]:level_unit_ptr[l + 1]], unit_q[level_unit_ptr[l]:level_unit_ptr[l + 1]]
        real = np.flatnonzero(rows >= 0)
        assert np.all(rows[rows < 0] == -1) and not q[rows < 0].any()
        per = np.array([TN.units_per_row(length[i], g4, g16) for i in rows[real]], np.int64)
        assert not ((real - q[real]) % per).any()                          # a row starts on a multiple of its unit count
        first = real[q[real] == 0]
        assert np.array_equal(rows[first], perm[level_ptr[l]:level_ptr[l + 1]])   # every row of the level once, in order
        assert np.all(np.diff(rows[first]) > 0)                                # ascending
        for u in first:                                                        # unit numbers 0 .. per_row - 1, consecutive
            k = TN.units_per_row(length[rows[u]], g4, g16)
            assert np.all(rows[u:u + k] == rows[u]) and np.array_equal(q[u:u + k], np.arange(k))
        assert len(real) == per[q[real] == 0].sum()
    return got


def test_trivial_sizes(sblas):
    got = check_pack(sblas, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), 0)
    assert [len(a) for a in got] == [0, 1, 1, 0, 0]
    got = check_pack(sblas, 1, np.array([0, 1], np.int32), np.zeros(1, np.int32), 1)
    assert got[3].tolist() == [0] and got[4].tolist() == [0] and got[2].tolist() == [0, 1]


def test_one_level_of_every_group_width(sblas):
    lim = sblas.sptrsv_limits()
    assert (lim["g4_max"], lim["g16_max"]) == (4, 32)                           # the lengths below sit on these boundaries
    lengths = [1, 40, 3, 20, 5, 33, 4, 32]
    rp = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    perm, level_ptr, level_unit_ptr, unit_row, unit_q = check_pack(sblas, 8, rp, np.zeros(8, np.int32), 1)
    # 1 | 15 pads | 16 | 1 | 3 pads | 4 | 4 | 4 pads | 16 | 1 | 3 pads | 4
    assert unit_row.tolist() == [0] + [-1] * 15 + [1] * 16 + [2] + [-1] * 3 + [3] * 4 + [4] * 4 + [-1] * 4 + [5] * 16 + [6] + [-1] * 3 + [7] * 4
    assert level_unit_ptr.tolist() == [0, 72]


def test_a_bidiagonal_chain_is_one_unit_a_level(sblas):
    rp, ci = TN.bidiagonal(10)
    lv, nl = sblas.sptrsv_levels(10, rp, ci)
    perm, level_ptr, level_unit_ptr, unit_row, unit_q = check_pack(sblas, 10, rp, lv, nl)
    assert nl == 10 and unit_row.tolist() == list(range(10)) and level_unit_ptr.tolist() == list(range(11))


def test_ash85_lower_triangle(sblas, ash85):
    n = ash85["m"]
    rp, ci = TN.triangle_of(n, ash85["rowptr"], ash85["colidx"], True)
    lv, nl = sblas.sptrsv_levels(n, rp, ci)
    got = check_pack(sblas, n, rp, lv, nl)
    assert nl > 1 and (got[3] < 0).any()                                        # several levels, and rows that needed pads


def test_a_level_wider_than_one_chain_pass(sblas):
    n = 300
    assert n > sblas.sptrsv_limits()["chain_threads"] // 4                     # units of one pass of the chain workgroup
    rp = (2 * np.arange(n + 1)).astype(np.int32)
    perm, level_ptr, level_unit_ptr, unit_row, unit_q = check_pack(sblas, n, rp, np.zeros(n, np.int32), 1)
    assert unit_row.tolist() == list(range(n)) and not unit_q.any()


def test_a_level_out_of_range_is_refused(sblas):
    rp = np.arange(4, dtype=np.int32)
    for level in ([0, 2, 1], [0, -1, 1]):
        with pytest.raises(sblas.SblasError):
            sblas.sptrsv_pack(3, rp, level, 2)
