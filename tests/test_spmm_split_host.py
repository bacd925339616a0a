"""The split SpMM plan's host classifier (sblas_spmm_split_classify, csrc/spmm_split.cpp): no GPU needed."""
import numpy as np
import pytest


def rowptr_of(lens):
    rp = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    return rp.astype(np.int32)


def check_tiling(rp, pieces, srows, piece):
    """pieces tile every split row exactly, in CSR order, at most `piece` entries each; slots 0, 1, .. in order"""
    assert list(pieces[:, 3]) == list(range(len(pieces)))
    assert (srows[:, 3] == -1).all()
    for row, first, count, _ in srows:
        p = pieces[first:first + count]
        assert (p[:, 0] == row).all()
        assert p[0, 1] == rp[row] and p[-1, 2] == rp[row + 1]
        assert (p[1:, 1] == p[:-1, 2]).all()
        assert ((p[:, 2] - p[:, 1]) <= piece).all() and ((p[:, 2] - p[:, 1]) > 0).all()
    assert sum(int(c) for c in srows[:, 2]) == len(pieces)


def test_pieces_tile_each_split_row(sblas):
    lens = [5, 0, 40000, 3, 16384, 0, 99999, 7]
    rp = rowptr_of(lens)
    pieces, srows = sblas.spmm_split_classify(rp)
    assert list(srows[:, 0]) == [2, 4, 6]
    check_tiling(rp, pieces, srows, sblas.SPMM_SPLIT_PIECE)
    assert list(srows[:, 2]) == [10, 4, 25]
    pieces, srows = sblas.spmm_split_classify(rp, split_min=1000, piece=777)
    check_tiling(rp, pieces, srows, 777)
    assert list(srows[:, 0]) == [2, 4, 6]


def test_threshold_is_inclusive(sblas):
    rp = rowptr_of([4999, 5000, 5001, 0])
    _, srows = sblas.spmm_split_classify(rp, split_min=5000, piece=1000)
    assert list(srows[:, 0]) == [1, 2]
    rp = rowptr_of([sblas.SPMM_SPLIT_MIN - 1, sblas.SPMM_SPLIT_MIN])
    _, srows = sblas.spmm_split_classify(rp)
    assert list(srows[:, 0]) == [1]


def test_empty_rows_split_last_row_and_two_in_one_panel(sblas):
    lens = [0] * 10 + [20000, 0, 30000] + [0] * 5 + [17000]
    rp = rowptr_of(lens)
    pieces, srows = sblas.spmm_split_classify(rp, direct_mask=[1, 1, 1], panel_rows=8)
    assert list(srows[:, 0]) == [10, 12, 18]     # 10 and 12 share panel 1; 18 is the last row
    check_tiling(rp, pieces, srows, sblas.SPMM_SPLIT_PIECE)
    assert pieces[-1, 2] == rp[-1]
    empty = rowptr_of([0] * 7)
    pieces, srows = sblas.spmm_split_classify(empty)
    assert len(pieces) == 0 and len(srows) == 0


def test_masked_out_panels_are_never_split(sblas):
    rng = np.random.default_rng(1)
    lens = rng.integers(0, 40, 5000)
    lens[rng.choice(5000, 40, replace=False)] = rng.integers(16384, 50000, 40)
    rp = rowptr_of(lens)
    panel_rows = 96
    mask = rng.integers(0, 2, (5000 + panel_rows - 1) // panel_rows)
    pieces, srows = sblas.spmm_split_classify(rp, direct_mask=mask, panel_rows=panel_rows)
    expect = [r for r in range(5000) if lens[r] >= sblas.SPMM_SPLIT_MIN and mask[r // panel_rows]]
    assert list(srows[:, 0]) == expect and 0 < len(expect) < 40
    check_tiling(rp, pieces, srows, sblas.SPMM_SPLIT_PIECE)
    _, srows = sblas.spmm_split_classify(rp, direct_mask=np.zeros_like(mask), panel_rows=panel_rows)
    assert len(srows) == 0


def test_bad_input_is_refused(sblas):
    L = sblas.lib()
    rp = rowptr_of([3, 2])
    with pytest.raises(sblas.SblasError):
        sblas.spmm_split_classify(np.array([0, 5, 3], np.int32))          # descending
    with pytest.raises(sblas.SblasError):
        sblas.spmm_split_classify(rp, nnz=4)                               # rowptr[rows] > nnz
    assert L.sblas_spmm_split_classify(rp.ctypes.data, 2, 5, 0, 0, np.ones(1, np.uint8).ctypes.data, 0, None, 0) == -1
    # the wrapper checks what the C function cannot: one mask entry per panel
    rp = rowptr_of([1] * 100)
    with pytest.raises(sblas.SblasError):
        sblas.spmm_split_classify(rp, direct_mask=[1, 1, 1], panel_rows=32)
    with pytest.raises(sblas.SblasError):
        sblas.spmm_split_classify(rp, direct_mask=[1] * 4, panel_rows=0)
    assert len(sblas.spmm_split_classify(rp, direct_mask=[1] * 4, panel_rows=32)[1]) == 0
    # a short output buffer is filled as far as it goes; the count stays the whole answer
    rp = rowptr_of([20000])
    out = np.full((2, 4), 7, np.int32)
    assert L.sblas_spmm_split_classify(rp.ctypes.data, 1, 20000, 0, 0, None, 0, out.ctypes.data, 2) == 6
    assert list(out[1]) == [0, 4096, 8192, 1]
