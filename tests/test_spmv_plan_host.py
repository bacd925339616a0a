"""The SpMV plan's host classifier (sblas_spmv_plan_classify): work items over the row pointers, no GPU needed."""
import numpy as np
import pytest

LPR, ST4096, ST6144, SEG, LDS2, LDS3, LDS4, LDS7, SPLIT = range(9)
BLOCK_ROWS = {LPR: 64, ST4096: 256, ST6144: 256, SEG: 16, LDS2: 8, LDS3: 8, LDS4: 8, LDS7: 8, SPLIT: 1}


def rowptr_of(lens):
    rp = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(np.asarray(lens, np.int64), out=rp[1:])
    return rp.astype(np.int32)


def check_cover(items, rows):
    """every row in exactly one item, items in row order, none longer than its kernel's block"""
    nxt = 0
    for r0, nr, kind, pieces in items:
        assert r0 == nxt and nr >= 1, (r0, nxt, nr)
        assert nr <= BLOCK_ROWS[int(kind)], (kind, nr)
        assert (pieces > 0) == (kind == SPLIT)
        nxt = r0 + nr
    assert nxt == rows


@pytest.mark.parametrize("length,kind", [(2, LPR), (7, ST4096), (48, ST6144), (73, SEG), (150, LDS3), (500, LDS7)])
def test_uniform_rows_get_the_unplanned_launchers_kernel(sblas, length, kind):
    """launch_spmv's picks for these averages: lanes-per-row (<= 2.5), stream with 4096 products (7 per row: one run
    either way) or 6144 (48 per row: two runs against three), segmented (64..96), LDS window with 3 / 7 slices"""
    rows = 5000
    items = sblas.spmv_plan_classify(rowptr_of([length] * rows))
    check_cover(items, rows)
    assert set(items[:, 2].tolist()) == {kind}
    # the items are the unplanned kernel's blocks: consecutive, aligned from row 0
    br = BLOCK_ROWS[kind]
    assert (items[:, 0] == np.arange(len(items)) * br).all()


def test_mixed_rows_get_per_item_classes(sblas):
    """two halves of 7 and 150 per row: one kernel for all of it today (average 78.5: segmented), one per half here"""
    rows = 4096
    items = sblas.spmv_plan_classify(rowptr_of([7] * (rows // 2) + [150] * (rows // 2)))
    check_cover(items, rows)
    first = items[items[:, 0] < rows // 2]
    second = items[items[:, 0] >= rows // 2]
    assert set(first[:, 2].tolist()) == {ST4096}
    assert set(second[:, 2].tolist()) == {LDS3}


def test_interleaved_rows_follow_their_tiles(sblas):
    rng = np.random.default_rng(3)
    lens = np.where((np.arange(9000) // 300) % 2 == 0, 7, 150) + rng.integers(-2, 3, 9000)
    items = sblas.spmv_plan_classify(rowptr_of(lens))
    check_cover(items, len(lens))
    kinds = set(items[:, 2].tolist())
    assert ST4096 in kinds and any(k in kinds for k in (LDS2, LDS3, LDS4, LDS7))


def test_tile_of_the_matrix_family_keeps_the_matrix_instantiation(sblas):
    """rows of 100..400 (LDS window throughout): one slice count, the one the matrix average asks for"""
    rng = np.random.default_rng(5)
    lens = rng.integers(100, 401, 6000)
    items = sblas.spmv_plan_classify(rowptr_of(lens))
    check_cover(items, len(lens))
    avg = lens.sum() / len(lens)
    want = LDS2 if avg <= 115 else LDS3 if avg <= 180 else LDS4 if avg <= 230 else LDS7
    assert set(items[:, 2].tolist()) == {want}


@pytest.mark.parametrize("length", [5001, 12289, 200000])
def test_long_row_becomes_a_split_item(sblas, length):
    lens = [3] * 1000
    lens[517] = length
    split_min, piece = (5000, 1024) if length == 5001 else (0, 0)
    items = sblas.spmv_plan_classify(rowptr_of(lens), split_min=split_min, piece=piece)
    check_cover(items, len(lens))
    sp = items[items[:, 2] == SPLIT]
    assert sp.shape[0] == 1 and sp[0, 0] == 517 and sp[0, 1] == 1
    p = piece or sblas.SPMV_SPLIT_PIECE
    assert sp[0, 3] == -(-length // p)


def test_row_at_the_threshold_is_not_split(sblas):
    lens = [3] * 300
    lens[10] = sblas.SPMV_SPLIT_MIN
    items = sblas.spmv_plan_classify(rowptr_of(lens))
    check_cover(items, len(lens))
    assert SPLIT not in items[:, 2]


def test_split_rows_leave_the_tile_class_to_the_other_rows(sblas):
    """a 10^6-entry row among rows of 3: the rows of 3 stay on the stream kernel (the long row does not drag the tile's
    average into another class)"""
    lens = [3] * 2000
    lens[700] = 1000000
    items = sblas.spmv_plan_classify(rowptr_of(lens))
    check_cover(items, len(lens))
    assert set(items[items[:, 2] != SPLIT][:, 2].tolist()) == {ST4096}


def test_empty_rows_and_empty_matrices(sblas):
    items = sblas.spmv_plan_classify(rowptr_of([0, 0, 5, 0, 9, 0] * 100))
    check_cover(items, 600)
    assert len(sblas.spmv_plan_classify(np.zeros(1, np.int32))) == 0            # rows = 0
    items = sblas.spmv_plan_classify(np.zeros(301, np.int32))                     # nnz = 0
    check_cover(items, 300)
    assert set(items[:, 2].tolist()) == {LPR}


def test_descending_row_pointers_are_refused(sblas):
    with pytest.raises(sblas.SblasError):
        sblas.spmv_plan_classify(np.array([0, 5, 3, 8], np.int32))


def test_random_structures_are_covered(sblas):
    from sblas_amd import synth
    for seed in range(4):
        rp, _, _ = synth.random_csr(3000 + 37 * seed, 500, 1 + 40 * seed, seed=seed, empty_every=7,
                                    long_row=(11 * seed, 30000))
        items = sblas.spmv_plan_classify(rp)
        check_cover(items, len(rp) - 1)
        sp = items[items[:, 2] == SPLIT]
        assert sp.shape[0] == 1 and sp[0, 0] == 11 * seed
