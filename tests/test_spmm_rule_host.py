"""The SpMM kernel rule (sblas_spmm_rule_describe, csrc/spmm_rule.cpp): what a column chunk stages, classifies and
launches in stage 2, for each row of DESIGN.md 3's selection table.  No GPU needed.

Every expected value is a known answer worked out by hand from the rule's definition, never by calling the rule.  The
panel geometry of the default shape (72 000 rows, 256 CUs) follows from cost = ceil(panels / 256) * (height + 40), times
20 / 23 for two / three groups per wave of the 64+-column kernel:
  64+ columns: two groups, 96 rows -> 750 panels, 3 rounds * 136 * 20 = 8160; three groups, 144 rows -> 500 panels,
      2 * 184 * 23 = 8464: two groups win;
  16 columns (one to three groups, no factor): 144 rows: 2 * 184 = 368 beats 96 rows (3 * 136 = 408) and 48 rows
      (1500 panels, 6 * 88 = 528): three groups; capped at two groups (32 columns, or two tile copies): 96 rows; capped at
      one group: 48 rows;
  8 columns: always one group of 48 rows (1500 panels)."""
import pytest

ROWS = 72000
ENV = ("SBLAS_SPMM_VARIANT", "SBLAS_TUNE", "SBLAS_DIRECT_LDS", "SBLAS_DIRECT_MERGE", "SBLAS_STAGE_RANGE", "SBLAS_DIRECT_MAP",
       "SBLAS_ROWS8_MIN_AVG", "SBLAS_WINDOW_DENSITY", "SBLAS_SPMM_PANEL_ROWS", "SBLAS_MFMA_MIN_FILL")

STAGE_CALLER, STAGE_FULL, STAGE_FUSED, STAGE_RANGE, STAGE_PLANNED = range(5)
VERDICTS_NONE, VERDICTS_STAGING, VERDICTS_SEPARATE, VERDICTS_EARLIER, VERDICTS_PLAN = range(5)
NONE, WINDOW6, LANES = range(3)


@pytest.fixture
def env(sblas, monkeypatch):
    """set(NAME=value, ...): the library's switches for one test (everything else at its default), restored afterwards"""
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    sblas.reload_env()

    def set_(**kw):
        for name, value in kw.items():
            monkeypatch.setenv(name, value)
        sblas.reload_env()
    yield set_
    monkeypatch.undo()
    sblas.reload_env()


def rule(sblas, ldbt, avg, n=None, cols=ROWS, **kw):
    return sblas.spmm_rule(ROWS, cols, int(avg * ROWS), ldbt, n=n, ncu=256, **kw)


def tiled(r):
    """the LDS-tiled launch: None, ("window6", G, NH, grid y) or ("lanes", NC, CP, G, LPE)"""
    if r["tiled"] == WINDOW6:
        assert (r["lanes_nc"], r["lanes_cp"], r["lanes_lpe"]) == (0, 0, 0)
        return ("window6", r["tiled_g"], r["w6_nh"], r["w6_grid_y"])
    if r["tiled"] == LANES:
        assert (r["w6_nh"], r["w6_grid_y"]) == (0, 0)
        return ("lanes", r["lanes_nc"], r["lanes_cp"], r["tiled_g"], r["lanes_lpe"])
    assert r["tiled"] == NONE and r["tiled_g"] == 0
    return None


def direct(r):
    """the direct launches in launch order: ("rows", waves, voted), "merge", ("dpp", GROUPS, pad), ("narrow", NC), "rows8" """
    out = []
    if r["four_rows"]:
        out.append(("rows", r["four_rows_waves"], r["four_rows_voted"]))
    else:
        assert (r["four_rows_waves"], r["four_rows_voted"]) == (0, 0)
    if r["merge"]:
        out.append("merge")
    if r["dpp_groups"]:
        out.append(("dpp", r["dpp_groups"], r["dpp_pad"]))
    if r["narrow"]:
        out.append(("narrow", r["narrow"]))
    if r["rows8"]:
        out.append("rows8")
    return out


def step(r):
    return (r["staging"], r["verdicts"], r["panel_rows"], r["groups"], r["panels"], r["plannable"])


CLASSIFIED_96 = (STAGE_FUSED, VERDICTS_STAGING, 96, 2, 750, 1)
UNCLASSIFIED = (STAGE_FULL, VERDICTS_NONE, 1, 2, 0, 0)

# (ldbt, nonzeros per row, cols) -> (step, LDS-tiled launch, matrix-core batch or 0, direct launches)
GEOMETRY = [
    # 64 columns: the row-length bar is 24, calls below three quarters of it (18) classify nothing; four rows per wave
    # below 56 per row, in workgroups of 4 waves below 8 per row
    (64, 400, ROWS, CLASSIFIED_96, ("window6", 2, 1, 1), 0, [("dpp", 2, 0)]),
    (64, 40, ROWS, CLASSIFIED_96, ("window6", 2, 1, 1), 0, [("rows", 16, 0)]),
    (64, 10, ROWS, UNCLASSIFIED, None, 0, [("rows", 16, 0)]),
    (64, 5, ROWS, UNCLASSIFIED, None, 0, [("rows", 4, 0)]),
    # 128+ columns: always classified, two halves per workgroup, matrix cores possible, the vote picks the direct kernel;
    # below 32 per row the four-rows kernel without a vote
    (128, 400, ROWS, CLASSIFIED_96, ("window6", 2, 2, 1), 2, [("rows", 16, 1), "merge", ("dpp", 1, 90000)]),
    (256, 20, ROWS, CLASSIFIED_96, ("window6", 2, 2, 2), 2, [("rows", 16, 0)]),
    # 8 columns: bar 56 (classified from 42 on), a wave per row from 256 per row on
    (8, 400, ROWS, (STAGE_FUSED, VERDICTS_STAGING, 48, 1, 1500, 1), ("lanes", 8, 1, 1, 1), 0, ["rows8"]),
    (8, 100, ROWS, (STAGE_FUSED, VERDICTS_STAGING, 48, 1, 1500, 1), ("lanes", 8, 1, 1, 1), 0, [("narrow", 8)]),
    (8, 10, ROWS, UNCLASSIFIED, None, 0, [("narrow", 8)]),
    # 16 columns: bar 20 (classified from 15 on), lane groups below 24 per row; three groups take two lanes per entry
    (16, 400, ROWS, (STAGE_FUSED, VERDICTS_STAGING, 144, 3, 500, 1), ("lanes", 16, 1, 3, 2), 0, [("dpp", 4, 0)]),
    (16, 18, ROWS, (STAGE_FUSED, VERDICTS_STAGING, 144, 3, 500, 1), ("lanes", 16, 1, 3, 2), 0, [("narrow", 16)]),
    (16, 10, ROWS, UNCLASSIFIED, None, 0, [("narrow", 16)]),
    # 32 columns: bar 16 (classified from 12 on), lane groups below 16 per row; two lanes per entry
    (32, 20, ROWS, CLASSIFIED_96, ("lanes", 32, 1, 2, 2), 0, [("dpp", 4, 0)]),
    (32, 10, ROWS, UNCLASSIFIED, None, 0, [("narrow", 32)]),
    # a staging copy of 20 000 001 x 32 doubles lies beyond 32-bit byte offsets: no classifier, no row-per-wave kernel
    (32, 400, 20000000, UNCLASSIFIED, None, 0, [("narrow", 32)]),
]


@pytest.mark.parametrize("ldbt,avg,cols,want_step,want_tiled,want_mfma,want_direct", GEOMETRY)
def test_width_row_length_and_geometry(sblas, env, ldbt, avg, cols, want_step, want_tiled, want_mfma, want_direct):
    r = rule(sblas, ldbt, avg, cols=cols)
    assert step(r) == want_step
    assert tiled(r) == want_tiled
    assert (r["mfma"], r["mfma_batch"], r["mfma_lds_floor"]) == (int(want_mfma > 0), want_mfma, 0)
    assert direct(r) == want_direct
    assert (r["interleave"], r["skip"], r["split_groups"]) == (-1, 0, 0)
    if r["dpp_groups"]:
        assert r["dpp_long"] == 4096


def test_describing_a_call_is_repeatable_and_reports_no_epoch(sblas, env):
    assert rule(sblas, 64, 400) == rule(sblas, 64, 400)
    assert "epoch" not in sblas.SPMM_RULE_FIELDS


def test_caller_staged_bt_gets_a_classifier_launch_of_its_own_and_no_plan(sblas, env):
    r = rule(sblas, 64, 400, caller_staged=True)
    assert step(r) == (STAGE_CALLER, VERDICTS_SEPARATE, 96, 2, 750, 0)
    assert tiled(r) == ("window6", 2, 1, 1) and direct(r) == [("dpp", 2, 0)]


def test_a_narrow_chunk_of_a_64_column_copy_sweeps_32_columns(sblas, env):
    """n <= 32 on the 64-column staging copy (SBLAS_SPMM_MIN_LDBT=64): the row-per-wave kernel with GROUPS 4, never four rows"""
    r = rule(sblas, 64, 10, n=32)
    assert step(r) == UNCLASSIFIED and direct(r) == [("dpp", 4, 0)]


def test_column_range_staging_of_a_row_block(sblas, env):
    """a block of 72 000 rows over 2 000 000 columns at 128 staged columns: (cols - 2 rows) * 128 * 16 bytes saved against
    8 bytes per nonzero + 40 MiB"""
    r = rule(sblas, 128, 400, cols=2000000)
    assert step(r) == (STAGE_RANGE, VERDICTS_STAGING, 96, 2, 750, 1)


# ---- SBLAS_SPMM_VARIANT -------------------------------------------------------------------------------------------

def test_variant_dpp_pins_the_row_per_wave_kernel(sblas, env):
    env(SBLAS_SPMM_VARIANT="dpp")
    r = rule(sblas, 64, 10)
    assert step(r) == UNCLASSIFIED and tiled(r) is None and direct(r) == [("dpp", 2, 0)]


def test_variant_rows_pins_the_four_rows_kernel(sblas, env):
    env(SBLAS_SPMM_VARIANT="rows")
    r = rule(sblas, 64, 400)
    assert step(r) == UNCLASSIFIED and tiled(r) is None and direct(r) == [("rows", 16, 0)]


def test_variant_merge_pins_the_row_merging_kernel(sblas, env):
    env(SBLAS_SPMM_VARIANT="merge")
    r = rule(sblas, 128, 400)
    assert step(r) == UNCLASSIFIED and tiled(r) is None and not r["mfma"] and direct(r) == ["merge"]


def test_variant_lanes_pins_the_lane_group_kernel(sblas, env):
    env(SBLAS_SPMM_VARIANT="lanes")
    r = rule(sblas, 8, 400)
    assert step(r) == UNCLASSIFIED and tiled(r) is None and direct(r) == [("narrow", 8)]


def test_variant_nomfma_never_launches_the_matrix_core_kernel(sblas, env):
    env(SBLAS_SPMM_VARIANT="nomfma")
    r = rule(sblas, 128, 400)
    assert step(r) == CLASSIFIED_96 and tiled(r) == ("window6", 2, 2, 1)
    assert (r["mfma"], r["mfma_batch"]) == (0, 0)
    assert direct(r) == [("rows", 16, 1), "merge", ("dpp", 1, 90000)]


def test_variant_mfma_classifies_64_columns_at_any_row_length(sblas, env):
    env(SBLAS_SPMM_VARIANT="mfma")
    r = rule(sblas, 64, 5)
    assert step(r) == CLASSIFIED_96 and r["groups"] <= 2
    assert tiled(r) == ("window6", 2, 1, 1)
    assert (r["mfma"], r["mfma_batch"]) == (1, 2)
    assert direct(r) == [("rows", 4, 0)]


def test_variant_mfma_keeps_two_groups_where_three_would_win(sblas, env):
    """36 000 rows on 256 CUs: 144-row panels of three groups (250 panels: one round, 184 * 23 = 4232) beat the best of two
    groups, 72 rows (500 panels: two rounds, 2 * 112 * 20 = 4480; 96 rows: 2 * 136 * 20), but the matrix-core kernel takes
    panels of up to 128 rows"""
    r = sblas.spmm_rule(36000, 36000, 36000 * 400, 64, ncu=256)
    assert (r["panel_rows"], r["groups"], r["panels"], tiled(r)) == (144, 3, 250, ("window6", 3, 1, 1))
    env(SBLAS_SPMM_VARIANT="mfma")
    r = sblas.spmm_rule(36000, 36000, 36000 * 400, 64, ncu=256)
    assert (r["panel_rows"], r["groups"], r["panels"], r["mfma"]) == (72, 2, 500, 1)


# ---- plans ---------------------------------------------------------------------------------------------------------

PLAN = dict(panel_rows=96, groups=2)
PLANNED = (STAGE_PLANNED, VERDICTS_PLAN, 96, 2, 750, 0)


def test_plan_without_lds_tiled_panels_skips_that_launch(sblas, env):
    r = rule(sblas, 64, 400, plan=dict(PLAN, n_direct=750))
    assert step(r) == PLANNED and tiled(r) is None and direct(r) == [("dpp", 2, 0)]
    r = rule(sblas, 128, 400, plan=dict(PLAN, n_direct=700, n_mfma_d=50))
    assert tiled(r) is None and r["mfma"] == 1


def test_plan_without_matrix_core_panels_skips_that_launch(sblas, env):
    r = rule(sblas, 128, 400, plan=dict(PLAN, n_window=700, n_direct=50))
    assert step(r) == PLANNED and tiled(r) == ("window6", 2, 2, 1) and (r["mfma"], r["mfma_batch"]) == (0, 0)
    assert direct(r) == [("dpp", 1, 90000)]


def test_plan_without_direct_panels_launches_no_direct_kernel(sblas, env):
    r = rule(sblas, 128, 400, plan=dict(PLAN, n_window=700, n_mfma_w=50))
    assert tiled(r) == ("window6", 2, 2, 1) and r["mfma"] == 1 and direct(r) == []
    r = rule(sblas, 8, 400, plan=dict(panel_rows=48, groups=1, n_window=1500))
    assert tiled(r) == ("lanes", 8, 1, 1, 1) and direct(r) == []


def test_plan_whose_vote_chose_the_row_merging_kernel(sblas, env):
    r = rule(sblas, 128, 400, plan=dict(PLAN, n_window=700, n_direct=50, merge=1))
    assert direct(r) == ["merge"]


def test_plan_whose_vote_chose_the_four_rows_kernel(sblas, env):
    r = rule(sblas, 256, 400, plan=dict(PLAN, n_window=700, n_direct=50, four_rows=1))
    assert direct(r) == [("rows", 16, 0)]


@pytest.mark.parametrize("ldbt,groups", [(256, 1), (128, 1), (64, 2), (32, 4), (8, 4)])
def test_split_plan_skips_the_split_rows_and_runs_the_split_kernels(sblas, env, ldbt, groups):
    plan = dict(PLAN, n_direct=750, n_split=3)
    r = rule(sblas, ldbt, 400, plan=plan)
    assert (r["skip"], r["split_groups"]) == (1, groups)
    r = rule(sblas, ldbt, 400, plan=dict(plan, n_split=0))
    assert (r["skip"], r["split_groups"]) == (0, 0)


# ---- SBLAS_TUNE ----------------------------------------------------------------------------------------------------

def test_tune_a_copies_of_a_bt_row_in_the_narrow_tile(sblas, env):
    env(SBLAS_TUNE="2,0,0,0")
    assert tiled(rule(sblas, 8, 400)) == ("lanes", 8, 2, 1, 1)
    r = rule(sblas, 16, 400)  # ... and at most two groups per wave at 16 columns: 96-row panels
    assert step(r) == CLASSIFIED_96 and tiled(r) == ("lanes", 16, 2, 2, 1)
    assert tiled(rule(sblas, 32, 20)) == ("lanes", 32, 1, 2, 2)
    env(SBLAS_TUNE="4:0:0:0")  # (colons are commas)
    assert tiled(rule(sblas, 8, 400)) == ("lanes", 8, 4, 1, 1)
    assert tiled(rule(sblas, 16, 400)) == ("lanes", 16, 1, 3, 2)  # four copies exist at 8 columns only
    env(SBLAS_TUNE="3,0,0,0")
    assert tiled(rule(sblas, 8, 400)) == ("lanes", 8, 1, 1, 1)


def test_tune_a_lds_floor_of_the_matrix_core_kernel(sblas, env):
    env(SBLAS_TUNE="100000")
    r = rule(sblas, 128, 400)
    assert (r["mfma"], r["mfma_lds_floor"]) == (1, 100000)
    assert tiled(rule(sblas, 8, 400)) == ("lanes", 8, 1, 1, 1)
    env(SBLAS_TUNE="163841")  # beyond 160 KiB: ignored
    assert rule(sblas, 128, 400)["mfma_lds_floor"] == 0


def test_tune_d_one_lane_per_entry_at_32_columns(sblas, env):
    env(SBLAS_TUNE="0,0,0,1")
    r = rule(sblas, 32, 20)
    assert step(r) == (STAGE_FUSED, VERDICTS_STAGING, 48, 1, 1500, 1)
    assert tiled(r) == ("lanes", 32, 1, 1, 1)
    assert direct(rule(sblas, 64, 40)) == [("rows", 16, 0)]


def test_tune_b_one_half_per_workgroup(sblas, env):
    env(SBLAS_TUNE="0,1,0,0")
    for ldbt in (128, 256):
        r = rule(sblas, ldbt, 400)
        assert step(r) == CLASSIFIED_96  # (three groups are allowed again; two still win on this shape)
        assert tiled(r) == ("window6", 2, 1, ldbt // 64)
        assert (r["mfma"], r["mfma_batch"]) == (1, 1)
    assert step(rule(sblas, 64, 22)) == CLASSIFIED_96  # 1 is no row-length bar


def test_tune_b_row_length_bar(sblas, env):
    assert step(rule(sblas, 64, 22)) == CLASSIFIED_96  # default bar 24: classified from 18 per row on
    env(SBLAS_TUNE="0,30,0,0")
    assert step(rule(sblas, 64, 22)) == UNCLASSIFIED  # bar 30: from 22.5 on
    assert step(rule(sblas, 64, 23)) == CLASSIFIED_96
    assert step(rule(sblas, 8, 23)) == (STAGE_FUSED, VERDICTS_STAGING, 48, 1, 1500, 1)  # (default bar 56)
    r = rule(sblas, 128, 400)  # and neither one half per workgroup nor another matrix-core batch
    assert tiled(r) == ("window6", 2, 2, 1) and r["mfma_batch"] == 2


def test_tune_b_matrix_core_batch_at_64_columns(sblas, env):
    for b, batch in ((3, 3), (4, 4), (5, 2)):
        env(SBLAS_TUNE="0,%d" % b, SBLAS_SPMM_VARIANT="mfma")
        assert (rule(sblas, 64, 400)["mfma"], rule(sblas, 64, 400)["mfma_batch"]) == (1, batch)
        assert rule(sblas, 128, 400)["mfma_batch"] == 2


def test_tune_c_long_row_threshold_of_the_row_per_wave_kernel(sblas, env):
    env(SBLAS_TUNE="0,0,5000,0")
    for ldbt, avg in ((16, 400), (32, 20), (64, 400), (128, 400)):
        assert rule(sblas, ldbt, avg)["dpp_long"] == 5000


def test_tune_d_waves_of_the_four_rows_kernel(sblas, env):
    env(SBLAS_TUNE="0,0,0,8")
    assert direct(rule(sblas, 64, 40)) == [("rows", 8, 0)]
    assert direct(rule(sblas, 64, 5)) == [("rows", 8, 0)]
    assert direct(rule(sblas, 128, 400))[0] == ("rows", 8, 1)
    assert tiled(rule(sblas, 32, 20)) == ("lanes", 32, 1, 2, 2)


# ---- the other switches the rule reads, and the export's argument checks ------------------------------------------------

def test_direct_kernel_switches(sblas, env):
    env(SBLAS_DIRECT_LDS="1024", SBLAS_DIRECT_MAP="interleave", SBLAS_DIRECT_MERGE="0", SBLAS_ROWS8_MIN_AVG="500")
    r = rule(sblas, 128, 400)
    assert direct(r) == [("rows", 16, 1), ("dpp", 1, 1024)] and r["interleave"] == 1
    assert direct(rule(sblas, 16, 400)) == [("dpp", 4, 0)]  # the 32-column sweep has no LDS pad
    assert direct(rule(sblas, 8, 400)) == [("narrow", 8)]


def test_bad_arguments_are_refused(sblas, env):
    L = sblas.lib()
    assert L.sblas_spmm_rule_describe(ROWS, ROWS, 100, 64, 64, 256, 0, None, None, 0) == len(sblas.SPMM_RULE_FIELDS)
    for bad in [(-1, ROWS, 100, 64, 64, 256), (ROWS, -1, 100, 64, 64, 256), (ROWS, ROWS, -1, 64, 64, 256),
                (ROWS, ROWS, 100, 48, 48, 256), (ROWS, ROWS, 100, 192, 192, 256), (ROWS, ROWS, 100, 64, 65, 256),
                (ROWS, ROWS, 100, 64, 0, 256), (ROWS, ROWS, 100, 64, 64, 0), (2 ** 31, ROWS, 100, 64, 64, 256)]:
        assert L.sblas_spmm_rule_describe(*bad, 0, None, None, 0) == -1, bad
    with pytest.raises(sblas.SblasError):
        rule(sblas, 64, 400, plan=dict(groups=2))  # a plan has a panel height
    with pytest.raises(sblas.SblasError):
        rule(sblas, 64, 400, plan=dict(PLAN, n_direct=-1))
