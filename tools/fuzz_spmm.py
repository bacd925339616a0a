"""Randomised differential test of SpMM and SpMV at the bar of the numerics judges (tests/numerics.py), one GPU.

  python tools/fuzz_spmm.py [--op spmm|spmm_typed|spmv|all] [--cases N] [--seed S] [--only K] [--max-rows R] [--cap C]

It follows tools/fuzz_plans.py, whose generator pieces (families, damage kinds, degenerate shapes, the planted row of
drawn_plant()) it imports, and adds tools/fuzz_parity.py's families that fuzz_plans lacks (scattered, queen_grid) and five
that give a kernel the panels it needs (wideband, dense_blocks, short_band, long_rows, mixed_band; HINTS).  Family,
degenerate shape, planted (limit, length) pair, entry point, order pair, type pair, SpMV selection and regime turn with
the case number (the families every 19 cases, SpMM's entry points every 11, the regimes every 3); everything else is
drawn.  Case k of operation op draws from
case_rng(seed, op, k); its parameters are printed when it fails (and with --only), so `--op X --seed S --only K` replays
it.  Exit status 1 on the first mismatch; nothing retries a failing case.

Operations:
  spmm        float64 / int32, the tuned kernels: spmm, SpmmPlan.spmm, a split SpmmPlan, spmm_ordered and
              SpmmPlan.spmm_ordered over the four (order_b, order_c) pairs, spmm_tensor on strided views with and
              without a plan, dense_to_rowmajor + spmm_rowmajorB
  spmm_typed  the three other (value, index) pairs through spmm_typed and spmm_ordered
  spmv        spmv under each of the twelve SBLAS_SPMV_VARIANTs, SpmvPlan, spmv_typed in the three other pairs

Every case draws a structure, a row block [a, b) of it (half the cases; re-based row pointers, C / y written at the block's
offset into the full-height array), leading dimensions with and without padding, a width, the switches SBLAS_SPMM_VARIANT,
SBLAS_STAGE_RANGE, SBLAS_SPMM_MIN_LDBT and SBLAS_SPMM_MAX_BT_BYTES, and a regime with the scalars the regime allows:

  grid       numerics.grid_problem in R1 / R2 / R3sub / R3over (test_gpu_numerics.grid_kwargs): == the integer result
  general    numerics.log_uniform data, non-dyadic alpha / beta, beta = 0 over a NaN-filled C inside the block:
             within numerics.bound of numerics.reference_dd
  nonfinite  the general problem with Inf / NaN planted in A, B / x or C / y: numerics.check_classes everywhere, the
             general bound on the untainted outputs

No tolerance is defined here.  Besides its regime every case checks that everything of C / y outside the block's rows and
columns -- other rows, the padding up to ldc -- keeps the bits it had, hands the workspace in filled with NaN bytes, and
(float64 / int32) holds the drawn entry point to the bits of the unplanned (COL, COL) call on the same operands, which
tests/test_gpu_order.py and the plan's contract promise; a split plan's rows and the caller-staged entry are summed in
their own order and go to the judges alone.

draw(op, ...) makes the problem on the host (and, from the host rule, what the call is going to launch); judge(P, ans)
raises AssertionError on an answer the references refuse; run_case() draws, computes on the device, judges and returns
what the case exercised.  tests/test_fuzz_spmm_host.py runs the host pieces without a GPU and shows that the judges
refuse spoiled answers; tests/test_gpu_fuzz_spmm.py runs run_case() and asserts a census of the returned dicts."""
import argparse
import contextlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "s-blas_amd", "python"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import sblas_amd as S
from sblas_amd import synth
import fuzz_plans as FP
from fuzz_plans import DAMAGE, DEGENERATE, RELATIONS, MIN_ROWS, need      # imported, not copied: the census reads them here
import numerics as N
import test_gpu_numerics as TG                           # grid_kwargs, R4_SCALARS, _scalars: the regimes' own definitions

OPS = ["spmm", "spmm_typed", "spmv"]
EXTRA_FAMILIES = ["scattered", "queen_grid", "wideband", "dense_blocks", "short_band", "long_rows", "mixed_band"]
FAMILIES = FP.FAMILIES + EXTRA_FAMILIES
WIDTHS = [1, 2, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 130, 256, 300]
SPMM_VARIANTS = ["auto", "dpp", "rows", "lanes", "merge", "mfma", "nomfma"]
SPMV_VARIANTS = ["plain", "lds", "lds2", "lds1s2", "lds1s3", "lds1s4", "seg2", "seg3", "seg4", "seg8", "stream", "auto"]
SWITCHES = ["SBLAS_SPMM_VARIANT", "SBLAS_STAGE_RANGE", "SBLAS_SPMM_MIN_LDBT", "SBLAS_SPMM_MAX_BT_BYTES", "SBLAS_SPMV_VARIANT"]
SPMM_ENTRIES = ["spmm", "plan", "split_plan", "ordered", "plan_ordered", "tensor", "tensor_plan", "rowmajorB"]
# case % 11 (no factor in common with the families' 19, the regimes' 3 or the orders' 4); the split plan comes twice, since
# it splits only where a long row meets a plan that is active and a panel the direct kernels own
SPMM_ENTRY_TURN = ["spmm", "plan", "split_plan", "ordered", "plan_ordered", "tensor", "split_plan", "tensor_plan", "rowmajorB", "plan", "ordered"]
TYPED_ENTRIES = ["typed", "ordered"]
SPMV_ENTRIES = ["variant", "plan", "typed"]
SPMV_ENTRY_TURN = ["variant", "plan", "typed", "plan"]    # case % 4; the variant itself turns with case // 4
COL, ROW = S.COL_MAJOR, S.ROW_MAJOR
ORDERS = [(COL, COL), (COL, ROW), (ROW, COL), (ROW, ROW)]
F64, F32, I32, I64 = np.float64, np.float32, np.int32, np.int64
TYPED = [(F32, I32), (F32, I64), (F64, I64)]
REGIMES = ["grid", "general", "nonfinite"]
GRID = TG.GRID
# the split SpmmPlan of a case: rows of SPLIT_MIN+ entries in pieces of PIECE (test_gpu_numerics' 500 / 128, a power of
# two here); the planted row of spmm / spmm_typed is drawn around SPLIT_MIN, so that "far" is a row of several pieces
SPLIT_MIN, PIECE = 512, 128
DPP_LONG = 4096                                           # kernels.h: entries from which the row-per-wave kernel sums a row on sixteen waves
STREAM_TIERS = (4096, 6144)                               # the two LDS capacities of the SpMV stream kernel (spmv_plan.cpp, spmv_kind)
# nnz * n of a case.  The judges cost in proportion to it (about 0.1 s per 10^6 for reference_dd): a case's rows are drawn
# so that a family of TYPICAL_ROW entries a row stays near TYPICAL, and a width that still gives more than CAP is redrawn
# downward.  The families with a size of their own (queen_grid, dense_blocks, clique) reach CAP.
TYPICAL, CAP, TYPICAL_ROW = 1.0e6, 5.0e6, 12
QUEEN_BLOCK = (240, 301)                                  # rows of a queen_grid case's block (test_gpu_numerics takes 300)
SENTINEL = -7.25e300                                      # B's padding: finite, and ruinous to any sum it reaches
# what the directed families are for: the widths (and selections) at which the kernel they feed is chosen
HINTS = dict(queen_grid=dict(n=[128, 130, 256], variant=["auto", "nomfma", "auto", "merge"]),  # rows in groups of three: row merging
             dense_blocks=dict(n=[33, 64, 65, 128, 130], variant=["mfma", "auto", "mfma"]),    # 16 x 4 blocks: the matrix cores
             wideband=dict(n=[2, 8, 16, 32, 64, 65, 128], variant=["auto", "nomfma", "lanes"]),  # dense bands: the LDS-tiled kernels
             short_band=dict(n=[64, 128, 130, 256, 300], variant=["auto", "rows", "nomfma"]),  # short rows: four rows per wave
             long_rows=dict(n=[1, 2, 5, 8, 17, 64, 130], variant=["auto", "dpp", "nomfma"]),   # 520+ a row: a wave per row at n <= 8, split rows
             mixed_band=dict(n=[16, 32, 64, 65, 128, 256], variant=["auto", "nomfma", "mfma"]))  # LDS-tiled and direct panels in one call


def limits_of(op):
    if op == "spmv":
        return dict(spmv_split=S.SPMV_SPLIT_MIN, stream4096=STREAM_TIERS[0], stream6144=STREAM_TIERS[1])
    if op == "spmm":
        return dict(split=SPLIT_MIN, dpp_long=DPP_LONG)
    return dict(split=SPLIT_MIN)


# ---------------------------------------------------------------------------------------------------------------------
# structure (host only)
# ---------------------------------------------------------------------------------------------------------------------
def _extra_family(kind, rng, rows, max_rows):
    seed = int(rng.integers(1 << 30))
    if kind == "scattered":                               # fuzz_parity's: 20-30 clusters of three columns a row
        rows = max(rows, 64)
        rp, ci, _ = synth.queen_like(rows, seed=seed, half_band=int(rng.integers(50, max(51, rows))))
    elif kind == "queen_grid":                            # fuzz_parity's "grid": rows in groups of three with one pattern; the
        # shape of test_gpu_numerics' "queen", of which a case takes a block of QUEEN_BLOCK rows (draw()): whole, a matrix
        # small enough for the judges is one dense band, which the LDS-tiled kernel takes from the row-merging one
        rp, ci, _ = synth.queen_like_grid(int(rng.integers(2700, 3300)), seed=seed, half_band=int(rng.integers(400, 1200)))
    elif kind == "wideband":                              # fuzz_parity's banded: up to 200 a row, several panels of them
        rows = max(rows, 150)
        per = int(rng.integers(30, 200))
        rp, ci, _ = synth.banded(rows, per, int(rng.integers(per, 3 * per + 2)), seed=seed)
    elif kind == "dense_blocks":                          # test_gpu_numerics' "block": 16 x 4 sub-blocks at 85 % fill
        rows = int(rng.integers(64, 330))
        rp, ci, _ = synth.block_structured(rows, nnz_per_row=int(rng.integers(48, 100)), half_band=int(rng.integers(100, 300)),
                                           fill=float(rng.uniform(0.7, 0.95)), seed=seed)
    elif kind == "short_band":                            # two to seven a row over a wide band
        rows = max(rows, 100)
        per = int(rng.integers(2, 8))
        rp, ci, _ = synth.banded(rows, per, int(rng.integers(per, 40 * per + 2)), seed=seed)
    elif kind == "long_rows":                             # a few rows of 520 to 700 scattered entries (260+ a row whatever the damage)
        rows, cols = int(rng.integers(8, 41)), int(rng.integers(1500, 4000))
        rp = np.concatenate([[0], np.cumsum(rng.integers(520, 701, rows))])
        ci = np.concatenate([np.sort(rng.choice(cols, int(c), replace=False)) for c in np.diff(rp)])
        return rows, cols, np.asarray(rp, np.int64), np.asarray(ci, np.int64)
    elif kind == "mixed_band":                            # runs of short rows between runs of long ones
        rows = max(rows, 128)
        long = int(rng.integers(40, 150))
        rp, ci, _ = synth.mixed_banded(rows, short=int(rng.integers(3, 9)), long=long, half_band=int(rng.integers(long, 3 * long)),
                                       interleave=int(rng.choice([0, 16, 48])), seed=seed)
    else:
        raise KeyError(kind)
    rows = len(rp) - 1
    return rows, rows, np.asarray(rp, np.int64), np.asarray(ci, np.int64)


def structure(rng, max_rows, limits, case):
    """fuzz_plans.structure() over FAMILIES (its own and EXTRA_FAMILIES), rectangular where the family allows it; the
    planted row is put in here: row `planted_row` holds exactly plant["L"] entries (columns drawn with repetition, sorted
    in half the cases)."""
    if max_rows < MIN_ROWS:
        raise ValueError("max_rows is %d: the families need at least %d rows" % (max_rows, MIN_ROWS))
    k = case
    degenerate = DEGENERATE[(k // 7) % len(DEGENERATE)] if k % 7 == 3 else None
    family = None if degenerate else FAMILIES[k % len(FAMILIES)]
    damage = str(rng.choice(DAMAGE))
    if family == "queen_grid" and rng.random() < 0.75:    # the groups of three equal rows are what this family is for
        damage = "none"
    if degenerate:
        rows, cols, rp, ci = FP._degenerate(degenerate, rng, max_rows, False)
    else:
        for attempt in range(FP.FAMILY_DRAWS):
            try:
                want = int(rng.integers(MIN_ROWS, max_rows + 1))
                if family in EXTRA_FAMILIES:
                    rows, cols, rp, ci = _extra_family(family, rng, want, max_rows)
                else:
                    rows, cols, rp, ci = FP._family(family, rng, want, max_rows, False)
                break
            except (ValueError, IndexError, ZeroDivisionError):           # a parameter draw the generator refuses
                if attempt == FP.FAMILY_DRAWS - 1:
                    raise
    rp, ci = FP._damage(damage, rng, rows, np.asarray(rp, np.int64), np.asarray(ci, np.int64))
    plant, planted_row = None, None
    if limits and not degenerate and k % 5 != 4 and rows and cols:
        plant = FP.drawn_plant(limits, k)
        planted_row = int(rng.integers(rows))
        new = rng.integers(0, cols, plant["L"])
        if rng.random() < 0.5:
            new = np.sort(new)
        rp, ci = FP.replace_row(rp, ci, planted_row, new)
    return dict(rows=rows, cols=cols, rp=rp, ci=ci, family=family, damage=damage, degenerate=degenerate, plant=plant,
                planted_row=planted_row)


# ---------------------------------------------------------------------------------------------------------------------
# switches: set for the time of one case, unset again on every path
# ---------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def switched(env):
    """the SBLAS_* switches of `env` set and read by the library; on leaving, every switch of SWITCHES is unset again
    and the library told so"""
    try:
        for name in SWITCHES:
            os.environ.pop(name, None)
        for name, value in env.items():
            assert name in SWITCHES, name
            os.environ[name] = str(value)
        S.reload_env()
        yield
    finally:
        for name in SWITCHES:
            os.environ.pop(name, None)
        S.reload_env()


def staged_widths(m, cols, nnz, n):
    """(chunk width, [staged width of every column chunk]) of an n-column call under the switches now set, from the
    library's own answers: the workspace holds (cols + 1) x ldbt doubles of the first chunk in front of a tail that does
    not depend on n, and n = 1 is staged 8 wide"""
    ldbt = lambda w: int(S.lib().sblas_hip_spmm_ldbt(w))
    first = (S.spmm_workspace_bytes(m, cols, nnz, n) - S.spmm_workspace_bytes(m, cols, nnz, 1)) // (8 * (cols + 1)) + 8
    if first >= ldbt(n):
        return n, [ldbt(n)]
    assert first >= 128 and first % 128 == 0, (first, n)                  # (the tool draws no limit below 128 columns)
    return first, [ldbt(min(first, n - j0)) for j0 in range(0, n, first)]


def host_rule(P):
    """what the host rule says the call launches, one dict per column chunk (no device: a plan is taken to own every
    panel with the direct kernels, and a split plan to cut what spmm_split_classify cuts then)"""
    m, cols, nnz, n = P["m"], P["cols"], P["nnz"], P["n"]
    if m == 0 or nnz == 0:
        return dict(chunks=0, ldbt=[], rules=[], split_rows=0, most_pieces=0)
    if P["entry"] == "rowmajorB":
        w, widths = n, [int(S.lib().sblas_hip_spmm_ldbt(n))]
    else:
        w, widths = staged_widths(m, cols, nnz, n)
    rules = [S.spmm_rule(m, cols, nnz, ldbt, min(w, n - j * w), caller_staged=P["entry"] == "rowmajorB") for j, ldbt in enumerate(widths)]
    pieces, srows = S.spmm_split_classify(P["sub_rp"], nnz, SPLIT_MIN, PIECE)
    out = dict(chunks=len(widths), ldbt=widths, rules=rules, split_rows=len(srows), most_pieces=int(srows[:, 2].max()) if len(srows) else 0)
    if P["entry"] == "split_plan" and rules[0]["plannable"] and len(srows):
        r = rules[0]
        plan = dict(n_direct=r["panels"], n_split=len(srows), panel_rows=max(r["panel_rows"], 1), groups=r["groups"])
        out["split_rule"] = S.spmm_rule(m, cols, nnz, widths[0], min(w, n), plan=plan)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# values: the regimes of test_gpu_numerics.py on the block's structure
# ---------------------------------------------------------------------------------------------------------------------
def plant_nonfinite(P, rng, where):
    """Inf / NaN `where` ("A", "B" or "C"), as test_gpu_numerics.nonfinite() places them"""
    rp, ci, m, k, n = P["sub_rp"], P["sub_ci"], P["m"], P["cols"], P["n"]
    A, B, C = P["A"].copy(), P["B"].copy(), P["C"].copy()
    lens = np.diff(rp)
    if where == "A":                # the first / last entry of isolated rows: their neighbours must stay finite
        rows = [r for r in range(1, m - 1, max(m // 7, 3)) if lens[r] > 0][:6] or [int(np.flatnonzero(lens)[0])]
        for q, r in enumerate(rows):
            A[rp[r] if q % 2 else rp[r + 1] - 1] = (np.inf, -np.inf, np.nan)[q % 3]
    elif where == "B":              # row 0, the last row, referenced rows and (where there is one) an unreferenced row
        used = np.zeros(k, bool)
        used[ci] = True
        rows = [0, k - 1] + list(rng.choice(np.flatnonzero(used), 3)) + list(np.flatnonzero(~used)[:2])
        for q, r in enumerate(rows):
            B[r, q % n] = (np.inf, np.nan, -np.inf)[q % 3]
        if n > 1:
            B[ci[0], n - 1] = np.inf           # a column where the rest of B is finite
    else:
        for q in range(5):
            C[rng.integers(0, m), rng.integers(0, n)] = (np.inf, -np.inf, np.nan)[q % 3]
    return A, B, C


def draw_values(P, rng, case):
    """A, B (cols x n) and C (m x n) of the block in the value type, the scalars, and the regime's reference"""
    rp, ci, m, k, n, vt = P["sub_rp"], P["sub_ci"], P["m"], P["cols"], P["n"], P["vt"]
    regime = P["regime"]
    if regime == "grid":
        g = N.grid_problem(rp, ci, k, n, dtype=vt, seed=int(rng.integers(1 << 30)), **TG.grid_kwargs(P["grid"], vt, case))
        P.update(A=g.A, B=g.B, C=g.C, alpha=g.alpha, beta=g.beta, expected=g.expected)
        return
    where = None
    if regime == "nonfinite":
        where = "C" if P["nnz"] == 0 else str(rng.choice(["A", "B", "C"]))
    alpha, beta = TG.R4_SCALARS[int(rng.integers(1, 3)) if where == "C" else int(rng.integers(3))]
    A = N.log_uniform(rng, len(ci), 60, vt)
    B = N.log_uniform(rng, (k, n), 20, vt)
    C = N.log_uniform(rng, (m, n), 60, vt) if beta else np.full((m, n), np.nan, vt)
    P.update(A=A, B=B, C=C, alpha=alpha, beta=beta, where=where)
    scal = TG._scalars(alpha, beta, vt)                 # the typed fp32 entry points take alpha / beta in the value type
    P["ref"] = N.reference_dd(rp, ci, A, B, C, *scal)
    P["bnd"] = N.bound(rp, ci, A, B, C, *scal, vt)
    if where:
        A, B, C = plant_nonfinite(P, rng, where)
        P.update(A=A, B=B, C=C, mask=N.finite_mask_inputs(rp, ci, A, B, C, beta))


# ---------------------------------------------------------------------------------------------------------------------
# layout: the flat buffers the entry points take
# ---------------------------------------------------------------------------------------------------------------------
def block_index(P):
    """flat positions of the block's (m x n) outputs in the C / y buffer"""
    (a, b), n, ldc = P["block"], P["n"], P["ldc"]
    r, j = np.arange(a, b)[:, None], np.arange(n)[None, :]
    return (j * ldc + r) if P["orders"][1] == COL else (r * ldc + j)


def c_size(P):
    return P["ldc"] * (P["n"] if P["orders"][1] == COL else P["rows"])


def padding_index(P):
    """flat positions of C's padding: between the rows (COL) or the columns (ROW) and ldc"""
    n, ldc, M = P["n"], P["ldc"], P["rows"]
    if P["orders"][1] == COL:
        return (np.arange(n)[:, None] * ldc + np.arange(M, ldc)[None, :]).reshape(-1)
    return (np.arange(M)[:, None] * ldc + np.arange(n, ldc)[None, :]).reshape(-1)


def pack_b(P):
    k, n, ldb, vt = P["cols"], P["n"], P["ldb"], P["vt"]
    if P["orders"][0] == COL:
        buf = np.full(n * ldb, SENTINEL if vt == F64 else -3.0e38, vt)
        buf.reshape(n, ldb)[:, :k] = P["B"].T
    else:
        buf = np.full(k * ldb, SENTINEL if vt == F64 else -3.0e38, vt)
        buf.reshape(k, ldb)[:, :n] = P["B"]
    return buf


def with_block(P, X):
    """the C / y buffer as handed in, with the block's outputs replaced by X (m x n)"""
    buf = P["cbuf"].copy()
    buf[block_index(P).reshape(-1)] = np.asarray(X, P["vt"]).reshape(-1)
    return buf


# ---------------------------------------------------------------------------------------------------------------------
# draw (host only)
# ---------------------------------------------------------------------------------------------------------------------
def draw(op, case, rng, max_rows, cap=CAP):
    k = case
    if op == "spmm":
        entry, (vt, it) = SPMM_ENTRY_TURN[k % len(SPMM_ENTRY_TURN)], (F64, I32)
        orders = ORDERS[(k // len(SPMM_ENTRY_TURN)) % 4] if entry in ("split_plan", "ordered", "plan_ordered", "tensor", "tensor_plan") else (COL, COL)
    elif op == "spmm_typed":
        entry, (vt, it) = TYPED_ENTRIES[k % 2], TYPED[(k // 2) % 3]
        orders = ORDERS[(k // 2) % 4] if entry == "ordered" else (COL, COL)
    else:
        entry, orders = SPMV_ENTRY_TURN[k % 4], (COL, COL)
        vt, it = TYPED[(k // 4) % 3] if entry == "typed" else (F64, I32)
    family = None if k % 7 == 3 else FAMILIES[k % len(FAMILIES)]
    hint = HINTS.get(family) if op != "spmv" else None
    n = 1 if op == "spmv" else int(rng.choice(hint["n"] if hint else WIDTHS))
    rows_cap = max_rows if op == "spmv" else int(min(max_rows, max(3 * MIN_ROWS, TYPICAL * (cap / CAP) / (n * TYPICAL_ROW))))
    st = structure(rng, rows_cap, limits_of(op), case)
    rows, cols, rp, ci = st["rows"], st["cols"], st["rp"], st["ci"]
    if family == "queen_grid" and op != "spmv":          # always a block, of QUEEN_BLOCK rows, around the planted row
        m = int(rng.integers(*QUEEN_BLOCK))
        a = int(rng.integers(0, rows - m + 1))
        if st["planted_row"] is not None:
            a = int(np.clip(st["planted_row"] - int(rng.integers(m)), 0, rows - m))
        b = a + m
    elif rng.random() < 0.5 and rows > 2:                # a row block (method 2); it holds the planted row
        a = int(rng.integers(0, rows - 1))
        b = int(rng.integers(a + 1, rows + 1))
        if st["planted_row"] is not None:
            a, b = min(a, st["planted_row"]), max(b, st["planted_row"] + 1)
    else:
        a, b = 0, rows
    m = b - a
    sub_rp, sub_ci = rp[a:b + 1] - rp[a], ci[rp[a]:rp[b]]
    nnz = len(sub_ci)
    while op != "spmv" and nnz * n > cap and n > WIDTHS[0]:   # the width redrawn downward
        n = WIDTHS[WIDTHS.index(n) - 1]
    variant = str(rng.choice(hint["variant"])) if hint else str(rng.choice(SPMM_VARIANTS + ["auto", "auto"]))
    env = {}
    if op == "spmv":
        spmv_variant = SPMV_VARIANTS[(k // 4) % len(SPMV_VARIANTS)] if entry == "variant" else None
        if spmv_variant:
            env["SBLAS_SPMV_VARIANT"] = spmv_variant
    else:
        if variant != "auto":
            env["SBLAS_SPMM_VARIANT"] = variant
        stage_range = str(rng.choice(["", "", "0", "1"]))
        if stage_range:
            env["SBLAS_STAGE_RANGE"] = stage_range
        if rng.random() < 0.3:
            env["SBLAS_SPMM_MIN_LDBT"] = "64"
        limit = 8 * (cols + 1) * 128 + 8                  # just above a 128-column copy: 256 and 300 columns take 2 and 3 chunks
        if n >= 256 and entry != "rowmajorB" and limit >= 4096 and rng.random() < 0.5:
            env["SBLAS_SPMM_MAX_BT_BYTES"] = limit
    pad_b, pad_c = int(rng.choice([0, 3])), int(rng.choice([0, 5]))
    ldb = (cols if orders[0] == COL else n) + pad_b
    ldc = (rows if orders[1] == COL else n) + pad_c
    if op == "spmv":
        pad_b = pad_c = 0
        ldb, ldc = cols, rows
    regime = REGIMES[k % 3]
    P = dict(op=op, case=case, st=st, rows=rows, cols=cols, block=(a, b), m=m, sub_rp=sub_rp, sub_ci=sub_ci, nnz=nnz, n=n,
             vt=vt, it=it, entry=entry, orders=orders, ldb=ldb, ldc=ldc, pad_b=pad_b, pad_c=pad_c, env=env,
             regime="general" if regime == "nonfinite" and m == 0 else regime, grid=GRID[(k // 3) % 4] if regime == "grid" else None)
    draw_values(P, rng, case)
    # the C / y buffer: other rows and the padding hold drawn values, the block C (NaN where beta = 0)
    P["cbuf"] = rng.standard_normal(c_size(P)).astype(vt)
    P["cbuf"] = with_block(P, P["C"])
    with switched(env):
        P["host"] = host_rule(P) if op == "spmm" else None
    P["params"] = FP.params_of(op, case, st, block=(a, b), nnz=nnz, n=n, vt=np.dtype(vt).name, it=np.dtype(it).name, entry=entry,
                               orders=orders, ldb=ldb, ldc=ldc, regime=P["regime"], grid=P["grid"], where=P.get("where"),
                               alpha=P["alpha"], beta=P["beta"], env=env)
    return P


def census_of(P, **more):
    st, host = P["st"], P["host"]
    lens = np.diff(P["sub_rp"])
    out = FP.census_of(st, rect=st["cols"] != st["rows"], block=P["block"] != (0, st["rows"]), pad_b=P["pad_b"] > 0, pad_c=P["pad_c"] > 0,
                       beta0=P["beta"] == 0, regime=P["grid"] or P["regime"], where=P.get("where"), entry=P["entry"], orders=P["orders"],
                       types=(np.dtype(P["vt"]).name, np.dtype(P["it"]).name), n=P["n"], env=dict(P["env"]),
                       longest=int(lens.max()) if len(lens) else 0)
    if host is not None:
        fired = set()
        for r in host["rules"]:
            fired |= {name for name in ("tiled", "mfma", "four_rows", "merge", "dpp_groups", "narrow", "rows8") if r[name]}
        if host.get("split_rule", {}).get("skip") and host["split_rule"]["split_groups"] > 0:
            fired.add("skip")
        out.update(rule=fired, ldbt=set(host["ldbt"]), chunks=host["chunks"], split_rows=host["split_rows"], most_pieces=host["most_pieces"])
    elif P["op"] == "spmv":
        items = S.spmv_plan_classify(P["sub_rp"]) if P["m"] else np.zeros((0, 4), np.int32)
        kinds = set(int(v) for v in items[:, 2])
        out.update(kinds=kinds, split_pieces=int(items[items[:, 2] == S.SPMV_ITEM_SPLIT, 3].max()) if S.SPMV_ITEM_SPLIT in kinds else 0)
    out.update(more)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the judge (host only)
# ---------------------------------------------------------------------------------------------------------------------
def same_bits(got, want):
    """bit for bit, a NaN for a NaN (which NaN an operation makes is the adder's choice)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan)) and got[~nan].tobytes() == want[~nan].tobytes()


def judge(P, ans):
    """ans: buf, the whole C / y buffer after the call; twin (optional), the same after the call it must equal"""
    vt, m, n = P["vt"], P["m"], P["n"]
    buf = np.asarray(ans["buf"])
    need(buf.dtype == np.dtype(vt) and buf.shape == P["cbuf"].shape, P, "the output buffer", buf.dtype, buf.shape)
    idx = block_index(P)
    outside = np.ones(buf.shape, bool)
    outside[idx.reshape(-1)] = False
    need(same_bits(buf[outside], P["cbuf"][outside]), P, "outside the block", "%d values changed" % int(
        ((buf[outside] != P["cbuf"][outside]) & ~(np.isnan(buf[outside]) & np.isnan(P["cbuf"][outside]))).sum()))
    got = buf[idx.reshape(-1)].reshape(m, n)
    rp, ci = P["sub_rp"], P["sub_ci"]
    if P["regime"] == "grid":
        bad = ~(got == P["expected"])
        if bad.any():
            r, c = np.argwhere(bad)[0]
            need(False, P, "grid", "%d of %d outputs differ from the exact result; first (row %d, col %d): got %r, want %r" % (
                bad.sum(), bad.size, r, c, got[r, c], P["expected"][r, c]))
    else:
        mask = P.get("mask")
        if P["regime"] == "nonfinite":
            ok, msg = N.check_classes(got, rp, ci, P["A"], P["B"], P["C"], *TG._scalars(P["alpha"], P["beta"], vt))
            need(ok, P, "classes", msg)
        res = N.check_bound(np.where(mask, got, 0.0) if mask is not None else got, P["ref"], P["bnd"], mask)
        need(res, P, "bound", res)
    if ans.get("twin") is not None:
        twin = np.asarray(ans["twin"]).reshape(m, n)
        need(same_bits(got, twin), P, "the unplanned (COL, COL) call's bits", "%d outputs differ" % int(
            ((got != twin) & ~(np.isnan(got) & np.isnan(twin))).sum()))


def reference_answer(P):
    """the references' own answer in the value type (what the host test feeds the judge)"""
    vt, rp, ci = P["vt"], P["sub_rp"], P["sub_ci"]
    if P["regime"] == "grid":
        return with_block(P, P["expected"])
    hi, lo = P["ref"]
    X = (hi + lo).astype(vt)
    if P["regime"] == "nonfinite":                        # a plain loop over the tainted data: its classes are IEEE's
        a, b = TG._scalars(P["alpha"], P["beta"], vt)
        with np.errstate(invalid="ignore", over="ignore"):
            loop = a * N.row_sums(rp, P["A"].astype(F64)[:, None] * P["B"].astype(F64)[ci])
            if b:
                loop = loop + b * P["C"].astype(F64)
        X = np.where(P["mask"], X, loop.astype(vt))
    return with_block(P, X)


# ---------------------------------------------------------------------------------------------------------------------
# the device
# ---------------------------------------------------------------------------------------------------------------------
def up(dev, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def nan_workspace(dev, nbytes):
    import torch
    return torch.full(((nbytes + 15) // 8 * 8,), 0xFF, dtype=torch.uint8, device=dev)


def tensor_views(P, dB, dC):
    (a, b), n, k, M, ldb, ldc = P["block"], P["n"], P["cols"], P["rows"], P["ldb"], P["ldc"]
    Bt = dB.view(n, ldb)[:, :k].t() if P["orders"][0] == COL else dB.view(k, ldb)[:, :n]
    Ct = dC.view(n, ldc)[:, a:b].t() if P["orders"][1] == COL else dC.view(M, ldc)[a:b, :n]
    return Bt, Ct


def run_spmm(P, dev):
    import torch
    m, k, n, nnz, entry, (ob, oc) = P["m"], P["cols"], P["n"], P["nnz"], P["entry"], P["orders"]
    (a, b), ldb, ldc, alpha, beta = P["block"], P["ldb"], P["ldc"], P["alpha"], P["beta"]
    f64 = P["op"] == "spmm"
    drp, dci, dv = up(dev, P["sub_rp"].astype(P["it"])), up(dev, P["sub_ci"].astype(P["it"])), up(dev, P["A"])
    dB, dC = up(dev, pack_b(P)), up(dev, P["cbuf"])
    c_off = a if oc == COL else a * ldc
    nbytes = S.spmm_workspace_bytes(m, k, nnz, n) if f64 else S.spmm_typed_workspace_bytes(dv.dtype, drp.dtype, m, k, nnz, n)
    ws8 = nan_workspace(dev, nbytes)
    ws = ws8.view(torch.float64) if f64 else ws8
    seen, plan, split, twin = {}, None, None, None
    try:
        if f64:
            plan = S.SpmmPlan(m, k, drp, dci, n)
            split = S.SpmmPlan(m, k, drp, dci, n, split=True, split_min=SPLIT_MIN, piece=PIECE)
            seen.update(plan=plan.info(), split=split.split_info())
            S.panel_census()
        if entry == "spmm":
            S.spmm(m, k, drp, dci, dv, dB, ldb, n, alpha, beta, dC, ldc, ws, c_offset=c_off)
        elif entry == "plan":
            plan.spmm(dv, dB, ldb, n, alpha, beta, dC, ldc, ws, c_offset=c_off)
        elif entry == "split_plan":
            split.spmm_ordered(dv, dB, ldb, ob, n, alpha, beta, dC, ldc, oc, ws, c_offset=c_off)
        elif entry == "ordered":
            S.spmm_ordered(m, k, drp, dci, dv, dB, ldb, ob, n, alpha, beta, dC, ldc, oc, ws, c_offset=c_off)
        elif entry == "plan_ordered":
            plan.spmm_ordered(dv, dB, ldb, ob, n, alpha, beta, dC, ldc, oc, ws, c_offset=c_off)
        elif entry in ("tensor", "tensor_plan"):
            Bt, Ct = tensor_views(P, dB, dC)
            S.spmm_tensor((m, k, drp, dci, dv), Bt, Ct, alpha, beta, workspace=ws, plan=plan if entry == "tensor_plan" else None)
        elif entry == "rowmajorB":
            S.dense_to_rowmajor(k, n, dB, ldb, ws)
            S.spmm_rowmajorB(m, k, drp, dci, dv, ws, n, alpha, beta, dC, ldc, c_offset=c_off)
        elif entry == "typed":
            S.spmm_typed(m, k, drp, dci, dv, dB, ldb, n, alpha, beta, dC, ldc, ws, c_offset=c_off)
        else:
            raise KeyError(entry)
        torch.cuda.synchronize()
        if f64:
            seen["panels"] = S.panel_census()
        buf = dC.cpu().numpy()
        if f64 and entry not in ("split_plan", "rowmajorB"):
            # the unplanned (COL, COL) call on the same operands, packed -- for the unplanned call itself the planned one:
            # the same bits
            dB2, dC2 = up(dev, np.ascontiguousarray(P["B"].T).reshape(-1)), up(dev, np.ascontiguousarray(P["C"].T).reshape(-1))
            ws8.fill_(0xFF)
            if entry == "spmm":
                plan.spmm(dv, dB2, k, n, alpha, beta, dC2, max(m, 1), ws)
            else:
                S.spmm(m, k, drp, dci, dv, dB2, k, n, alpha, beta, dC2, max(m, 1), ws)
            torch.cuda.synchronize()
            twin = dC2.cpu().numpy().reshape(n, m).T
    finally:
        for p in (plan, split):
            if p is not None:
                p.destroy()
    return dict(buf=buf, twin=twin), seen


def run_spmv(P, dev):
    import torch
    m, k, nnz, entry, (a, b) = P["m"], P["cols"], P["nnz"], P["entry"], P["block"]
    drp, dci, dv = up(dev, P["sub_rp"].astype(P["it"])), up(dev, P["sub_ci"].astype(P["it"])), up(dev, P["A"])
    dx, dy = up(dev, P["B"][:, 0]), up(dev, P["cbuf"])
    seen = {}
    if entry == "plan":
        plan = S.SpmvPlan(m, k, drp, dci)
        try:
            seen["plan"] = plan.info()
            plan(dv, dx, P["alpha"], P["beta"], dy, y_offset=a)
            torch.cuda.synchronize()
        finally:
            plan.destroy()
    elif entry == "typed":
        S.spmv_typed(m, k, drp, dci, dv, dx, P["alpha"], P["beta"], dy, y_offset=a)
    else:
        S.spmv(m, k, drp, dci, dv, dx, P["alpha"], P["beta"], dy, y_offset=a)
    torch.cuda.synchronize()
    return dict(buf=dy.cpu().numpy()), seen


DRAW = {op: (lambda case, rng, max_rows, cap=CAP, _op=op: draw(_op, case, rng, max_rows, cap)) for op in OPS}
JUDGE = {op: judge for op in OPS}
RUN = dict(spmm=run_spmm, spmm_typed=run_spmm, spmv=run_spmv)


def case_rng(seed, op, case):
    return np.random.default_rng([seed, OPS.index(op), case])


def run_case(op, case, seed, cuda, max_rows, cap=CAP):
    """case `case` of `op` on the device -> what it exercised; AssertionError (with the parameters) on a mismatch, and
    also when the library refuses a call of a generated case: every generated case is within the contracts"""
    P = DRAW[op](case, case_rng(seed, op, case), max_rows, cap)
    with switched(P["env"]):
        try:
            ans, seen = RUN[op](P, cuda)
        except S.SblasError as e:
            raise AssertionError("the library refused a call: %s %s" % (e, P["params"])) from e
    JUDGE[op](P, ans)
    return census_of(P, **seen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", default="all", choices=OPS + ["all"])
    ap.add_argument("--cases", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-rows", type=int, default=1500)
    ap.add_argument("--only", type=int, default=-1)
    ap.add_argument("--cap", type=float, default=CAP, help="nnz * n above which a case's width is redrawn downward")
    args = ap.parse_args()
    if args.max_rows < MIN_ROWS:
        ap.error("--max-rows must be at least %d" % MIN_ROWS)
    import torch
    dev = torch.device("cuda:0")
    for op in (OPS if args.op == "all" else [args.op]):
        for case in ([args.only] if args.only >= 0 else range(args.cases)):
            try:
                seen = run_case(op, case, args.seed, dev, args.max_rows, args.cap)
            except AssertionError as e:
                print("MISMATCH %s case %d: %s" % (op, case, e), flush=True)
                print("fuzz: FAILED (replay: --op %s --seed %d --max-rows %d --cap %g --only %d)" % (op, args.seed, args.max_rows, args.cap, case))
                return 1
            if args.only >= 0:
                print(DRAW[op](case, case_rng(args.seed, op, case), args.max_rows, args.cap)["params"])
                print("exercised:", seen)
        print("%s: all cases match their references" % op, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
