"""Numerics of every kernel path against references the GPU code does not share (tests/numerics.py).

Regimes:
  R1  exact grid, rows of exactly cancelling pairs plus small terms       -> == the integer result
  R2  exact grid, >= 20 binades of products inside a row (fp64)           -> ==
  R3  exact grid at the subnormal scale (products k * 2^-1074 / 2^-149) and near overflow (~2^1000 / 2^120)  -> ==
  R4  signed data, log-uniform over 60 binades, non-dyadic alpha / beta (beta = 0 over a NaN-filled C)
      -> within gamma(L+2) (|alpha| sum|a b| + |beta c|) + (L+2) eta of the double-double reference
  R5  Inf / NaN in A (next to rows that must stay finite), in B / x (referenced and unreferenced rows, row 0, the last
      row) and in C / y under beta != 0 -> the predicted IEEE class everywhere, the R4 bound on the untainted outputs

R1-R3 rotate over the widths of each kernel selection, so every selection sees every grid regime on every matrix
family; R4 and R5 run every selection at one narrow (17) and one wide (128) width.  References are computed once per
problem and shared by the selections (module-level cache)."""
import numpy as np
import pytest

import numerics as N
from test_gpu_parity import SPMM_VARIANTS, _env_switch

pytestmark = pytest.mark.gpu

COL, ROW = 0, 1
F64, F32 = np.float64, np.float32
I32, I64 = np.int32, np.int64
SPMV_VARIANTS = ["plain", "lds", "lds2", "lds1s2", "lds1s3", "lds1s4", "seg2", "seg3", "seg4", "seg8", "stream", "auto"]
WIDTHS = [1, 3, 8, 16, 17, 32, 64, 65, 128, 256]
GRID = ["R1", "R2", "R3sub", "R3over"]
R4_SCALARS = [(0.1, 0.0), (-1 / 3, 0.3), (7.3e5, -2 / 7)]


@pytest.fixture(scope="module")
def env(sblas, cuda):
    import torch
    return sblas, torch, cuda


@pytest.fixture
def variant_env():
    yield from _env_switch("SBLAS_SPMM_VARIANT")


@pytest.fixture
def spmv_variant_env():
    yield from _env_switch("SBLAS_SPMV_VARIANT")


# ---------------------------------------------------------------------------------------------------------------------
# matrices: families that give each kernel real panels (a few thousand rows at most, except for split rows)
# ---------------------------------------------------------------------------------------------------------------------
_MATS = {}


def _from_lens(lens, cols, rng, sort=True):
    rp = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    ci = rng.integers(0, cols, int(rp[-1])).astype(np.int32)
    if sort:
        for r in np.flatnonzero(lens > 1):
            ci[rp[r]:rp[r + 1]].sort()
    return rp.astype(np.int32), ci


def matrix(name):
    """(rows, cols, rowptr int32, colidx int32)"""
    if name not in _MATS:
        from sblas_amd import synth
        rng = np.random.default_rng(17)
        if name == "banded":              # LDS-tiled panels (test_spmm_panel_census_paths_are_really_taken's band)
            rp, ci, _ = synth.banded(600, 60, 150)
            m = k = 600
        elif name == "wideband":          # the narrow LDS-tiled kernel's panels (test_narrow_banded_every_width_and_selection)
            rp, ci, _ = synth.banded(1100, 70, 330)
            m = k = 1100
        elif name == "block":             # dense 16 x 4 sub-blocks at 85 % fill: the matrix cores
            rp, ci, _ = synth.block_structured(320, nnz_per_row=96, half_band=200, fill=0.85)
            m = k = 320
        elif name == "queen":             # rows in groups of three with one pattern: the row-merging kernel (a row block)
            rp, ci, _ = synth.queen_like_grid(3000, half_band=400)
            k = len(rp) - 1
            a, b = 1200, 1500
            ci, rp, m = ci[rp[a]:rp[b]], (rp[a:b + 1] - rp[a]).astype(np.int32), b - a
        elif name == "powerlaw":          # short rows with very long ones: the whole workgroup / split rows
            rp, ci, _ = synth.powerlaw(1500, max_len=1500)
            lens = np.diff(rp.astype(np.int64))
            lens[[70, 71, 1499]] = (600, 1400, 700)
            rp, ci = _from_lens(lens, 1500, rng)
            m = k = 1500
        elif name == "longrows":          # rows of 30-50 scattered entries (direct panels) and three of 600+: split rows
            lens = rng.integers(30, 51, 800)
            lens[[70, 71, 799]] = (600, 1400, 700)
            rp, ci = _from_lens(lens, 20000, rng)
            m, k = 800, 20000
        elif name == "random":            # empty rows, unsorted rows, duplicates, a long row
            rp, ci, _ = synth.random_csr(400, 300, 9, seed=4, empty_every=11, long_row=(5, 333))
            ci = ci.copy()
            ci[rp[20]:rp[21]] = ci[rp[20]]                               # one row repeating a single column
            m, k = 400, 300
        elif name == "long":              # SpMV / A^T split rows: one row of 20 000 entries
            lens = rng.integers(2, 14, 3000)
            lens[7] = 20000
            rp, ci = _from_lens(lens, 25000, rng)
            m, k = 3000, 25000
        elif name == "tall":              # A^T split rows: one column of 17 000 entries
            m, k = 17000, 300
            lens = np.full(m, 3)
            rp, ci = _from_lens(lens, k, rng, sort=False)
            ci[rp[:-1]] = 5
        _MATS[name] = (m, k, np.asarray(rp, np.int32), np.asarray(ci, np.int32))
    return _MATS[name]


SPMM_FAMILIES = ["banded", "block", "queen", "powerlaw", "random"]


# ---------------------------------------------------------------------------------------------------------------------
# problems: values for one structure, and the expected result / reference
# ---------------------------------------------------------------------------------------------------------------------
class Problem:
    def __init__(self, rp, ci, k, A, B, C, alpha, beta, dtype, expected=None, ref=None, bnd=None, mask=None,
                 nonfinite=False):
        self.rp, self.ci, self.k = rp, ci, k
        self.m, self.n = len(rp) - 1, B.shape[1]
        self.A, self.B, self.C, self.alpha, self.beta, self.dtype = A, B, C, alpha, beta, np.dtype(dtype)
        self.expected, self.ref, self.bnd, self.mask, self.nonfinite = expected, ref, bnd, mask, nonfinite


_PROBLEMS = {}


def grid_kwargs(regime, dtype, which):
    f32 = np.dtype(dtype) == np.float32
    if regime == "R1":
        return dict(cancel=True)
    if regime == "R2":
        return dict(spread=6 if f32 else 24)
    scal = [(1.0, 0.0), (2.0, 1.0), (-1.0, 0.5), (4.0, -0.25)][which % 4]
    if regime == "R3sub":
        return dict(scale=-75, scale_b=-74, alpha=scal[0], beta=scal[1]) if f32 else \
            dict(scale=-537, alpha=scal[0], beta=scal[1])
    return dict(scale=50 if f32 else 480, alpha=[1.0, -0.5, 0.25, -1.0][which % 4], beta=scal[1])


def grid(key, rp, ci, k, n, regime, dtype, seed):
    key = ("grid", key, n, regime, np.dtype(dtype).str, seed)
    if key not in _PROBLEMS:
        g = N.grid_problem(rp, ci, k, n, dtype=dtype, seed=seed, **grid_kwargs(regime, dtype, seed))
        _PROBLEMS[key] = Problem(rp, ci, k, g.A, g.B, g.C, g.alpha, g.beta, dtype, expected=g.expected)
    return _PROBLEMS[key]


def general(key, rp, ci, k, n, alpha, beta, dtype, seed, ones=False):
    """R4: 60 binades in A and C, 20 in B (products over 80), signs random; beta = 0 over a NaN-filled C.
    ones: A = 1 (the merges and axpby, whose operands are the B rows themselves)."""
    key = ("general", key, n, alpha, beta, np.dtype(dtype).str, seed, ones)
    if key not in _PROBLEMS:
        rng = np.random.default_rng(seed)
        m = len(rp) - 1
        A = np.ones(len(ci), dtype) if ones else N.log_uniform(rng, len(ci), 60, dtype)
        B = N.log_uniform(rng, (k, n), 60 if ones else 20, dtype)
        C = N.log_uniform(rng, (m, n), 60, dtype) if beta else np.full((m, n), np.nan, dtype)
        ref = N.reference_dd(rp, ci, A, B, C, *_scalars(alpha, beta, dtype))
        bnd = N.bound(rp, ci, A, B, C, *_scalars(alpha, beta, dtype), dtype)
        _PROBLEMS[key] = Problem(rp, ci, k, A, B, C, alpha, beta, dtype, ref=ref, bnd=bnd)
    return _PROBLEMS[key]


def _scalars(alpha, beta, dtype):
    """the typed fp32 entry points take alpha / beta in the value type"""
    if np.dtype(dtype) == np.float32:
        return float(np.float32(alpha)), float(np.float32(beta))
    return alpha, beta


def nonfinite(key, rp, ci, k, n, alpha, beta, dtype, seed, where, ones=False):
    """R5: the R4 problem of the same key with Inf / NaN planted `where` ("A", "B" or "C")."""
    base = general(key, rp, ci, k, n, alpha, beta, dtype, seed, ones)
    A, B, C = base.A.copy(), base.B.copy(), base.C.copy()
    rng = np.random.default_rng(seed + 1)
    m = len(rp) - 1
    lens = np.diff(rp.astype(np.int64))
    if where == "A":                # the first / last entry of isolated rows: their neighbours must stay finite
        rows = [r for r in range(1, m - 1, max(m // 7, 3)) if lens[r] > 0][:6]
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
    mask = N.finite_mask_inputs(rp, ci, A, B, C, beta)
    return Problem(rp, ci, k, A, B, C, alpha, beta, dtype, ref=base.ref, bnd=base.bnd, mask=mask, nonfinite=True)


def judge(got, P, what):
    got = np.asarray(got)
    assert got.shape == (P.m, P.n) and got.dtype == P.dtype, (what, got.shape, got.dtype)
    if P.expected is not None:
        bad = ~(got == P.expected)
        if bad.any():
            r, c = np.argwhere(bad)[0]
            pytest.fail("%s: %d of %d outputs differ from the exact grid result; first (row %d, col %d): got %r, want %r"
                        % (what, bad.sum(), bad.size, r, c, got[r, c], P.expected[r, c]))
        return
    if P.nonfinite:
        ok, msg = N.check_classes(got, P.rp, P.ci, P.A, P.B, P.C, *_scalars(P.alpha, P.beta, P.dtype))
        assert ok, "%s: %s" % (what, msg)
    res = N.check_bound(np.where(P.mask, got, 0.0) if P.mask is not None else got, P.ref, P.bnd, P.mask)
    assert res, "%s: %r" % (what, res)


def regimes_for(i, family_index):
    """the grid regime of width index i on family j: every family meets every regime over the widths"""
    return GRID[(i + family_index) % len(GRID)]


def cells(n, fam_list, dtype=F64):
    """(family, problem) pairs of the grid sweep at width n"""
    i = WIDTHS.index(n) if n in WIDTHS else n
    out = []
    for j, fam in enumerate(fam_list):
        m, k, rp, ci = matrix(fam)
        out.append((fam, grid(fam, rp, ci, k, n, regimes_for(i, j), dtype, seed=i + 7 * j)))
    return out


def general_cells(n, fam_list, dtype=F64, placements=("A", "B", "C")):
    """R4 (three scalar pairs) and R5 (one placement per scalar pair; C only where beta != 0)"""
    out = []
    for j, fam in enumerate(fam_list):
        m, k, rp, ci = matrix(fam)
        for q, (alpha, beta) in enumerate(R4_SCALARS):
            out.append((fam + "/R4", general(fam, rp, ci, k, n, alpha, beta, dtype, seed=j)))
        for q, where in enumerate(placements):
            alpha, beta = R4_SCALARS[1 + q % 2] if where == "C" else R4_SCALARS[q % 3]
            out.append((fam + "/R5" + where, nonfinite(fam, rp, ci, k, n, alpha, beta, dtype, seed=j, where=where)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# entry points: each takes a Problem and returns the (m x n) result in the problem's value type
# ---------------------------------------------------------------------------------------------------------------------
def up(torch, dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def pack(X, order):
    """logical (r x c) -> (flat buffer, leading dimension)"""
    return (np.ascontiguousarray(X.T).reshape(-1), X.shape[0]) if order == COL else (np.ascontiguousarray(X).reshape(-1), X.shape[1])


def unpack(buf, order, r, c):
    return buf.reshape(c, r).T if order == COL else buf.reshape(r, c)


class Dev:
    def __init__(self, env, P, idx=I32):
        S, torch, dev = env
        self.rp, self.ci = up(torch, dev, P.rp.astype(idx)), up(torch, dev, P.ci.astype(idx))
        self.val = up(torch, dev, P.A)


def ws_f64(env, m, k, nnz, n):
    S, torch, dev = env
    return torch.empty(S.spmm_workspace_bytes(m, k, nnz, n) // 8 + 1, dtype=torch.float64, device=dev)


def run_spmm(env, P, idx=I32, entry="unplanned", ob=COL, oc=COL, plan=None, D=None):
    S, torch, dev = env
    D = D or Dev(env, P, idx)
    m, k, n, nnz = P.m, P.k, P.n, len(P.ci)
    Bf, ldb = pack(P.B, ob)
    Cf, ldc = pack(P.C, oc)
    B, C = up(torch, dev, Bf), up(torch, dev, Cf)
    f64i32 = P.dtype == np.float64 and idx == I32
    if entry == "unplanned" and f64i32:
        S.spmm(m, k, D.rp, D.ci, D.val, B, ldb, n, P.alpha, P.beta, C, ldc, ws_f64(env, m, k, nnz, n))
    elif entry == "plan":
        plan.spmm(D.val, B, ldb, n, P.alpha, P.beta, C, ldc, ws_f64(env, m, k, nnz, n))
    elif entry == "plan_ordered":
        plan.spmm_ordered(D.val, B, ldb, ob, n, P.alpha, P.beta, C, ldc, oc, ws_f64(env, m, k, nnz, n))
    elif entry == "rowmajorB":
        Bt = ws_f64(env, m, k, nnz, n)          # (the header's contract: (cols + 1) x ldbt and the verdicts behind)
        S.dense_to_rowmajor(k, n, B, ldb, Bt)
        S.spmm_rowmajorB(m, k, D.rp, D.ci, D.val, Bt, n, P.alpha, P.beta, C, ldc)
    elif entry == "tensor":
        Bt = B.view(n, k).t() if ob == COL else B.view(k, n)
        Ct = C.view(n, m).t() if oc == COL else C.view(m, n)
        S.spmm_tensor((m, k, D.rp, D.ci, D.val), Bt, Ct, P.alpha, P.beta, plan=plan)
    else:                                      # "unplanned" typed, or "ordered" in any type
        nb = S.spmm_typed_workspace_bytes(D.val.dtype, D.rp.dtype, m, k, nnz, n)
        ws = torch.full((nb + 1,), 0xFF, dtype=torch.uint8, device=dev)
        if entry == "ordered":
            S.spmm_ordered(m, k, D.rp, D.ci, D.val, B, ldb, ob, n, P.alpha, P.beta, C, ldc, oc, ws)
        else:
            S.spmm_typed(m, k, D.rp, D.ci, D.val, B, ldb, n, P.alpha, P.beta, C, ldc, ws)
    torch.cuda.synchronize()
    return unpack(C.cpu().numpy(), oc, m, n)


def run_spmv(env, P, idx=I32, plan=None):
    S, torch, dev = env
    D = Dev(env, P, idx)
    x, y = up(torch, dev, P.B[:, 0]), up(torch, dev, P.C[:, 0])
    if plan is not None:
        plan(D.val, x, P.alpha, P.beta, y)
    elif P.dtype == np.float64 and idx == I32:
        S.spmv(P.m, P.k, D.rp, D.ci, D.val, x, P.alpha, P.beta, y)
    else:
        S.spmv_typed(P.m, P.k, D.rp, D.ci, D.val, x, P.alpha, P.beta, y)
    torch.cuda.synchronize()
    return y.cpu().numpy()[:, None]


# ---------------------------------------------------------------------------------------------------------------------
# SpMM, unplanned, column-major: every selection x every width
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", WIDTHS)
@pytest.mark.parametrize("variant", SPMM_VARIANTS)
def test_spmm_grid_exact(env, variant_env, variant, n):
    S = env[0]
    variant_env(variant)
    for fam, P in cells(n, SPMM_FAMILIES):
        S.panel_census()
        got = run_spmm(env, P)
        census = S.panel_census()
        judge(got, P, "%s n=%d %s" % (variant, n, fam))
        if fam == "block" and n > 32:      # the census of test_spmm_mfma_block_structured: the regime ran where it claims
            if variant == "mfma":
                assert census["mfma"] > 0 and census["windowed"] == 0 and census["direct"] == 0, census
            if variant == "nomfma":
                assert census["mfma"] == 0, census
        if fam == "banded" and n == 64 and variant in ("auto", "nomfma"):      # the 64-column LDS-tiled kernel
            assert census["windowed"] > 0 and census["fallback"] == 0, census


@pytest.mark.parametrize("n", [17, 128])
@pytest.mark.parametrize("variant", SPMM_VARIANTS)
def test_spmm_general_and_nonfinite(env, variant_env, variant, n):
    variant_env(variant)
    for what, P in general_cells(n, SPMM_FAMILIES):
        judge(run_spmm(env, P), P, "%s n=%d %s a=%g b=%g" % (variant, n, what, P.alpha, P.beta))


# ---------------------------------------------------------------------------------------------------------------------
# subnormal A or B values (not only subnormal products) where the kernels that could flush them run, by the census:
# the f64 MFMA (its A / B inputs follow MODE.denorm) and the narrow LDS-tiled kernel, whose lanes' partial sums are
# added with LDS atomics (ds_add_f64)
# ---------------------------------------------------------------------------------------------------------------------
SUBNORMAL_INPUTS = {"A": dict(scale=-1050, scale_b=-24), "B": dict(scale=-24, scale_b=-1050)}


@pytest.fixture
def min_ldbt_env():
    yield from _env_switch("SBLAS_SPMM_MIN_LDBT")


def subnormal_grid(fam, n, which, seed):
    m, k, rp, ci = matrix(fam)
    key = ("subnormal", fam, n, which, seed)
    if key not in _PROBLEMS:
        alpha, beta = [(1.0, 0.0), (2.0, 1.0), (-1.0, 0.5), (1.0, -0.25)][seed % 4]
        g = N.grid_problem(rp, ci, k, n, seed=seed, alpha=alpha, beta=beta, **SUBNORMAL_INPUTS[which])
        vals = g.A if which == "A" else g.B
        assert (np.abs(vals) < np.finfo(np.float64).tiny).mean() > 0.9            # the inputs themselves are subnormal
        _PROBLEMS[key] = Problem(rp, ci, k, g.A, g.B, g.C, g.alpha, g.beta, F64, expected=g.expected)
    return _PROBLEMS[key]


@pytest.mark.parametrize("which", ["A", "B"])
def test_subnormal_inputs_on_matrix_cores_and_lds_tiled_kernels(env, variant_env, min_ldbt_env, which):
    S = env[0]
    runs = [("mfma", "block", n, "64") for n in (64, 65, 128, 256)]                       # the matrix cores, forced
    runs += [("auto", "wideband", n, "64") for n in (1, 5, 8)]                            # the narrow LDS-tiled kernel
    runs += [("auto", "wideband", n, "0") for n in (16, 17, 32)]                          # its 16- / 32-column forms
    runs += [("auto", "banded", 64, "64"), ("nomfma", "wideband", 128, "64")]            # the 64-column LDS-tiled kernel
    for i, (variant, fam, n, min_ldbt) in enumerate(runs):
        variant_env(variant)
        min_ldbt_env(min_ldbt)
        P = subnormal_grid(fam, n, which, seed=i)
        S.panel_census()
        got = run_spmm(env, P)
        census = S.panel_census()
        judge(got, P, "subnormal %s: %s n=%d %s" % (which, variant, n, fam))
        if variant == "mfma":
            assert census["mfma"] > 0 and census["windowed"] == 0 and census["direct"] == 0, (n, census)
        else:
            assert census["windowed"] > 0 and census["direct"] == 0 and census["fallback"] == 0, (fam, n, census)


# ---------------------------------------------------------------------------------------------------------------------
# SpMM plans, split plans, order pairs, the row-major-B entry, spmm_tensor
# ---------------------------------------------------------------------------------------------------------------------
ORDERS = [(COL, COL), (COL, ROW), (ROW, COL), (ROW, ROW)]


@pytest.mark.parametrize("n", [8, 17, 64, 128, 256])
def test_spmm_plans_orders_and_entries(env, n):
    S, torch, dev = env
    i = WIDTHS.index(n)
    probs = cells(n, SPMM_FAMILIES) + [(fam, grid(fam, *matrix(fam)[2:], matrix(fam)[1], n, GRID[(i + j + 2) % 4], F64,
                                                  seed=50 + j)) for j, fam in enumerate(SPMM_FAMILIES)]
    probs.append(("longrows", grid("longrows", *matrix("longrows")[2:], matrix("longrows")[1], n, GRID[i % 4], F64, seed=60)))
    if n in (17, 128):
        probs += general_cells(n, ["powerlaw", "random", "longrows"])
    for fam, P in probs:
        fam0 = fam.split("/")[0]
        m, k, rp, ci = matrix(fam0)
        D = Dev(env, P)
        plan = S.SpmmPlan(m, k, D.rp, D.ci, n)
        split = S.SpmmPlan(m, k, D.rp, D.ci, n, split=True, split_min=500, piece=128)
        # the split plan really splits: rows of 600, 700 and 1400 entries in direct panels (the short rows of
        # "powerlaw" leave a call of 64 columns or fewer unclassified, and so unsplit)
        if fam0 == "longrows" and n >= 17 or fam0 == "powerlaw" and n >= 128:
            assert split.split_info()["split_rows"] >= 1, (fam, n, split.split_info())
        if fam0 == "queen" and n >= 128:    # the row-merging kernel (test_planned_call_is_bit_identical_..., "grid")
            assert plan.info()["merge"], plan.info()
        if fam0 == "banded" and n == 64:
            assert plan.info()["windowed"] > 0, plan.info()
        judge(run_spmm(env, P, entry="plan", plan=plan, D=D), P, "plan n=%d %s" % (n, fam))
        for ob, oc in ORDERS:
            what = "n=%d %s orders %d%d" % (n, fam, ob, oc)
            judge(run_spmm(env, P, entry="ordered", ob=ob, oc=oc, D=D), P, "ordered " + what)
            judge(run_spmm(env, P, entry="plan_ordered", ob=ob, oc=oc, plan=split, D=D), P, "split plan " + what)
        judge(run_spmm(env, P, entry="rowmajorB", D=D), P, "rowmajorB n=%d %s" % (n, fam))
        judge(run_spmm(env, P, entry="tensor", ob=ROW, oc=COL, plan=plan, D=D), P, "tensor n=%d %s" % (n, fam))
        plan.destroy()
        split.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# SpMV: every selection, the plan (split rows included)
# ---------------------------------------------------------------------------------------------------------------------
SPMV_FAMILIES = ["banded", "powerlaw", "random", "long"]


def spmv_cells(fam_list, dtype=F64):
    out = []
    for j, fam in enumerate(fam_list):
        m, k, rp, ci = matrix(fam)
        for i, reg in enumerate(GRID):
            out.append((fam + "/" + reg, grid(fam, rp, ci, k, 1, reg, dtype, seed=3 * i + j)))
    return out + general_cells(1, fam_list, dtype)


@pytest.mark.parametrize("variant", SPMV_VARIANTS)
def test_spmv_every_selection(env, spmv_variant_env, variant):
    spmv_variant_env(variant)
    for what, P in spmv_cells(SPMV_FAMILIES):
        judge(run_spmv(env, P), P, "spmv %s %s a=%g b=%g" % (variant, what, P.alpha, P.beta))


def test_spmv_plan_with_split_rows(env):
    S = env[0]
    for what, P in spmv_cells(SPMV_FAMILIES):
        fam = what.split("/")[0]
        D = Dev(env, P)
        plan = S.SpmvPlan(P.m, P.k, D.rp, D.ci)
        if fam == "long":
            assert plan.info()["split_rows"] >= 1
        judge(run_spmv(env, P, plan=plan), P, "spmv plan %s a=%g b=%g" % (what, P.alpha, P.beta))
        plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# transposed products: A^T x, A^T B in both orders, split and unsplit
# ---------------------------------------------------------------------------------------------------------------------
def transposed(fam, n, regime_or_general, dtype=F64, seed=0):
    """The problem of A^T (built on the host CSC) and A's values in CSR order."""
    m, k, rp, ci = matrix(fam)
    cp, ri, perm = N.csc_of(m, k, rp, ci)
    cp, ri = cp.astype(np.int32), ri.astype(np.int32)
    if regime_or_general in GRID:
        P = grid(fam + "^T", cp, ri, m, n, regime_or_general, dtype, seed)
    else:
        P = regime_or_general(fam + "^T", cp, ri, m)
    val = np.empty_like(P.A)
    val[perm] = P.A
    return P, val


@pytest.mark.parametrize("fam,split", [("banded", False), ("random", False), ("tall", True), ("powerlaw", True)])
def test_transposed_products(env, fam, split):
    S, torch, dev = env
    m, k, rp, ci = matrix(fam)
    rp_d, ci_d = up(torch, dev, rp), up(torch, dev, ci)
    for n in ((1, 17) if fam == "tall" else (1, 17, 128)):
        probs = [transposed(fam, n, reg, seed=i) for i, reg in enumerate(GRID)]
        for alpha, beta in R4_SCALARS:
            probs.append(transposed(fam, n, lambda key, a, b, kk: general(key, a, b, kk, n, alpha, beta, F64, 3)))
        for j, where in enumerate("ABC"):
            alpha, beta = R4_SCALARS[1 + j % 2]
            probs.append(transposed(fam, n, lambda key, a, b, kk: nonfinite(key, a, b, kk, n, alpha, beta, F64, 3, where)))
        for P, val in probs:
            plan = S.TransposePlan(m, k, rp_d, ci_d, up(torch, dev, val), n=0 if n == 1 else n, split=split)
            if split and fam == "tall":
                info = plan.info()
                assert info["spmv_split_rows"] >= 1 and (n == 1 or info["spmm_split_rows"] >= 1), info
            what = "A^T %s n=%d split=%s a=%g b=%g" % (fam, n, split, P.alpha, P.beta)
            if n == 1:
                x, y = up(torch, dev, P.B[:, 0]), up(torch, dev, P.C[:, 0])
                plan.spmv(x, P.alpha, P.beta, y)
                torch.cuda.synchronize()
                judge(y.cpu().numpy()[:, None], P, what)
            else:
                ws = ws_f64(env, k, m, len(ci), n)
                for ob, oc in ((COL, COL), (ROW, ROW), (COL, ROW)):
                    Bf, ldb = pack(P.B, ob)
                    Cf, ldc = pack(P.C, oc)
                    B, C = up(torch, dev, Bf), up(torch, dev, Cf)
                    plan.spmm_ordered(B, ldb, ob, n, P.alpha, P.beta, C, ldc, oc, ws)
                    torch.cuda.synchronize()
                    judge(unpack(C.cpu().numpy(), oc, k, n), P, what + " orders %d%d" % (ob, oc))
            plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# typed paths: (f32, i32), (f32, i64), (f64, i64)
# ---------------------------------------------------------------------------------------------------------------------
TYPED = [(F32, I32), (F32, I64), (F64, I64)]


@pytest.mark.parametrize("vt,it", TYPED)
@pytest.mark.parametrize("n", [1, 7, 17, 64, 65, 128])
def test_typed_spmm(env, vt, it, n):
    probs = cells(n, ["banded", "random", "powerlaw"], vt)
    probs += [(f, grid(f, *matrix(f)[2:], matrix(f)[1], n, reg, vt, seed=90 + i))
              for i, (f, reg) in enumerate(zip(["banded", "random", "powerlaw"], GRID[1:]))]
    if n in (17, 128):
        probs += general_cells(n, ["banded", "random"], vt)
    for what, P in probs:
        judge(run_spmm(env, P, idx=it, entry="unplanned"), P, "typed %s/%s n=%d %s" % (vt.__name__, it.__name__, n, what))
        for ob, oc in ORDERS[1:]:
            judge(run_spmm(env, P, idx=it, entry="ordered", ob=ob, oc=oc), P,
                  "typed ordered %d%d %s/%s n=%d %s" % (ob, oc, vt.__name__, it.__name__, n, what))


@pytest.mark.parametrize("vt,it", TYPED)
def test_typed_spmv(env, vt, it):
    for what, P in spmv_cells(["banded", "powerlaw", "random"], vt):
        judge(run_spmv(env, P, idx=it), P, "typed spmv %s/%s %s a=%g b=%g" % (vt.__name__, it.__name__, what, P.alpha, P.beta))


# ---------------------------------------------------------------------------------------------------------------------
# merges: the folded-rank row-block merge and axpby (operands are B rows: A = 1, one entry per block covering a row)
# ---------------------------------------------------------------------------------------------------------------------
def merge_structure(M, starts, nrows):
    """output row r sums block q's row r - starts[q] for every block covering r: entries point into the stacked blocks"""
    offs = np.concatenate([[0], np.cumsum(nrows)])
    rows, cols = [], []
    for q, (s, c) in enumerate(zip(starts, nrows)):
        rows.append(np.arange(s, s + c))
        cols.append(offs[q] + np.arange(c))
    r, c = np.concatenate(rows), np.concatenate(cols)
    order = np.lexsort((c, r))
    rp = np.zeros(M + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=M), out=rp[1:])
    return rp.astype(np.int32), c[order].astype(np.int32), int(offs[-1])


def folded(P):
    """A grid problem with A folded into B (exact: the products of grid values are grid values).  Every row of B is
    referenced by one entry only (the stacked blocks, axpby's x)."""
    assert len(np.unique(P.ci)) == len(P.ci)
    Bf = P.B.copy()
    Bf[P.ci] = (P.A.astype(np.float64)[:, None] * P.B.astype(np.float64)[P.ci]).astype(P.dtype)
    return Problem(P.rp, P.ci, P.k, np.ones(len(P.ci), P.dtype), Bf, P.C, P.alpha, P.beta, P.dtype, expected=P.expected)


def test_merge_rowblocks_local(env):
    S, torch, dev = env
    vt = F64
    M, N = 500, 24
    starts, nrows = [0, 160, 250, 499], [250, 180, 250, 1]
    rp, ci, K = merge_structure(M, starts, nrows)
    offs = np.concatenate([[0], np.cumsum(nrows)])
    probs = [folded(grid("merge", rp, ci, K, N, reg, vt, seed=i)) for i, reg in enumerate(GRID)]
    probs += [general("merge", rp, ci, K, N, a, b, vt, 5, ones=True) for a, b in R4_SCALARS]
    probs += [nonfinite("merge", rp, ci, K, N, a, b, vt, 5, w, ones=True) for w, (a, b) in zip("BC", R4_SCALARS[1:])]
    for P in probs:
        stacked = P.B                            # (K x N): block q is rows offs[q]:offs[q+1]
        blocks = [up(torch, dev, np.ascontiguousarray(stacked[offs[q]:offs[q + 1]].T).reshape(-1)) for q in range(4)]
        C = up(torch, dev, np.ascontiguousarray(P.C.T).reshape(-1))
        S.merge_rowblocks_local(M, N, starts, nrows, blocks, P.alpha, P.beta, C)
        torch.cuda.synchronize()
        judge(C.cpu().numpy().reshape(N, M).T, P, "merge %s a=%g b=%g" % (vt.__name__, P.alpha, P.beta))


@pytest.mark.parametrize("vt", [F64, F32])
def test_axpby(env, vt):
    """y = beta*y + alpha*x; unlike the products it reads y under beta = 0 (kernel.h semantics), so C stays finite"""
    S, torch, dev = env
    n = 3001
    rp, ci = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)
    probs = [folded(grid("axpby", rp, ci, n, 1, reg, vt, seed=i)) for i, reg in enumerate(GRID)]
    probs += [general("axpby", rp, ci, n, 1, a, b, vt, 6, ones=True) for a, b in R4_SCALARS[1:]]
    probs += [nonfinite("axpby", rp, ci, n, 1, a, b, vt, 6, w, ones=True) for w, (a, b) in zip("BC", R4_SCALARS[1:])]
    assert len(probs) >= 5
    for P in probs:
        x, y = up(torch, dev, P.B[:, 0]), up(torch, dev, P.C[:, 0])
        if vt == F64:
            S.axpby(n, P.alpha, x, P.beta, y)
        else:
            S.axpby_typed(n, P.alpha, x, P.beta, y)
        torch.cuda.synchronize()
        judge(y.cpu().numpy()[:, None], P, "axpby %s a=%g b=%g" % (vt.__name__, P.alpha, P.beta))
