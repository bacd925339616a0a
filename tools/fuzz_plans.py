"""Randomised differential test of the plans added after the SpMM fuzz (tools/fuzz_parity.py), one GPU.

  python tools/fuzz_plans.py [--op OP|all] [--cases N] [--seed S] [--only K] [--max-rows R]

Operations: transpose, coo, spgemm, sddmm, softmax, attention, sptrsv, ilu0, color, pipeline.  Case k of operation op
draws from np.random.default_rng([seed, index of op, k]); its parameters are printed when it fails (and with --only), so
`--op X --seed S --only K` replays it.  Exit status 1 on the first mismatch; nothing retries a failing case.

Every operation is judged only by the reference its own GPU test file uses, at that file's bar (the numpy modules under
tests/): no tolerance is defined here.  Each operation has three host-only pieces -- draw_<op>() makes the problem,
ref_<op>() the answer the references give, judge_<op>() raises AssertionError on an answer they refuse -- and
case_<op>(case, rng, dev, max_rows), which draws, computes the answer on the device, judges it and returns what the case
exercised.  tests/test_fuzz_plans_host.py runs the first three without a GPU (and shows that the judges refuse spoiled
answers); tests/test_gpu_fuzz_plans.py runs case_<op> and asserts a census of the returned dicts.

The shared generator structure() draws a family, damage, a degenerate shape and one planted long row whose length lies
below, at, above or far above a limit read at run time from sptrsv_limits() / ilu0_limits() / color_limits() /
spgemm_limits() (for softmax and attention: the longest row that needs no workspace, found by asking the workspace
functions).  Family, degenerate shape and planted (limit, length) pair rotate with the case number, so that any run of RUN
consecutive cases meets every one of them, and at rates that have no common factor, so that a longer run pairs every
family with every limit and length (drawn_plant()); everything else is drawn."""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "s-blas_amd", "python"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import sblas_amd as S
from sblas_amd import synth
import numerics as NM
import sptrsv_numerics as TN
import ilu0_numerics as IN
import color_numerics as CN
import spgemm_numerics as GN
import sddmm_numerics as DN
import softmax_numerics as XN
import attention_numerics as AN

OPS = ["transpose", "coo", "spgemm", "sddmm", "softmax", "attention", "sptrsv", "ilu0", "color", "pipeline"]
FAMILIES = ["banded", "powerlaw", "random", "blocks", "grid5", "messy", "random_lower", "staircase", "near_diagonal",
            "arrow_band", "clique", "star"]
DAMAGE = ["none", "shuffle", "dups", "empty"]
DEGENERATE = ["rows0", "rows1", "nnz0", "col1", "one_row"]
RELATIONS = ["below", "at", "above", "far"]              # limit - 1, limit, limit + 1, 2 * limit + 3
RUN = 60                                                  # cases after which every rotated draw has occurred
PLANT_SHIFT = 5                                           # see drawn_plant()
MIN_ROWS = 8                                              # the fewest rows a family is drawn with
FAMILY_DRAWS = 20                                         # parameter draws a family gets before its refusal is raised
COO_RUN = 64                                              # the issue's figure for a long duplicate run of triplets
# The bar tests/test_gpu_softmax.py holds the device to against numpy_backward.  Here it is also put on the forward
# pass and on attention's P, against numpy's own: a check on top of the Decimal bounds of the sampled rows, over every
# row, and no looser than where it comes from.
SOFTMAX_ALLCLOSE = dict(rtol=1e-11, atol=1e-15)
I32, F64 = np.int32, np.float64


def bits(a):
    return np.ascontiguousarray(a, F64).view(np.int64)


def csr32(rp, ci):
    return np.ascontiguousarray(rp, I32), np.ascontiguousarray(ci, I32)


# ---------------------------------------------------------------------------------------------------------------------
# the shared generator (host only)
# ---------------------------------------------------------------------------------------------------------------------
def _family(kind, rng, rows, max_rows, square):
    """(rows, cols, rowptr, colidx) of one family; raises ValueError & co. on a draw its generator refuses"""
    seed = int(rng.integers(1 << 30))
    cols = None
    if kind == "banded":
        per = int(rng.integers(1, 24))
        rp, ci, _ = synth.banded(rows, per, int(rng.integers(per, 40 * per + 2)), seed=seed)
    elif kind == "powerlaw":
        rp, ci, _ = synth.powerlaw(max(rows, 10), avg=float(rng.uniform(1.5, 8)), max_len=int(rng.integers(10, 600)), seed=seed)
    elif kind == "random":
        cols = rows if square else int(rng.integers(1, max_rows + 1))
        rp, ci, _ = synth.random_csr(rows, cols, float(rng.uniform(0.2, 20)), seed=seed, sorted_rows=bool(rng.random() < 0.5),
                                     empty_every=int(rng.choice([0, 0, 3, 17])))
    elif kind == "blocks":
        rp, ci, _ = synth.block_structured(max(rows, 64), nnz_per_row=int(rng.integers(8, 48)), half_band=int(rng.integers(300, 3000)),
                                           fill=float(rng.uniform(0.2, 1.0)), seed=seed)
    elif kind == "grid5":
        rp, ci = IN.grid5(max(2, math.isqrt(rows)))
    elif kind == "messy":
        rp, ci = TN.messy(rng, rows)
    elif kind == "random_lower":
        rp, ci = TN.random_lower(rng, max(rows, 2), int(rng.integers(1, 6)))
    elif kind == "staircase":
        cr = S.sptrsv_limits()["chain_rows"]
        count = max(1, min(int(rng.integers(2, 12)), max_rows // (cr + 2)))
        rp, ci = TN.staircase([max(1, int(w)) for w in cr + rng.integers(-2, 3, count)])
    elif kind == "near_diagonal":
        rp, ci = IN.random_near_diagonal(rng, rows, int(rng.integers(2, 12)), int(rng.integers(1, 200)))
    elif kind == "arrow_band":
        top = max(2, min(300, max_rows // 2 - 12))
        rp, ci, _ = IN.arrow_band([int(v) for v in rng.integers(1, top + 1, int(rng.integers(2, 5)))], every=int(rng.integers(2, 7)))
    elif kind == "clique":
        rp, ci = CN.clique(int(rng.integers(2, min(150, max_rows) + 1)))
    elif kind == "star":
        rp, ci = CN.star(int(rng.integers(1, max_rows)))
    else:
        raise KeyError(kind)
    rows = len(rp) - 1
    return rows, (rows if cols is None else cols), np.asarray(rp, np.int64), np.asarray(ci, np.int64)


def _degenerate(kind, rng, max_rows, square):
    small = int(rng.integers(1, 40))
    if kind == "rows0":
        return 0, (0 if square else small), np.zeros(1, np.int64), np.zeros(0, np.int64)
    if kind == "rows1":
        cols = 1 if square else small
        k = int(rng.integers(1, 2 * cols + 1))
        return 1, cols, np.array([0, k], np.int64), rng.integers(0, cols, k)
    rows = int(rng.integers(2, max(3, max_rows // 4)))
    cols = rows if square else small
    if kind == "nnz0":
        return rows, cols, np.zeros(rows + 1, np.int64), np.zeros(0, np.int64)
    if kind == "col1":                                    # a single column (of a square matrix: only column 0 is named)
        lens = rng.integers(0, 4, rows)
        rp = np.concatenate([[0], np.cumsum(lens)])
        return rows, (rows if square else 1), rp, np.zeros(int(rp[-1]), np.int64)
    r, k = int(rng.integers(rows)), int(rng.integers(1, 3 * cols + 1))      # every entry in one row
    rp = np.zeros(rows + 1, np.int64)
    rp[r + 1:] = k
    return rows, cols, rp, rng.integers(0, cols, k)


def _damage(kind, rng, rows, rp, ci):
    rp, ci = rp.copy(), ci.copy()
    if kind == "shuffle" and len(ci) and rows:
        for r in rng.integers(0, rows, size=max(1, rows // 5)):
            a, b = rp[r], rp[r + 1]
            ci[a:b] = ci[a:b][rng.permutation(b - a)]
    elif kind == "dups" and len(ci) > 1:
        idx = rng.integers(1, len(ci), size=max(1, len(ci) // 30))
        ci[idx] = ci[idx - 1]                             # may cross a row boundary: still a valid column
    elif kind == "empty" and rows:
        q = int(rng.choice([2, 3, 7]))
        lens = np.diff(rp)
        keep = np.repeat(np.arange(rows) % q != q - 1, lens)
        lens[q - 1::q] = 0
        rp, ci = np.concatenate([[0], np.cumsum(lens)]), ci[keep]
    return rp, ci


def drawn_plant(limits, k):
    """the planted row of case k: the (limit, length) pairs take turns with the case number, so that every
    round of the families (len(FAMILIES) cases from a multiple of that) meets every pair, and the turn is shifted by PLANT_SHIFT once per round of the families: a
    family meets another pair in every round, and every pair after as many rounds as there are pairs (PLANT_SHIFT has
    no factor in common with 4, 8 or 12, the numbers of pairs of one, two or three limits)"""
    pairs = [(name, rel) for name in sorted(limits) for rel in RELATIONS]
    assert math.gcd(PLANT_SHIFT, len(pairs)) == 1 and len(pairs) <= len(FAMILIES), sorted(limits)
    name, rel = pairs[(k + PLANT_SHIFT * (k // len(FAMILIES))) % len(pairs)]
    L = {"below": limits[name] - 1, "at": limits[name], "above": limits[name] + 1, "far": 2 * limits[name] + 3}[rel]
    return dict(name=name, rel=rel, L=int(L))


def structure(rng, max_rows, square, limits=None, case=None, grow=None):
    """-> dict(rows, cols, rp, ci (int64; rows may be unsorted, hold duplicates, lack diagonals), family (None for a
    degenerate shape, which uses none), damage, degenerate (a name or None), plant (None or dict(name, rel, L))).
    limits: {name: value}: the plant is drawn here and put in by the operation, after it has conformed the pattern to
    its contract.  grow: None, or the rows beyond L to which the matrix is padded with empty rows so that a row of L
    distinct columns fits.  case: the case number (None: family, degenerate shape and planted limit are drawn too)."""
    if max_rows < MIN_ROWS:
        raise ValueError("max_rows is %d: the families need at least %d rows" % (max_rows, MIN_ROWS))
    k = int(rng.integers(1 << 20)) if case is None else case
    degenerate = DEGENERATE[(k // 7) % len(DEGENERATE)] if k % 7 == 3 else None
    family = None if degenerate else FAMILIES[k % len(FAMILIES)]
    damage = str(rng.choice(DAMAGE))
    if degenerate:
        rows, cols, rp, ci = _degenerate(degenerate, rng, max_rows, square)
    else:
        for attempt in range(FAMILY_DRAWS):
            try:
                rows, cols, rp, ci = _family(family, rng, int(rng.integers(MIN_ROWS, max_rows + 1)), max_rows, square)
                break
            except (ValueError, IndexError, ZeroDivisionError):           # a parameter draw the generator refuses
                if attempt == FAMILY_DRAWS - 1:
                    raise
    rp, ci = _damage(damage, rng, rows, rp, ci)
    plant = None
    if limits and not degenerate and k % 5 != 4:
        plant = drawn_plant(limits, k)
        more = 0 if grow is None else plant["L"] + grow - rows
        if more > 0:
            rp = np.concatenate([rp, np.full(more, rp[-1])])
            rows += more
            cols = max(cols, rows) if square else cols
    return dict(rows=rows, cols=cols, rp=rp, ci=ci, family=family, damage=damage, degenerate=degenerate, plant=plant)


def replace_row(rp, ci, r, new):
    """the CSR with row r's columns replaced by `new`"""
    new = np.asarray(new, np.int64)
    rp2 = rp.copy()
    rp2[r + 1:] += len(new) - (rp[r + 1] - rp[r])
    return rp2, np.concatenate([ci[:rp[r]], new, ci[rp[r + 1]:]])


def distinct(rng, lo, hi, count, without=None):
    """`count` distinct integers of [lo, hi) other than `without`, in random order"""
    pool = np.arange(lo, hi)
    if without is not None:
        pool = pool[pool != without]
    return rng.permutation(pool)[:count]


def census_of(st, **more):
    out = dict(family=st["family"], damage=st["damage"], degenerate=st["degenerate"],
               planted=(st["plant"]["name"], st["plant"]["rel"]) if st["plant"] else None)
    out.update(more)
    return out


def params_of(op, case, st, **more):
    out = dict(op=op, case=case, family=st["family"], damage=st["damage"], degenerate=st["degenerate"], rows=st["rows"],
               cols=st["cols"], plant=st["plant"])
    out.update(more)
    return out


def need(cond, P, what, *detail):
    if not cond:
        raise AssertionError("%s: %s %s" % (what, " ".join(str(d) for d in detail), P["params"]))


def need_equal(got, want, P, what):
    got, want = np.asarray(got), np.asarray(want)
    need(got.shape == want.shape, P, what, "shape", got.shape, "for", want.shape)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    need(len(bad) == 0, P, what, "%d of %d entries differ, first at %s: %r for %r" % (
        len(bad), want.size, bad[:1], got.reshape(-1)[bad[:1]], want.reshape(-1)[bad[:1]]))


def need_bits(got, want, P, what, nan_as_nan=False):
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    need(got.shape == want.shape, P, what, "shape", got.shape, "for", want.shape)
    if nan_as_nan:                                        # which NaN an operation makes is the adder's choice
        nan = np.isnan(want)
        need(np.array_equal(np.isnan(got), nan), P, what, "NaNs elsewhere")
        got, want = got[~nan], want[~nan]
    need_equal(bits(got), bits(want), P, what + " (bits)")


def wanted(P, ref):
    """the references' answer, made once per problem"""
    if "_want" not in P:
        P["_want"] = ref(P)
    return P["_want"]


def _workspace_threshold(nbytes):
    """the longest row that needs no workspace: the greatest nnz of a one-row matrix for which nbytes(1, nnz) is 0"""
    lo, hi = 1, 2
    while nbytes(1, hi) == 0:
        lo, hi = hi, 2 * hi
        if hi > 1 << 24:
            raise AssertionError("no workspace threshold below 2^24")
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if nbytes(1, mid) == 0 else (lo, mid)
    return lo


def up(dev, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def padded(dev, a, pad, fill=float("nan"), col_major=False):
    """a 2-D numpy array as a device view with `pad` unused elements behind every row (or column, col_major)"""
    import torch
    r, c = a.shape
    if col_major:
        buf = torch.full((c, r + pad), fill, dtype=torch.float64, device=dev)
        view = buf[:, :r].t()
    else:
        buf = torch.full((r, c + pad), fill, dtype=torch.float64, device=dev)
        view = buf[:, :c]
    view.copy_(up(dev, a))
    return view


# ---------------------------------------------------------------------------------------------------------------------
# transpose
# ---------------------------------------------------------------------------------------------------------------------
def draw_transpose(case, rng, max_rows):
    limits = dict(spmv_split=S.SPMV_SPLIT_MIN, spmm_split=S.SPMM_SPLIT_MIN)
    st = structure(rng, max_rows, False, None, case)
    rows, cols, rp, ci = st["rows"], st["cols"], st["rp"], st["ci"]
    k = case
    if not st["degenerate"] and rows and cols and k % 5 != 4:        # the planted row is a row of A^T: a column of A
        st["plant"] = drawn_plant(limits, k)
        L = st["plant"]["L"]
        c = int(rng.integers(cols))
        row = NM.row_of_entries(rp)
        keep = ci != c
        row, col = np.concatenate([row[keep], rng.integers(0, rows, L)]), np.concatenate([ci[keep], np.full(L, c)])
        key = np.concatenate([np.arange(int(keep.sum()), dtype=F64), rng.uniform(0, max(int(keep.sum()), 1), L)])
        order = np.lexsort((key, row))
        ci = col[order]
        rp = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=rows))])
    nnz = len(ci)
    n = int(rng.choice([1, 8, 33, 64]))
    P = dict(st=st, rows=rows, cols=cols, rp=rp, ci=ci, n=n, split=bool(case % 3 == 1), alpha=float(rng.choice([1.0, -2.5, 3.0])),
             beta=float(rng.choice([0.0, 1.0, -0.5])), val=rng.standard_normal(nnz), val2=NM.log_uniform(rng, nnz, 6),
             x=rng.standard_normal(rows), y0=rng.standard_normal(cols), B=rng.standard_normal((rows, n)),
             C0=rng.standard_normal((cols, n)), col_major=(bool(rng.random() < 0.5), bool(rng.random() < 0.5)),
             pad=(int(rng.choice([0, 3])), int(rng.choice([0, 5]))))
    P["params"] = params_of("transpose", case, st, nnz=nnz, n=n, split=P["split"], alpha=P["alpha"], beta=P["beta"],
                            col_major=P["col_major"], pad=P["pad"])
    P["csc"] = NM.csc_of(rows, cols, rp, ci)
    return P


def _transpose_products(P):
    """(colptr, rowidx, valT after update_values, y0 and C0 as the references read them)"""
    cp, ri, perm = P["csc"]
    beta = P["beta"]
    return cp, ri, P["val2"][perm], (P["y0"][:, None] if beta else None), (P["C0"] if beta else None)


def ref_transpose(P):
    cp, ri, perm = P["csc"]
    ans = dict(colptr=cp.astype(I32), rowidx=ri.astype(I32), perm=perm.astype(I32), valT=P["val"][perm])
    cp, ri, vT, y0, C0 = _transpose_products(P)
    for key, dense, old in (("y", P["x"][:, None], y0), ("C", P["B"], C0)):
        hi, lo = NM.reference_dd(cp, ri, vT, dense, old, P["alpha"], P["beta"])
        ans[key] = (hi + lo).reshape(-1) if key == "y" else hi + lo
    ans["_bound"] = dict(y=NM.bound(cp, ri, vT, P["x"][:, None], y0, P["alpha"], P["beta"], F64).reshape(-1),
                         C=NM.bound(cp, ri, vT, P["B"], C0, P["alpha"], P["beta"], F64))
    return ans


def judge_transpose(P, ans):
    cp, ri, perm = P["csc"]
    need_equal(ans["colptr"], cp, P, "colptr")
    need_equal(ans["rowidx"], ri, P, "rowidx")
    need_equal(ans["perm"], perm, P, "perm")
    need_bits(ans["valT"], P["val"][perm], P, "valT")
    cp, ri, vT, y0, C0 = _transpose_products(P)
    res = NM.check_general(np.asarray(ans["y"])[:, None], cp, ri, vT, P["x"][:, None], y0, P["alpha"], P["beta"], F64)
    need(res, P, "A^T x", res)
    res = NM.check_general(ans["C"], cp, ri, vT, P["B"], C0, P["alpha"], P["beta"], F64)
    need(res, P, "A^T B", res)


def case_transpose(case, rng, dev, max_rows):
    import torch
    P = draw_transpose(case, rng, max_rows)
    rows, cols, n = P["rows"], P["cols"], P["n"]
    rp, ci = csr32(P["rp"], P["ci"])
    drp, dci, dval = up(dev, rp), up(dev, ci), up(dev, P["val"])
    cp, ri, perm = P["csc"]
    for val, with_perm in ((dval, True), (None, True), (dval, False)):
        got = S.csr_transpose(rows, cols, drp, dci, val, with_perm=with_perm)
        torch.cuda.synchronize()
        need_equal(got[0].cpu().numpy(), cp, P, "csr_transpose colptr")
        need_equal(got[1].cpu().numpy(), ri, P, "csr_transpose rowidx")
        need((got[2] is None) == (val is None) and (got[3] is None) == (not with_perm), P, "csr_transpose", "None where asked")
        if val is not None:
            need_bits(got[2].cpu().numpy(), P["val"][perm], P, "csr_transpose valT")
        if with_perm:
            need_equal(got[3].cpu().numpy(), perm, P, "csr_transpose perm")
    plan = S.TransposePlan(rows, cols, drp, dci, dval, n=n, split=P["split"])
    try:
        info = plan.info()
        c0, c1, c2 = plan.csc()
        ans = dict(colptr=c0.cpu().numpy(), rowidx=c1.cpu().numpy(), perm=perm, valT=c2.cpu().numpy())
        plan.update_values(up(dev, P["val2"]))
        beta = P["beta"]
        y = up(dev, P["y0"]) if beta else torch.full((cols,), float("nan"), dtype=torch.float64, device=dev)
        if rows and cols:
            plan.spmv(up(dev, P["x"]), P["alpha"], beta, y)
        dB = padded(dev, P["B"], P["pad"][0], col_major=P["col_major"][0])
        dC = padded(dev, P["C0"] if beta else np.full((cols, n), np.nan), P["pad"][1], col_major=P["col_major"][1])
        if rows and cols:
            plan.spmm_tensor(dB, dC, P["alpha"], beta)
        torch.cuda.synchronize()
        ans["y"], ans["C"] = y.cpu().numpy(), dC.cpu().numpy()
    finally:
        plan.destroy()
    torch.cuda.synchronize()
    if not (rows and cols):                               # nothing to multiply: the products are the references' own
        ref = ref_transpose(P)
        ans["y"], ans["C"] = ref["y"], ref["C"]
    judge_transpose(P, ans)
    return census_of(P["st"], split_rows=info["spmv_split_rows"] + info["spmm_split_rows"])


# ---------------------------------------------------------------------------------------------------------------------
# coo
# ---------------------------------------------------------------------------------------------------------------------
def restate_coo(*args):
    """the numpy restatement of the COO contract that tests/test_gpu_coo.py holds the device to (its restate())"""
    import test_gpu_coo
    return test_gpu_coo.restate(*args)


def draw_coo(case, rng, max_rows):
    st = structure(rng, max_rows, False, dict(run=COO_RUN), case)
    rows, cols, rp, ci = st["rows"], st["cols"], st["rp"], st["ci"]
    r = NM.row_of_entries(rp)
    c = ci.copy()
    if len(r) and rng.random() < 0.5:                     # split duplicates: some triplets listed two to four times
        again = rng.integers(0, len(r), max(1, len(r) // 10))
        times = rng.integers(1, 4, len(again))
        r, c = np.concatenate([r, np.repeat(r[again], times)]), np.concatenate([c, np.repeat(c[again], times)])
    if st["plant"] and rows and cols:                     # the planted run: one (row, col) pair listed L times
        L = st["plant"]["L"]
        pr, pc = int(rng.integers(rows)), int(rng.integers(cols))
        keep = ~((r == pr) & (c == pc))
        r, c = np.concatenate([r[keep], np.full(L, pr)]), np.concatenate([c[keep], np.full(L, pc)])
    order = rng.permutation(len(r))
    r, c = r[order].astype(I32), c[order].astype(I32)
    nnz = len(r)
    P = dict(st=st, rows=rows, cols=cols, r=r, c=c, dup=str(rng.choice(["keep", "sum"])),
             val=NM.log_uniform(rng, nnz, 20), val2=rng.standard_normal(nnz))
    P["params"] = params_of("coo", case, st, triplets=nnz, plan_dup=P["dup"])
    return P


COO_KEYS = ("rowptr", "colidx", "val", "perm", "runptr")


def ref_coo(P):
    ans = {}
    for dup in ("keep", "sum"):
        ans[dup] = dict(zip(COO_KEYS, restate_coo(P["rows"], P["cols"], P["r"], P["c"], P["val"], dup)))
    ans["plan"] = dict(ans[P["dup"]])
    ans["plan"]["val2"] = restate_coo(P["rows"], P["cols"], P["r"], P["c"], P["val2"], P["dup"])[2]
    return ans


def judge_coo(P, ans):
    want = wanted(P, ref_coo)
    for which in ("keep", "sum", "plan"):
        for key, w in want[which].items():
            if key.startswith("val"):
                need_bits(ans[which][key], w, P, "%s %s" % (which, key))
            else:
                need_equal(ans[which][key], w, P, "%s %s" % (which, key))


def case_coo(case, rng, dev, max_rows):
    import torch
    P = draw_coo(case, rng, max_rows)
    dr, dc, dv, dv2 = up(dev, P["r"]), up(dev, P["c"]), up(dev, P["val"]), up(dev, P["val2"])
    ans = {}
    for dup in ("keep", "sum"):
        got = S.coo_to_csr(P["rows"], P["cols"], dr, dc, dv, dup=dup)
        torch.cuda.synchronize()
        ans[dup] = {k: t.cpu().numpy() for k, t in zip(COO_KEYS, got)}
    plan = S.CooPlan(P["rows"], P["cols"], dr, dc, dup=P["dup"])
    try:
        info = plan.info()
        rowptr, colidx, perm, runptr = (t.cpu().numpy().copy() for t in plan.csr())
        first = plan.assemble(dv).cpu().numpy()
        second = plan.assemble(dv2).cpu().numpy()
        again = plan.assemble(dv).cpu().numpy()
        ans["plan"] = dict(rowptr=rowptr, colidx=colidx, perm=perm, runptr=runptr, val=first, val2=second)
    finally:
        plan.destroy()
    torch.cuda.synchronize()
    need_bits(again, first, P, "assemble after other values")
    judge_coo(P, ans)
    return census_of(P["st"], triplets=len(P["r"]), longest_run=info["longest_run"])


# ---------------------------------------------------------------------------------------------------------------------
# spgemm
# ---------------------------------------------------------------------------------------------------------------------
SPGEMM_MODES = (("auto", dict()), ("general", dict(general=True)), ("chunks", dict(general=True, chunk_cap=257)))


def _random_b(rng, k, n, per_row, ascending):
    """k x n: distinct columns in every row, ascending or (not ascending) shuffled inside the rows with a few doubled"""
    lens = rng.integers(0, 2 * per_row + 1, k)
    row = np.repeat(np.arange(k, dtype=np.int64), lens)
    key = np.unique(row * max(n, 1) + rng.integers(0, max(n, 1), len(row))) if n else np.zeros(0, np.int64)
    row, col = key // max(n, 1), key % max(n, 1)
    if not ascending and len(col):
        again = rng.integers(0, len(col), max(1, len(col) // 20))
        row, col = np.concatenate([row, row[again]]), np.concatenate([col, col[again]])
        order = np.lexsort((rng.random(len(row)), row))
        row, col = row[order], col[order]
    return np.concatenate([[0], np.cumsum(np.bincount(row, minlength=k))]).astype(np.int64), col


def draw_spgemm(case, rng, max_rows):
    lim = S.spgemm_limits()
    st = structure(rng, max_rows, False, dict(acc_cap=lim["acc_cap"], s_max=lim["s_max"]), case)
    m, k, rpa, cia = st["rows"], st["cols"], st["rp"], st["ci"]
    if st["plant"]:                                       # row 0 .. of A must be able to name a B row
        k = max(k, 2)
    n = int(rng.integers(1, max_rows + 1))
    ascending = bool(rng.random() < 0.5)
    if case % 2 and len(cia):                             # A unsorted with duplicates in half the cases
        rpa, cia = _damage("dups", rng, m, *_damage("shuffle", rng, m, rpa, cia))
    plant = st["plant"]
    if plant and plant["name"] == "s_max":
        n = max(n, plant["L"])
    elif plant:
        n = max(n, plant["L"] + int(rng.integers(0, 50)))
    rpb, cib = _random_b(rng, k, n, int(rng.integers(1, 9)), ascending)
    if plant and m:
        ra, rb = int(rng.integers(m)), int(rng.integers(k))
        if plant["name"] == "acc_cap":                    # one B row of L distinct columns, one A row that names it alone
            new = distinct(rng, 0, n, plant["L"])
            rpb, cib = replace_row(rpb, cib, rb, np.sort(new) if ascending else new)
            rpa, cia = replace_row(rpa, cia, ra, [rb])
        else:                                             # two B rows whose columns span exactly L, named by one A row
            rb2 = (rb + 1) % k
            rpb, cib = replace_row(rpb, cib, rb, [0])
            rpb, cib = replace_row(rpb, cib, rb2, [plant["L"] - 1])
            rpa, cia = replace_row(rpa, cia, ra, [rb2, rb] if case % 4 < 2 else [rb, rb2])
    v = lambda count: NM.log_uniform(rng, count, 6)
    P = dict(st=st, m=m, k=k, n=n, A=csr32(rpa, cia), B=csr32(rpb, cib), va=[v(len(cia)), v(len(cia))], vb=[v(len(cib)), v(len(cib))])
    P["params"] = params_of("spgemm", case, st, m=m, k=k, n=n, nnz_a=len(cia), nnz_b=len(cib), b_ascending=ascending,
                            a_messy=bool(case % 2))
    return P


def ref_spgemm(P):
    (rpa, cia), (rpb, cib) = P["A"], P["B"]
    out = [GN.reference(P["m"], P["n"], rpa, cia, P["va"][i], rpb, cib, P["vb"][i]) for i in range(2)]
    return dict(rowptr=out[0][0], colidx=out[0][1], val=out[0][2], val2=out[1][2])


def judge_spgemm(P, ans, want=None, what="spgemm"):
    want = wanted(P, ref_spgemm) if want is None else want
    need_equal(ans["rowptr"], want["rowptr"], P, what + " rowptr")
    need_equal(ans["colidx"], want["colidx"], P, what + " colidx")
    for key in ("val", "val2"):
        need(GN.same_bits(ans[key], want[key]), P, what + " " + key, "differs from the reference in",
             int((bits(ans[key]) != bits(want[key])).sum()) if np.shape(ans[key]) == np.shape(want[key]) else "shape", "entries")


def case_spgemm(case, rng, dev, max_rows):
    import torch
    P = draw_spgemm(case, rng, max_rows)
    want = wanted(P, ref_spgemm)
    dA, dB = [up(dev, a) for a in P["A"]], [up(dev, a) for a in P["B"]]
    dva, dvb = [up(dev, v) for v in P["va"]], [up(dev, v) for v in P["vb"]]
    seen = dict(rows_row=0, rows_general=0, chunks=0)
    for mode, kw in SPGEMM_MODES:
        plan = S.SpgemmPlan(P["m"], P["k"], P["n"], dA[0], dA[1], dB[0], dB[1], **kw)
        try:
            info = plan.info()
            rp, ci = (t.cpu().numpy().copy() for t in plan.csr())
            val = plan.multiply(dva[0], dvb[0]).cpu().numpy()
            val2 = plan.multiply(dva[1], dvb[1]).cpu().numpy()
        finally:
            plan.destroy()
        torch.cuda.synchronize()
        judge_spgemm(P, dict(rowptr=rp, colidx=ci, val=val, val2=val2), want, "spgemm / " + mode)
        need(info["nnz_c"] == len(want["colidx"]), P, "nnz_c", mode, info)
        need(mode == "auto" or info["rows_row"] == 0, P, "rows_row", mode, info)
        if mode == "auto":
            seen.update(rows_row=info["rows_row"], rows_general=info["rows_general"])
        seen["chunks"] = max(seen["chunks"], info["chunks"])
    return census_of(P["st"], **seen)


# ---------------------------------------------------------------------------------------------------------------------
# sddmm
# ---------------------------------------------------------------------------------------------------------------------
SDDMM_WORK = 1500000                                      # entries * k a case keeps, so that the double-double reference takes well under a second


def _leading_rows(rp, ci, budget):
    """the leading row block whose entries stay within the budget"""
    m = int(np.searchsorted(rp, budget, side="right")) - 1
    m = max(m, min(1, len(rp) - 1))
    return m, rp[:m + 1], ci[:rp[m]]


def draw_sddmm(case, rng, max_rows):
    st = structure(rng, max_rows, False, None, case)
    k = int(rng.choice([1, 3, 16, 17, 64, 130]))
    rows, rp, ci = _leading_rows(st["rp"], st["ci"], SDDMM_WORK // k)
    cols, nnz = st["cols"], len(ci)
    block = None
    if rng.random() < 0.4 and rows > 2:                   # a re-based row block, X addressed through x_offset
        a = int(rng.integers(0, rows - 1))
        block = (a, int(rng.integers(a + 1, rows + 1)))
    alpha = float(rng.choice([1.0, -0.5, 2.0]))
    beta = float(rng.choice([0.0, 0.0, 2.0, -0.25]))
    X, Y = NM.log_uniform(rng, (rows, k), 6), NM.log_uniform(rng, (cols, k), 6)
    old = NM.log_uniform(rng, nnz, 6)
    nonfinite = case % 8 == 5
    if nonfinite:
        for arr in (X, Y, old):
            if arr.size:
                spots = rng.integers(0, arr.size, max(1, arr.size // 200))
                arr.reshape(-1)[spots] = rng.choice([np.inf, -np.inf, np.nan, 0.0], len(spots))
    P = dict(st=st, rows=rows, cols=cols, rp=rp, ci=ci, k=k, block=block, alpha=alpha, beta=beta, X=X, Y=Y, old=old,
             nonfinite=nonfinite, col_major=(bool(rng.random() < 0.4), bool(rng.random() < 0.4)),
             pad=(int(rng.choice([0, 3])), int(rng.choice([0, 2]))))
    P["params"] = params_of("sddmm", case, st, used_rows=rows, nnz=nnz, k=k, block=block, alpha=alpha, beta=beta,
                            nonfinite=nonfinite, col_major=P["col_major"], pad=P["pad"])
    return P


def _sddmm_scope(P):
    """(entry range judged, rowptr, colidx, X of the judged rows): the whole pattern, or the row block's own"""
    if P["block"] is None:
        return 0, len(P["ci"]), P["rp"], P["ci"], P["X"]
    a, b = P["block"]
    e0, e1 = int(P["rp"][a]), int(P["rp"][b])
    return e0, e1, P["rp"][a:b + 1] - e0, P["ci"][e0:e1], P["X"][a:b]


def ref_sddmm(P):
    e0, e1, rp, ci, X = _sddmm_scope(P)
    old = P["old"][e0:e1]
    out = np.full(len(P["ci"]), np.nan) if P["beta"] == 0 else P["old"].copy()
    if P["nonfinite"]:
        with np.errstate(all="ignore"):
            r, c = DN.entry_rows(rp, ci)
            out[e0:e1] = P["alpha"] * np.einsum("ek,ek->e", X[r], P["Y"][c]) + (P["beta"] * old if P["beta"] else 0.0)
        return dict(out=out)
    hi, lo = DN.reference_dd(rp, ci, X, P["Y"], old, P["alpha"], P["beta"])
    out[e0:e1] = hi + lo
    bound = np.zeros(len(out))
    bound[e0:e1] = DN.bound(rp, ci, X, P["Y"], old, P["alpha"], P["beta"])
    return dict(out=out, _bound=dict(out=bound))


def judge_sddmm(P, ans):
    e0, e1, rp, ci, X = _sddmm_scope(P)
    got, old = np.asarray(ans["out"], F64), P["old"][e0:e1]
    need(got.shape == P["old"].shape, P, "sddmm", "shape", got.shape)
    start = np.full(len(got), np.nan) if P["beta"] == 0 else P["old"]
    outside = np.ones(len(got), bool)
    outside[e0:e1] = False
    need_equal(bits(got[outside]), bits(start[outside]), P, "entries outside the row block")
    if P["nonfinite"]:
        need_equal(DN.class_of(got[e0:e1]), DN.predict_class(rp, ci, X, P["Y"], old, P["alpha"], P["beta"]), P, "IEEE classes")
        return
    ok, worst, where, over = DN.check_general(got[e0:e1], rp, ci, X, P["Y"], old, P["alpha"], P["beta"])
    need(ok, P, "sddmm", "worst error / bound %.3g at entry %s, %d over" % (worst, where, over))


def case_sddmm(case, rng, dev, max_rows):
    import torch
    P = draw_sddmm(case, rng, max_rows)
    rows, cols, k = P["rows"], P["cols"], P["k"]
    rp, ci = csr32(P["rp"], P["ci"])
    out = up(dev, P["old"]) if P["beta"] else torch.full((len(ci),), float("nan"), dtype=torch.float64, device=dev)
    if P["block"] is None:
        dX = padded(dev, P["X"], P["pad"][0], col_major=P["col_major"][0])
        dY = padded(dev, P["Y"], P["pad"][1], col_major=P["col_major"][1])
        S.sddmm_tensor((rows, cols, up(dev, rp), up(dev, ci)), dX, dY, out, P["alpha"], P["beta"])
    else:
        a, b = P["block"]
        e0, e1 = int(rp[a]), int(rp[b])
        ldx, ldy = k + P["pad"][0], k + P["pad"][1]
        Xb, Yb = np.full((rows, ldx), np.nan), np.full((cols, ldy), np.nan)
        Xb[:, :k], Yb[:, :k] = P["X"], P["Y"]
        if e1 > e0:
            S.sddmm(b - a, cols, up(dev, (rp[a:b + 1] - e0).astype(I32)), up(dev, ci)[e0:e1], up(dev, Xb.reshape(-1)), ldx,
                    S.ROW_MAJOR, up(dev, Yb.reshape(-1)), ldy, S.ROW_MAJOR, k, P["alpha"], P["beta"], out[e0:e1], x_offset=a * ldx)
    torch.cuda.synchronize()
    judge_sddmm(P, dict(out=out.cpu().numpy()))
    return census_of(P["st"], k=k, block=P["block"] is not None, nonfinite=P["nonfinite"], beta=P["beta"] != 0)


# ---------------------------------------------------------------------------------------------------------------------
# softmax
# ---------------------------------------------------------------------------------------------------------------------
def softmax_limit():
    return _workspace_threshold(S.csr_softmax_workspace_bytes)


def draw_softmax(case, rng, max_rows):
    st = structure(rng, max_rows, False, dict(workspace=softmax_limit()), case)
    rp = st["rp"]
    if st["plant"] and st["rows"]:
        lens = np.diff(rp)
        lens[int(rng.integers(st["rows"]))] = st["plant"]["L"]
        rp = np.concatenate([[0], np.cumsum(lens)])
    rp = rp.astype(I32)
    scale = float(rng.choice([1.0, 0.125, -0.3]))
    seed = int(rng.integers(1 << 30))
    x = XN.scores(rp, seed, scale=scale)
    p = XN.numpy_forward(rp, XN.scores(rp, seed + 1, spread=20.0), 1.0)
    dp = rng.uniform(-2.0, 2.0, len(p))
    nonfinite = case % 8 == 5
    if nonfinite and len(x):
        spots = rng.integers(0, len(x), max(1, len(x) // 100))
        x[spots] = rng.choice([np.inf, -np.inf, np.nan], len(spots))
    P = dict(st=st, rp=rp, scale=scale, x=x, p=p, dp=dp, nonfinite=nonfinite, sample=XN.sample_rows(rp, seed=seed, n=3))
    P["params"] = params_of("softmax", case, st, nnz=len(x), scale=scale, nonfinite=nonfinite, longest=int(np.diff(rp).max()) if len(rp) > 1 else 0)
    return P


def ref_softmax(P):
    with np.errstate(all="ignore"):
        out = XN.numpy_forward(P["rp"], P["x"], P["scale"])
    return dict(out=out, dx=XN.numpy_backward(P["rp"], P["p"], P["dp"], P["scale"]))


def judge_softmax(P, ans):
    rp, scale = P["rp"], P["scale"]
    out, dx = np.asarray(ans["out"], F64), np.asarray(ans["dx"], F64)
    need(out.shape == P["x"].shape and dx.shape == P["x"].shape, P, "softmax", "shapes", out.shape, dx.shape)
    if P["nonfinite"]:
        bad = XN.class_mismatches(XN.predict_class(rp, P["x"], scale), out)
        need(len(bad) == 0, P, "softmax classes", "%d entries, first %s: %r" % (len(bad), bad[:1], out[bad[:1]]))
    else:
        res = XN.check_forward(out, rp, P["x"], scale, P["sample"])
        need(res["ok"], P, "softmax forward", res)
        want = XN.numpy_forward(rp, P["x"], scale)                   # every row, at the backward pass's bar (see SOFTMAX_ALLCLOSE)
        need(np.allclose(out, want, **SOFTMAX_ALLCLOSE), P, "softmax forward against numpy", "largest difference",
             float(np.abs(out - want).max()) if len(want) else 0.0)
    res = XN.check_backward(dx, rp, P["p"], P["dp"], scale, P["sample"])
    need(res["ok"], P, "softmax backward", res)
    want = XN.numpy_backward(rp, P["p"], P["dp"], scale)
    need(np.allclose(dx, want, **SOFTMAX_ALLCLOSE), P, "softmax backward against numpy", "largest difference",
         float(np.abs(dx - want).max()) if len(want) else 0.0)


def case_softmax(case, rng, dev, max_rows):
    import torch
    P = draw_softmax(case, rng, max_rows)
    R, X, Pp, DP = up(dev, P["rp"]), up(dev, P["x"]), up(dev, P["p"]), up(dev, P["dp"])
    out = S.csr_softmax(R, X, torch.full_like(X, float("nan")), P["scale"])
    dx = S.csr_softmax_backward(R, Pp, DP, torch.full_like(DP, float("nan")), P["scale"])
    X2, DP2 = X.clone(), DP.clone()
    S.csr_softmax(R, X2, X2, P["scale"])
    S.csr_softmax_backward(R, Pp, DP2, DP2, P["scale"])
    torch.cuda.synchronize()
    ans = dict(out=out.cpu().numpy(), dx=dx.cpu().numpy())
    nan = np.isnan(ans["out"])
    need(np.array_equal(np.isnan(X2.cpu().numpy()), nan), P, "softmax in place", "NaNs elsewhere")
    need_equal(bits(X2.cpu().numpy())[~nan], bits(ans["out"])[~nan], P, "softmax in place")
    need_equal(bits(DP2.cpu().numpy()), bits(ans["dx"]), P, "softmax backward in place")
    judge_softmax(P, ans)
    rows = len(P["rp"]) - 1
    return census_of(P["st"], workspace=S.csr_softmax_workspace_bytes(rows, len(P["x"])), nonfinite=P["nonfinite"])


# ---------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------
ATTENTION_WORK = 3000000                                  # entries * max(d, dv) a case keeps


def attention_limit():
    return _workspace_threshold(lambda rows, nnz: S.csr_attention_workspace_bytes(rows, nnz, 1, 1))


def draw_attention(case, rng, max_rows):
    st = structure(rng, max_rows, False, dict(workspace=attention_limit()), case)
    d, dv = int(rng.choice([1, 7, 64, 128])), int(rng.choice([1, 7, 64, 128]))
    rp, ci, cols = st["rp"], st["ci"], max(st["cols"], 1)
    if st["plant"] and st["rows"]:
        rp, ci = replace_row(rp, ci, int(rng.integers(st["rows"])), rng.integers(0, cols, st["plant"]["L"]))
    budget = ATTENTION_WORK // max(d, dv)
    if st["plant"]:
        budget = max(budget, int(rp[np.diff(rp).argmax() + 1]))                 # the planted row stays
    rows, rp, ci = _leading_rows(rp, ci, budget)
    u = lambda *shape: rng.uniform(-1.0, 1.0, shape)
    P = dict(st=st, rows=rows, cols=cols, rp=rp.astype(I32), ci=ci.astype(I32), d=d, dv=dv, scale=float(rng.choice(AN.SCALES)),
             Q=u(rows, d), K=u(cols, d), V=u(cols, dv), dO=u(rows, dv), pad=[int(v) for v in rng.choice([0, 3], 6)])
    P["sample"] = AN.sample_rows(rp, count=2, seed=case) if rows else []
    P["params"] = params_of("attention", case, st, used_rows=rows, nnz=len(ci), d=d, dv=dv, scale=P["scale"], pad=P["pad"],
                            longest=int(np.diff(rp).max()) if rows else 0)
    return P


def ref_attention(P):
    """the composition in numpy; `P` and `dS` double as the composition's own (the device compares bits with its own)"""
    rp, ci = P["rp"], P["ci"]
    O, prob, m, z = AN.numpy_attention(rp, ci, P["Q"], P["K"], P["V"], P["scale"])
    r = NM.row_of_entries(rp)
    dP = np.einsum("ek,ek->e", P["dO"][r], P["V"][ci.astype(np.int64)]) if len(ci) else np.zeros(0)
    dS = XN.numpy_backward(rp, prob, dP, P["scale"]) if len(ci) else np.zeros(0)
    dQ = AN.numpy_rows(rp, ci, dS, P["K"], P["rows"])
    return dict(O=O, dQ=dQ, P=prob, dS=dS, comp_P=prob.copy(), comp_dS=dS.copy())


def judge_attention(P, ans):
    rp, ci = P["rp"], P["ci"]
    need_bits(ans["P"], ans["comp_P"], P, "P against csr_softmax(sddmm(Q, K))")
    need_bits(ans["dS"], ans["comp_dS"], P, "dS against csr_softmax_backward(P, sddmm(dO, V))")
    need(np.shape(ans["O"]) == (P["rows"], P["dv"]) and np.shape(ans["dQ"]) == (P["rows"], P["d"]), P, "attention", "shapes")
    res = AN.check_rows(ans["O"], rp, ci, ans["P"], P["V"], P["sample"])
    need(res["ok"], P, "attention O", res)
    res = AN.check_rows(ans["dQ"], rp, ci, ans["dS"], P["K"], P["sample"])
    need(res["ok"], P, "attention dQ", res)
    # the weights themselves: the composition's P is a softmax of the pattern's rows (the bar is borrowed from the softmax's
    # backward pass, see SOFTMAX_ALLCLOSE: an extra check, the identity above and check_rows are the issue's)
    want = AN.numpy_attention(rp, ci, P["Q"], P["K"], P["V"], P["scale"])[1]
    need(np.allclose(ans["P"], want, **SOFTMAX_ALLCLOSE), P, "attention P against numpy")


def case_attention(case, rng, dev, max_rows):
    import torch
    P = draw_attention(case, rng, max_rows)
    rows, cols, pad = P["rows"], P["cols"], P["pad"]
    R, Ci = up(dev, P["rp"]), up(dev, P["ci"])
    A = (rows, cols, R, Ci)
    Q, K, V, dO = (padded(dev, P[k], pad[i]) for i, k in enumerate(("Q", "K", "V", "dO")))
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
    O, dQ = nan(rows, P["dv"] + pad[4])[:, :P["dv"]], nan(rows, P["d"] + pad[5])[:, :P["d"]]
    m, z, prob, dS = nan(rows), nan(rows), nan(len(P["ci"])), nan(len(P["ci"]))
    S.csr_attention(A, Q, K, V, P["scale"], O, m, z)
    S.csr_attention_backward(A, Q, K, V, dO, m, z, P["scale"], dQ, prob, dS)
    sc, dP = nan(len(P["ci"])), nan(len(P["ci"]))
    S.sddmm_tensor(A, Q, K, sc)
    comp_P = S.csr_softmax(R, sc, None, P["scale"])
    S.sddmm_tensor(A, dO, V, dP)
    comp_dS = S.csr_softmax_backward(R, comp_P, dP, None, P["scale"])
    torch.cuda.synchronize()
    judge_attention(P, {k: v.cpu().numpy() for k, v in dict(O=O, dQ=dQ, P=prob, dS=dS, comp_P=comp_P, comp_dS=comp_dS).items()})
    return census_of(P["st"], workspace=S.csr_attention_workspace_bytes(rows, len(P["ci"]), P["d"], P["dv"]), d=P["d"], dv=P["dv"])


# ---------------------------------------------------------------------------------------------------------------------
# sptrsv
# ---------------------------------------------------------------------------------------------------------------------
def schedules(widest):
    """the six schedules of tests/test_gpu_sptrsv.py"""
    import test_gpu_sptrsv
    return test_gpu_sptrsv.schedules(widest)


def _one_diagonal(rng, n, rp, ci, share=1.0):
    """the pattern with its stored diagonals removed and one put back, at a random place, in `share` of the rows"""
    row = NM.row_of_entries(rp)
    keep = ci != row
    add = np.flatnonzero(rng.random(n) < share) if share < 1.0 else np.arange(n)
    old = int(keep.sum())
    row2, col2 = np.concatenate([row[keep], add]), np.concatenate([ci[keep], add])
    key = np.concatenate([np.arange(old, dtype=F64), rng.uniform(-1.0, old, len(add))])
    order = np.lexsort((key, row2))
    return np.concatenate([[0], np.cumsum(np.bincount(row2, minlength=n))]).astype(np.int64), col2[order]


def draw_sptrsv(case, rng, max_rows):
    lim = S.sptrsv_limits()
    st = structure(rng, max_rows, True, dict(g4_max=lim["g4_max"], g16_max=lim["g16_max"]), case, grow=1)
    n, rp, ci = st["rows"], st["rp"], st["ci"]
    lower, unit, clean = bool(rng.random() < 0.5), bool(rng.random() < 0.3), bool(rng.random() < 0.4)
    if clean:                                             # the triangle alone, sorted; else as messy as the contract allows
        rp, ci = (np.asarray(a, np.int64) for a in TN.triangle_of(n, rp, ci, lower))
    else:
        rp, ci = _one_diagonal(rng, n, rp, ci, 0.5 if unit else 1.0)
    if st["plant"] and n:                                 # the row with every other row in its triangle: L stored entries
        r, L = (n - 1, st["plant"]["L"]) if lower else (0, st["plant"]["L"])
        off = distinct(rng, 0, n, L - 1, without=r)
        new = np.concatenate([np.sort(off), [r]]) if lower else np.concatenate([[r], np.sort(off)])
        rp, ci = replace_row(rp, ci, r, new if clean else rng.permutation(new))
    rp, ci = csr32(rp, ci)
    shape = [(n,), (n, 1), (n, 2), (n, 5), (n, 33)][int(rng.integers(5))]
    nrhs = None if len(shape) == 1 else shape[1]
    if n:
        g = TN.grid_problem(rng, n, rp, ci, lower, unit, nrhs)
    else:                                                 # nothing to solve: the references' reshapes need a row
        g = TN.Exact()
        g.val, g.alpha, g.b, g.x = np.zeros(0), 0.5, np.zeros(shape), np.zeros(shape)
    P = dict(st=st, n=n, rp=rp, ci=ci, lower=lower, unit=unit, alpha=float(rng.choice([1.0, -1.25, 0.5, 2.0])), shape=shape,
             val=TN.dominant_values(rng, n, rp, ci, lower, unit), b=NM.log_uniform(rng, shape, 8), grid=g,
             pad=(int(rng.choice([0, 3])), int(rng.choice([0, 5]))), in_place=bool(rng.random() < 0.4))
    lv, nl = TN.levels(n, rp, ci, lower)
    P["widest"] = int(TN.level_widths(lv, nl).max()) if n else 0
    P["params"] = params_of("sptrsv", case, st, nnz=len(ci), lower=lower, unit=unit, clean=clean, alpha=P["alpha"], shape=shape,
                            pad=P["pad"], in_place=P["in_place"], levels=nl, widest=P["widest"])
    return P


def ref_sptrsv(P):
    if P["n"] == 0:
        return dict(x=np.zeros(P["shape"]), grid_x=np.zeros(P["shape"]), _bound=dict(x=np.zeros(P["shape"])))
    x = TN.reference(P["n"], P["rp"], P["ci"], P["val"], P["b"], P["lower"], P["unit"], P["alpha"])
    _, bnd = TN.residual_bound(P["n"], P["rp"], P["ci"], P["val"], P["b"], x, P["lower"], P["unit"], P["alpha"])
    dg = TN.on_diagonal(P["rp"], P["ci"])
    diag = np.ones(P["n"])
    if not P["unit"]:
        diag[NM.row_of_entries(P["rp"])[dg]] = np.abs(P["val"][dg])
    # a change dx of x[i] moves row i's residual by t_ii dx: the bound on x that the residual bound implies for that row
    return dict(x=x, grid_x=P["grid"].x.copy(), _bound=dict(x=bnd / diag.reshape((-1,) + (1,) * (x.ndim - 1))))


def judge_sptrsv(P, ans):
    g = P["grid"]
    need_equal(np.asarray(ans["grid_x"]), g.x, P, "the exact grid's x")
    x = np.asarray(ans["x"], F64)
    need(x.shape == tuple(P["shape"]), P, "sptrsv", "shape", x.shape)
    if P["n"] == 0:
        return
    try:
        TN.check_residual(P["n"], P["rp"], P["ci"], P["val"], P["b"], x, P["lower"], P["unit"], P["alpha"], what="fuzz")
    except AssertionError as e:
        need(False, P, "sptrsv residual", e)


def _solve_into(P, plan, dev, dval, b, alpha):
    """one solve with the case's padding and placement -> x as numpy"""
    import torch
    n, shape = P["n"], P["shape"]
    if len(shape) == 1:
        db = up(dev, b)
        x = db if P["in_place"] else torch.full_like(db, -7.0)
        plan.solve(dval, db, x=x, alpha=alpha)
        return x.cpu().numpy()
    db = padded(dev, b, P["pad"][0])
    xbuf = torch.full((n, shape[1] + P["pad"][1]), -7.0, dtype=torch.float64, device=dev)
    x = db if P["in_place"] else xbuf[:, :shape[1]]
    plan.solve(dval, db, x=x, alpha=alpha)
    need(bool((xbuf[:, shape[1]:] == -7.0).all()), P, "sptrsv", "the padding of X was written")
    return x.cpu().numpy()


def case_sptrsv(case, rng, dev, max_rows):
    import torch
    P = draw_sptrsv(case, rng, max_rows)
    g = P["grid"]
    drp, dci, dval, dgval = up(dev, P["rp"]), up(dev, P["ci"]), up(dev, P["val"]), up(dev, g.val)
    first, auto = None, None
    for label, kw in schedules(P["widest"]):
        plan = S.SptrsvPlan(P["n"], drp, dci, lower=P["lower"], unit_diag=P["unit"], **kw)
        try:
            info = plan.info()
            got = dict(x=_solve_into(P, plan, dev, dval, P["b"], P["alpha"]), grid_x=_solve_into(P, plan, dev, dgval, g.b, g.alpha))
        finally:
            plan.destroy()
        torch.cuda.synchronize()
        if first is None:
            first, auto = got, info
            judge_sptrsv(P, got)
        else:
            need_bits(got["x"], first["x"], P, "schedule %s against auto" % label)
            need_bits(got["grid_x"], first["grid_x"], P, "schedule %s against auto, exact grid" % label)
    return census_of(P["st"], wide=auto["wide_launches"], chain=auto["chain_launches"], lower=P["lower"], unit=P["unit"],
                     nrhs=P["shape"][1] if len(P["shape"]) == 2 else 0)


# ---------------------------------------------------------------------------------------------------------------------
# ilu0
# ---------------------------------------------------------------------------------------------------------------------
def ilu0_pattern(rng, st):
    """the structure conformed to ILU(0)'s contract (full_sorted) with its planted row of exactly L stored entries"""
    n = st["rows"]
    rp, ci = (np.asarray(a, np.int64) for a in IN.full_sorted(n, st["rp"], st["ci"]))
    if st["plant"] and n:
        r = int(rng.integers(n))
        rp, ci = replace_row(rp, ci, r, np.sort(np.concatenate([distinct(rng, 0, n, st["plant"]["L"] - 1, without=r), [r]])))
    return csr32(rp, ci)


def draw_ilu0(case, rng, max_rows):
    lim = S.ilu0_limits()
    st = structure(rng, max_rows, True, dict(g4_max=lim["g4_max"], g16_max=lim["g16_max"], lds_max=lim["lds_max"]), case, grow=1)
    n = st["rows"]
    rp, ci = ilu0_pattern(rng, st)
    P = dict(st=st, n=n, rp=rp, ci=ci, val=[IN.dominant_values(rng, n, rp, ci) for _ in range(2)],
             r=NM.log_uniform(rng, (n,) if rng.random() < 0.5 else (n, 3), 8))
    lv, nl = TN.levels(n, rp, ci, True)
    P["widest"] = int(TN.level_widths(lv, nl).max()) if n else 0
    # the same structure damaged after generation: a dropped diagonal, or a swapped pair
    bad_rp, bad_ci, kind = rp.astype(np.int64), ci.astype(np.int64), "none"
    lens = np.diff(bad_rp)
    if n and rng.random() < 0.5:
        i = int(rng.integers(n))
        bad_rp, bad_ci = replace_row(bad_rp, bad_ci, i, [c for c in bad_ci[bad_rp[i]:bad_rp[i + 1]] if c != i])
        kind = "dropped diagonal"
    elif (lens > 1).any():
        i = int(rng.choice(np.flatnonzero(lens > 1)))
        e = int(bad_rp[i] + rng.integers(lens[i] - 1))
        bad_ci = bad_ci.copy()
        bad_ci[[e, e + 1]] = bad_ci[[e + 1, e]]
        kind = "swapped pair"
    P["damaged"] = (kind,) + csr32(bad_rp, bad_ci)
    P["params"] = params_of("ilu0", case, st, nnz=len(ci), levels=nl, widest=P["widest"], longest=int(np.diff(rp).max()) if n else 0,
                            damaged=kind, nrhs=P["r"].shape[1:] or None)
    return P


def ref_ilu0(P):
    lu = [IN.ilu0_ref(P["n"], P["rp"], P["ci"], v) for v in P["val"]]
    return dict(lu=lu[0], lu2=lu[1])


def judge_ilu0(P, ans, want=None, what="ilu0"):
    want = wanted(P, ref_ilu0) if want is None else want
    need_bits(ans["lu"], want["lu"], P, what + " lu", nan_as_nan=True)
    need_bits(ans["lu2"], want["lu2"], P, what + " lu of the second values", nan_as_nan=True)


def judge_ilu0_structure(P):
    """the library's host check against ilu0_numerics.check, on the sound structure and on the damaged one"""
    n = P["n"]
    dpos, bad = IN.check(n, P["rp"], P["ci"])
    need(bad is None, P, "the generated structure", "is refused at row", bad)
    need_equal(S.ilu0_check(n, P["rp"], P["ci"]), dpos, P, "ilu0_check's diagonal positions")
    kind, rp, ci = P["damaged"]
    dpos, bad = IN.check(n, rp, ci)
    if kind == "none":
        return
    need(bad is not None, P, "the damaged structure", "passes the numpy check")
    try:
        S.ilu0_check(n, rp, ci)
    except S.SblasError as e:
        need(e.bad_row == bad, P, "ilu0_check", "names row", e.bad_row, "for", bad)
    else:
        need(False, P, "ilu0_check", "accepts the damaged structure")


def case_ilu0(case, rng, dev, max_rows):
    import torch
    P = draw_ilu0(case, rng, max_rows)
    judge_ilu0_structure(P)
    want = wanted(P, ref_ilu0)
    need(np.isfinite(want["lu"]).all() and np.isfinite(want["lu2"]).all(), P, "dominant values", "do not factor finitely")
    n = P["n"]
    drp, dci = up(dev, P["rp"]), up(dev, P["ci"])
    dval = [up(dev, v) for v in P["val"]]
    auto = None
    for label, kw in schedules(P["widest"]):
        plan = S.Ilu0Plan(n, drp, dci, **kw)
        try:
            info = plan.info()
            lu = plan.factor(dval[0], out=torch.full_like(dval[0], -7.0))
            lu2 = plan.factor(dval[1])
            torch.cuda.synchronize()
            judge_ilu0(P, dict(lu=lu.cpu().numpy(), lu2=lu2.cpu().numpy()), want, "ilu0 / " + label)
            if label == "auto":
                auto = info
                dr = up(dev, P["r"])
                got = plan.apply(lu, dr)
                lo_plan, up_plan = plan.solvers()
                by_hand = up_plan.solve(lu, lo_plan.solve(lu, dr))
                torch.cuda.synchronize()
                need_bits(got.cpu().numpy(), by_hand.cpu().numpy(), P, "apply against the two solves")
        finally:
            plan.destroy()
        torch.cuda.synchronize()
    if P["damaged"][0] != "none":
        try:
            S.Ilu0Plan(n, up(dev, P["damaged"][1]), up(dev, P["damaged"][2])).destroy()
        except S.SblasError as e:
            need(e.bad_row == IN.check(n, P["damaged"][1], P["damaged"][2])[1], P, "Ilu0Plan", "names row", e.bad_row)
        else:
            need(False, P, "Ilu0Plan", "accepts the damaged structure")
    return census_of(P["st"], wide=auto["wide_launches"], chain=auto["chain_launches"], long_rows=auto["long_rows"])


# ---------------------------------------------------------------------------------------------------------------------
# colour / permute
# ---------------------------------------------------------------------------------------------------------------------
def draw_color(case, rng, max_rows):
    lim = S.color_limits()
    st = structure(rng, max_rows, True, dict(g4_max=lim["g4_max"], g16_max=lim["g16_max"], window=lim["window"]), case, grow=0)
    n, rp, ci = st["rows"], st["rp"], st["ci"]
    if st["plant"]:                                       # one more vertex that names L others and that nobody names: p = L
        rp = np.concatenate([rp, [rp[-1] + st["plant"]["L"]]])
        ci = np.concatenate([ci, distinct(rng, 0, n, st["plant"]["L"])])
        n += 1
    rp, ci = csr32(rp, ci)
    P = dict(st=st, n=n, rp=rp, ci=ci, seed=int(rng.integers(0, 1 << 32)), perm=rng.permutation(n).astype(I32),
             val=rng.standard_normal(len(ci)), x=rng.standard_normal(n))
    P["params"] = params_of("color", case, st, n=n, nnz=len(ci), color_seed=P["seed"], largest_degree=int(CN.degrees(n, rp, ci).max()) if n else 0)
    return P


def ref_color(P):
    n, rp, ci = P["n"], P["rp"], P["ci"]
    color = CN.color_scalar(n, rp, ci, P["seed"])
    perm, inv, ptr, k = CN.order(color)
    rpb, cib, src = CN.permute(n, rp, ci, P["perm"])
    return dict(color=color, perm=perm, inv=inv, color_ptr=ptr, rowptr_b=rpb, colidx_b=cib, src=src, val_b=P["val"][src.astype(np.int64)],
                round_trip=P["x"].copy())


def judge_color(P, ans):
    want = wanted(P, ref_color)
    for key in ("color", "perm", "inv", "color_ptr", "rowptr_b", "colidx_b", "src"):
        need_equal(ans[key], want[key], P, key)
    try:
        CN.check_coloring(P["n"], P["rp"], P["ci"], np.asarray(ans["color"]), len(want["color_ptr"]) - 1)
    except AssertionError as e:
        need(False, P, "check_coloring", e)
    need_bits(ans["val_b"], want["val_b"], P, "the permuted values")
    need_bits(ans["round_trip"], P["x"], P, "from_permuted(to_permuted(x))")


def case_color(case, rng, dev, max_rows):
    import torch
    P = draw_color(case, rng, max_rows)
    n = P["n"]
    drp, dci = up(dev, P["rp"]), up(dev, P["ci"])
    plan = S.ColorPlan(n, drp, dci, seed=P["seed"])
    try:
        info = plan.info()
        ans = dict(zip(("color", "perm", "inv", "color_ptr"), (t.cpu().numpy().copy() for t in plan.order())))
    finally:
        plan.destroy()
    pp = S.PermutePlan(n, drp, dci, up(dev, P["perm"]))
    try:
        ans.update(zip(("rowptr_b", "colidx_b", "src"), (t.cpu().numpy().copy() for t in pp.csr())))
        ans["val_b"] = pp.values(up(dev, P["val"])).cpu().numpy()
        ans["round_trip"] = pp.from_permuted(pp.to_permuted(up(dev, P["x"]))).cpu().numpy()
    finally:
        pp.destroy()
    torch.cuda.synchronize()
    judge_color(P, ans)
    need(info["colors"] == len(ans["color_ptr"]) - 1, P, "info", info)
    return census_of(P["st"], colors=info["colors"], largest_degree=info["largest_degree"])


# ---------------------------------------------------------------------------------------------------------------------
# pipeline: COO -> CooPlan (sum) -> ColorPlan -> PermutePlan -> Ilu0Plan.factor -> apply
# ---------------------------------------------------------------------------------------------------------------------
def draw_pipeline(case, rng, max_rows):
    if case % 2:
        rp, ci = IN.grid5(int(rng.integers(2, max(3, math.isqrt(max_rows)) + 1)))
        family = "grid5"
    else:
        rp, ci = IN.random_near_diagonal(rng, int(rng.integers(2, max_rows + 1)), int(rng.integers(2, 10)), int(rng.integers(1, 100)))
        family = "near_diagonal"
    n = len(rp) - 1
    val = IN.dominant_values(rng, n, rp, ci)
    r, c = NM.row_of_entries(rp), ci.astype(np.int64)
    split = rng.random(len(c)) < 0.3                      # split duplicates: v as two or three triplets that sum to about v
    parts = rng.integers(2, 4, int(split.sum()))
    share = val[split] / parts
    r = np.concatenate([r[~split], np.repeat(r[split], parts)])
    c = np.concatenate([c[~split], np.repeat(c[split], parts)])
    v = np.concatenate([val[~split], np.repeat(share, parts) * rng.uniform(0.9, 1.1, int(parts.sum()))])
    order = rng.permutation(len(r))
    st = dict(family=family, damage="none", degenerate=None, plant=None, rows=n, cols=n)
    P = dict(st=st, n=n, r=r[order].astype(I32), c=c[order].astype(I32), v=v[order], seed=int(rng.integers(0, 1 << 32)),
             rhs=NM.log_uniform(rng, n, 8))
    P["params"] = params_of("pipeline", case, st, triplets=len(r), color_seed=P["seed"])
    return P


def ref_pipeline(P):
    """every stage by its own host reference, composed in the device's order"""
    n = P["n"]
    rp, ci, val, _, _ = restate_coo(n, n, P["r"], P["c"], P["v"], "sum")
    perm = CN.order(CN.color_scalar(n, rp, ci, P["seed"]))[0]
    rpb, cib, src = CN.permute(n, rp, ci, perm)
    valb = val[src.astype(np.int64)]
    need(IN.check(n, rpb, cib)[1] is None, P, "the permuted pattern", "does not meet ILU(0)'s contract")
    lu = IN.ilu0_ref(n, rpb, cib, valb)
    rhs_b = P["rhs"][perm.astype(np.int64)]
    y = TN.reference(n, rpb, cib, lu, rhs_b, True, True)
    x = TN.reference(n, rpb, cib, lu, y, False, False)
    # y_fresh, x_fresh: what a fresh Ilu0Plan makes of these references on the device; here the host's own stand in
    return dict(rowptr=rp, colidx=ci, val=val, perm=perm, rowptr_b=rpb, colidx_b=cib, val_b=valb, lu=lu, rhs_b=rhs_b, y=y, x=x,
                y_fresh=y.copy(), x_fresh=x.copy())


def judge_pipeline(P, ans):
    want = wanted(P, ref_pipeline)
    for key in ("rowptr", "colidx", "perm", "rowptr_b", "colidx_b"):
        need_equal(ans[key], want[key], P, "pipeline " + key)
    for key in ("val", "val_b", "lu", "rhs_b"):
        need_bits(ans[key], want[key], P, "pipeline " + key)
    n, rpb, cib, lu = P["n"], want["rowptr_b"], want["colidx_b"], want["lu"]
    try:                                                  # the two solves have no bit reference: the solves' own bar, stage by stage
        TN.check_residual(n, rpb, cib, lu, want["rhs_b"], np.asarray(ans["y"]), True, True, what="pipeline L")
        TN.check_residual(n, rpb, cib, lu, np.asarray(ans["y"]), np.asarray(ans["x"]), False, False, what="pipeline U")
    except AssertionError as e:
        need(False, P, "pipeline apply", e)
    # ... and by bits against a plan that never saw the earlier stages' device arrays: the hand-over changes nothing
    need_bits(ans["y"], ans["y_fresh"], P, "pipeline y against a fresh plan on the references")
    need_bits(ans["x"], ans["x_fresh"], P, "pipeline x against a fresh plan on the references")


def case_pipeline(case, rng, dev, max_rows):
    import torch
    P = draw_pipeline(case, rng, max_rows)
    n = P["n"]
    plans = []
    try:
        coo = S.CooPlan(n, n, up(dev, P["r"]), up(dev, P["c"]), dup="sum")
        plans.append(coo)
        rowptr, colidx, _, _ = coo.csr()
        val = coo.assemble(up(dev, P["v"]))
        color = S.ColorPlan(n, rowptr, colidx, seed=P["seed"])
        plans.append(color)
        pp = color.permute(rowptr, colidx)
        plans.append(pp)
        rpb, cib, _ = pp.csr()
        valb = pp.values(val)
        ilu = S.Ilu0Plan(n, rpb, cib)
        plans.append(ilu)
        lu = ilu.factor(valb)
        rhs_b = pp.to_permuted(up(dev, P["rhs"]))
        y = torch.full_like(rhs_b, -7.0)
        x = ilu.apply(lu, rhs_b, tmp=y)
        torch.cuda.synchronize()
        ans = {k: t.cpu().numpy().copy() for k, t in dict(rowptr=rowptr, colidx=colidx, val=val, perm=color.order()[1], rowptr_b=rpb,
                                                         colidx_b=cib, val_b=valb, lu=lu, rhs_b=rhs_b, y=y, x=x).items()}
        info = ilu.info()
    finally:
        for plan in reversed(plans):
            plan.destroy()
    torch.cuda.synchronize()
    want = wanted(P, ref_pipeline)
    fresh = S.Ilu0Plan(n, *(up(dev, a) for a in csr32(want["rowptr_b"], want["colidx_b"])))
    try:
        y = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
        x = fresh.apply(up(dev, want["lu"]), up(dev, want["rhs_b"]), tmp=y)
        torch.cuda.synchronize()
        ans["y_fresh"], ans["x_fresh"] = y.cpu().numpy().copy(), x.cpu().numpy().copy()
    finally:
        fresh.destroy()
    torch.cuda.synchronize()
    judge_pipeline(P, ans)
    return census_of(P["st"], wide=info["wide_launches"], chain=info["chain_launches"], levels=info["levels"])


DRAW = dict(transpose=draw_transpose, coo=draw_coo, spgemm=draw_spgemm, sddmm=draw_sddmm, softmax=draw_softmax,
            attention=draw_attention, sptrsv=draw_sptrsv, ilu0=draw_ilu0, color=draw_color, pipeline=draw_pipeline)
REF = dict(transpose=ref_transpose, coo=ref_coo, spgemm=ref_spgemm, sddmm=ref_sddmm, softmax=ref_softmax,
           attention=ref_attention, sptrsv=ref_sptrsv, ilu0=ref_ilu0, color=ref_color, pipeline=ref_pipeline)
JUDGE = dict(transpose=judge_transpose, coo=judge_coo, spgemm=judge_spgemm, sddmm=judge_sddmm, softmax=judge_softmax,
             attention=judge_attention, sptrsv=judge_sptrsv, ilu0=judge_ilu0, color=judge_color, pipeline=judge_pipeline)
CASE = dict(transpose=case_transpose, coo=case_coo, spgemm=case_spgemm, sddmm=case_sddmm, softmax=case_softmax,
            attention=case_attention, sptrsv=case_sptrsv, ilu0=case_ilu0, color=case_color, pipeline=case_pipeline)


def case_rng(seed, op, case):
    return np.random.default_rng([seed, OPS.index(op), case])


def run_case(op, case, seed, dev, max_rows):
    """case `case` of `op` on the device -> what it exercised; AssertionError (with the parameters) on a mismatch, and
    also when the library refuses a call of a generated case: every generated case is within the contracts"""
    try:
        return CASE[op](case, case_rng(seed, op, case), dev, max_rows)
    except S.SblasError as e:
        params = DRAW[op](case, case_rng(seed, op, case), max_rows)["params"]
        raise AssertionError("the library refused a call: %s %s" % (e, params)) from e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", default="all", choices=OPS + ["all"])
    ap.add_argument("--cases", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-rows", type=int, default=1500)
    ap.add_argument("--only", type=int, default=-1)
    args = ap.parse_args()
    if args.max_rows < MIN_ROWS:
        ap.error("--max-rows must be at least %d" % MIN_ROWS)
    import torch
    dev = torch.device("cuda:0")
    for op in (OPS if args.op == "all" else [args.op]):
        for case in ([args.only] if args.only >= 0 else range(args.cases)):
            try:
                seen = run_case(op, case, args.seed, dev, args.max_rows)
            except AssertionError as e:
                print("MISMATCH %s case %d: %s" % (op, case, e), flush=True)
                print("fuzz: FAILED (replay: --op %s --seed %d --max-rows %d --only %d)" % (op, args.seed, args.max_rows, case))
                return 1
            if args.only >= 0:
                print(DRAW[op](case, case_rng(args.seed, op, case), args.max_rows)["params"])
                print("exercised:", seen)
        print("%s: all cases match their references" % op, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
