"""Randomised differential test of the sparse algebra added after tools/fuzz_spmm.py, one GPU: CSR addition (GeamPlan),
masked SpGEMM (MaskedSpgemmPlan), the header's identity between masked SpGEMM and SpGEMM, and the gradients of
autograd.SpgemmOperator and autograd.csr_add in one graph.

  python tools/fuzz_algebra.py [--op OP|all] [--cases N] [--seed S] [--only K] [--max-rows R]

Operations: mspgemm, mspgemm_spgemm, geam, grad.  Case k of operation op draws from
np.random.default_rng([seed, index of op, k]); its parameters are printed when it fails (and with --only), so
`--op X --seed S --only K` replays it.  Exit status 1 on the first mismatch; nothing retries a failing case.

It follows tools/fuzz_plans.py, whose generator it imports and does not copy: the structures come from
fuzz_plans.structure() (every family, damage kind and degenerate shape, turning with the case number), the planted row
from drawn_plant(), B-like operands from _random_b().  No tolerance is defined here.  Values are judged bit for bit
(spgemm_numerics.same_bits: a NaN where the reference has one) against the library's scalar references S.geam_ref and
S.mspgemm_ref, which the host tests pin to the numpy restatements of the contracts; structures and maps on ==.  On top
of that mspgemm holds sampled entries to an error bound that shares no code with the reference (exact sums in
fractions.Fraction), and every operation to the metamorphic statements its header makes.

Each operation has host-only pieces -- draw_<op>() makes the problem, ref_<op>() the references' answer,
judge_<op>() raises AssertionError on an answer they refuse, reference_answer_<op>() is the answer in the form the device
run returns it -- and case_<op>(case, rng, dev, max_rows), which draws, computes on the device, judges and returns what
the case exercised.  tests/test_fuzz_algebra_host.py runs the host pieces without a GPU and shows that the judges refuse
spoiled answers; tests/test_gpu_fuzz_algebra.py runs case_<op> and asserts a census of the returned dicts.

What turns with the case number k (everything else is drawn):
  mspgemm         (x_ascending, y_ascending) (k // 2) % 4, the value regime k % 3, an exact fill of the last workgroup k % 6 == 1
  geam            B's relation to A k % 6, the value regime k % 3
  grad            the planted side k % 2, duplicates in A / B / neither k % 3, the requested gradients (k // 2) % 3,
                  general (k // 3) % 2"""
import argparse
import os
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "s-blas_amd", "python"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import sblas_amd as S
import fuzz_plans as FP
from fuzz_plans import FAMILIES, DAMAGE, DEGENERATE, RELATIONS, MIN_ROWS, need, need_equal, up      # imported, not copied
import numerics as NM
import spgemm_numerics as GN
import geam_numerics as AN

OPS = ["mspgemm", "mspgemm_spgemm", "geam", "grad"]
REGIMES = ["log_uniform", "grid", "nonfinite"]
ASCENDING_TURN = [(True, True), (True, False), (False, True), (False, False)]
GEAM_RELATIONS = ["independent", "subset", "same", "disjoint", "transpose", "empty"]
GEAM_WG = 256                                             # csrc/geam.h, GEAM_THREADS: the entries one workgroup of the entry passes takes
GEAM_SCAN_TILE = 4096                                     # csrc/radix_sort.h, SCAN_TILE: the flags one workgroup of the scan takes
WAVE = 64
SAMPLE = 200                                              # mask entries a case hands to the Fraction judge, the planted row's first
PLANT_MASK_ROW = (130, 200)                               # entries of the mask row over the planted X row: whole waves, and all sampled
SENTINEL = -7.25e300                                      # a preset of `out` that is no NaN: an unwritten entry shows beside a NaN too
DENSE_CELLS = 250000                                      # m * n up to which the gradients are also held to the dense bound
GRAD_NEED = ["both", "a", "b"]
I32, I64, F64 = np.int32, np.int64, np.float64
U = Fraction(1, 2 ** 53)


# ---------------------------------------------------------------------------------------------------------------------
# shared host pieces
# ---------------------------------------------------------------------------------------------------------------------
def rowptr_of(row, rows):
    return np.concatenate([[0], np.cumsum(np.bincount(np.asarray(row, I64), minlength=rows))]).astype(I64)


def split_rows(rp, ci):
    return [np.asarray(ci[rp[i]:rp[i + 1]], I64) for i in range(len(rp) - 1)]


def join_rows(rows):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(I64)
    return rp, (np.concatenate(rows).astype(I64) if len(rows) and rp[-1] else np.zeros(0, I64))


def ascending(rp, ci):
    """every row strictly ascending"""
    ci = np.asarray(ci, I64)
    if len(ci) < 2:
        return True
    ok = np.ones(len(ci), bool)
    ok[1:] = ci[1:] > ci[:-1]
    lens = np.diff(np.asarray(rp, I64))
    ok[np.asarray(rp, I64)[:-1][lens > 0]] = True
    return bool(ok.all())


def has_duplicates(rp, ci, cols):
    key = NM.row_of_entries(rp) * max(cols, 1) + np.asarray(ci, I64)
    return len(np.unique(key)) < len(key)


def clean_rows(rows, cols, rp, ci):
    """the pattern with every row ascending and free of duplicates"""
    key = np.unique(NM.row_of_entries(rp) * max(cols, 1) + np.asarray(ci, I64))
    return rowptr_of(key // max(cols, 1), rows), key % max(cols, 1)


def permute_rows(rp, p):
    """row i becomes row p[i], its entries in their order -> (rowptr, src): entry u of the result is entry src[u]"""
    new = np.asarray(p, I64)[NM.row_of_entries(rp)]
    return rowptr_of(new, len(rp) - 1), np.argsort(new, kind="stable")


def values(rng, count, regime):
    """log-uniform over six binades, the exact integer grid, or log-uniform with Inf / NaN / -0.0 sprinkled"""
    if regime == "grid":
        return rng.integers(-8, 9, count).astype(F64)
    v = NM.log_uniform(rng, count, 6)
    if regime == "nonfinite" and count:
        spots = rng.integers(0, count, max(1, count // 40))
        v[spots] = rng.choice([np.inf, -np.inf, np.nan, -0.0], len(spots))
    return v


def break_one(rng, rp, ci, cols):
    """one duplicate or one descent in one row: the least that makes a structure not ascending"""
    rp, ci = rp.copy(), ci.copy()
    lens = np.diff(rp)
    two = np.flatnonzero(lens >= 2)
    if len(two):
        r = int(rng.choice(two))
        a = int(rng.integers(rp[r], rp[r + 1] - 1))
        if rng.random() < 0.5:
            ci[a + 1] = ci[a]
        else:
            ci[[a, a + 1]] = ci[[a + 1, a]]
        return rp, ci
    if len(lens) and cols:                                # no row of two entries: one row becomes a pair of equal columns
        r = int(rng.integers(len(lens)))
        c = int(rng.integers(cols))
        return FP.replace_row(rp, ci, r, [c, c])
    return rp, ci


def operand_rows(rng, rows, cols, ascend):
    """rows x cols with fuzz_plans._random_b's rows; not ascending: its own mess in half the draws, one break in the rest"""
    per = int(rng.integers(1, 9))
    if ascend or rng.random() < 0.5:
        return FP._random_b(rng, rows, cols, per, ascend)
    return break_one(rng, *FP._random_b(rng, rows, cols, per, True), cols)


def same_bits_or_raise(got, want, P, what):
    got = np.asarray(got)
    need(got.shape == np.shape(want), P, what, "shape", got.shape, "for", np.shape(want))
    if not GN.same_bits(got, want):
        want = np.asarray(want, F64)
        bad = np.flatnonzero((GN.bits(got) != GN.bits(want)) & ~(np.isnan(got) & np.isnan(want)))
        need(False, P, what, "%d of %d values differ from the reference's bits, first at %s: %r for %r" % (
            len(bad), len(want), bad[:1], got[bad[:1]], want[bad[:1]]))


def gamma(K):
    return K * U / (1 - K * U)


def nan_bytes(dev, count):
    import torch
    return torch.full((count * 8,), 0xFF, dtype=torch.uint8, device=dev).view(torch.float64)


def preset(dev, count, rnd):
    """`out` before a call: NaN bytes in the first round, a finite sentinel in the second"""
    import torch
    return nan_bytes(dev, count) if rnd == 0 else torch.full((count,), SENTINEL, dtype=torch.float64, device=dev)


def dev_csr(dev, rp, ci):
    return up(dev, np.ascontiguousarray(rp, I32)), up(dev, np.ascontiguousarray(ci, I32))


# ---------------------------------------------------------------------------------------------------------------------
# mspgemm: out = M o (X Y^T)
# ---------------------------------------------------------------------------------------------------------------------
def wave_census(mrow, xlen, cap):
    """what the sorted kernel's waves meet, from the row of every mask entry and X's row lengths: waves that stage a row,
    waves whose entries name more than one row, and among those the ones whose first row is staged while a later one is
    at or above the limit (staged_then_long) and the reverse (long_then_staged)"""
    out = dict(staged_rows=0, straddled_waves=0, staged_then_long=0, long_then_staged=0)
    for t0 in range(0, len(mrow), WAVE):
        rows = mrow[t0:t0 + WAVE]
        first = rows[0]
        out["staged_rows"] += int(xlen[first] <= cap)
        if rows[-1] != first:
            out["straddled_waves"] += 1
            later = xlen[rows[rows != first]]
            if xlen[first] <= cap and (later >= cap).any():
                out["staged_then_long"] += 1
            if xlen[first] >= cap and (later <= cap).any():
                out["long_then_staged"] += 1
    return out


def matched_pairs(P, t, rnd):
    """(x values, y values) of the products of mask entry t in the contract's order: X's stored order, then Y's"""
    (rpx, cix), (rpy, ciy) = P["X"], P["Y"]
    i, j = P["mrow"][t], P["M"][1][t]
    e, g = np.nonzero(cix[rpx[i]:rpx[i + 1], None] == ciy[None, rpy[j]:rpy[j + 1]])
    return P["vx"][rnd][rpx[i] + e], P["vy"][rnd][rpy[j] + g]


def exact_sums(xs, ys):
    """(sum of x * y, sum of |x * y|) of finite doubles as Fractions, exactly: a double is an integer of 53 bits times a
    power of two, so the products are integers over one common power of two and are added as such -- what Fraction's own
    sum does, without reducing after every term (tests/test_fuzz_algebra_host.py holds it to Fraction's)"""
    (mx, ex), (my, ey) = np.frexp(xs), np.frexp(ys)
    ax, ay = np.ldexp(mx, 53).astype(I64).tolist(), np.ldexp(my, 53).astype(I64).tolist()
    e = ex.astype(I64) + ey - 106
    low = int(e.min())
    prods = [(a * b) << s for a, b, s in zip(ax, ay, (e - low).tolist())]
    unit = Fraction(2) ** low
    return sum(prods) * unit, sum(map(abs, prods)) * unit


def draw_mspgemm(case, rng, max_rows):
    lim = S.mspgemm_limits()
    cap = lim["lds_row"]
    st = FP.structure(rng, max_rows, False, dict(lds_row=cap), case)
    m, n, rpm, cim = st["rows"], st["cols"], st["rp"], st["ci"]
    x_asc, y_asc = ASCENDING_TURN[(case // 2) % 4]
    regime = REGIMES[case % 3]
    if m < 2:
        st["plant"] = None
    plant = st["plant"]
    L = plant["L"] if plant else 0
    k = int(rng.choice([1, 7, 64, cap + 40, int(rng.integers(1, 2 * cap))]))
    if plant:                                             # room for L distinct columns and for a Y row of L + 1
        k = max(k, L + 1 + int(rng.integers(0, 40)))
        n = max(n, PLANT_MASK_ROW[1])
    rpx, cix = operand_rows(rng, m, k, x_asc)
    rpy, ciy = operand_rows(rng, n, k, y_asc)
    r = None
    if plant:
        r = int(rng.integers(1, m))
        if not PLANT_MASK_ROW[0] <= rpm[r + 1] - rpm[r] <= PLANT_MASK_ROW[1]:
            rpm, cim = FP.replace_row(rpm, cim, r, FP.distinct(rng, 0, n, int(rng.integers(*PLANT_MASK_ROW))))
        # the row before is no multiple of 64 long and the planted row begins inside a wave: one of 0, 1, 2 more entries does both
        before = int(rpm[r] - rpm[r - 1])
        extra = next(x for x in range(3) if (before + x) % WAVE and (int(rpm[r]) + x) % WAVE)
        if extra:
            rpm, cim = FP.replace_row(rpm, cim, r - 1, np.concatenate([cim[rpm[r - 1]:rpm[r]], rng.integers(0, n, extra)]))
        xcols = FP.distinct(rng, 0, k, L)
        if x_asc:
            xcols = np.sort(xcols)
        elif ascending([0, L], xcols):                    # shuffled, and not by chance in order
            xcols[[0, 1]] = xcols[[1, 0]]
        rpx, cix = FP.replace_row(rpx, cix, r, xcols)
        # the Y rows the planted mask row names: lengths on both sides of the planted row's, so that xn <= yn goes both ways
        yrows = split_rows(rpy, ciy)
        named = cim[rpm[r]:rpm[r + 1]]
        named = named[np.sort(np.unique(named, return_index=True)[1])]
        for q, j in enumerate(named):
            ycols = FP.distinct(rng, 0, k, [0, 1, L - 1, L, L + 1, 3][q % 6])
            yrows[j] = np.sort(ycols) if y_asc else ycols
        rpy, ciy = join_rows(yrows)
        if not y_asc and ascending(rpy, ciy):
            rpy, ciy = break_one(rng, rpy, ciy, k)
    exact = case % 6 == 1 and rpm[-1] > 0
    if exact and rpm[-1] % lim["threads"]:                # the last non-empty row trimmed or padded to a whole workgroup
        last = int(np.flatnonzero(np.diff(rpm))[-1])
        row, over = cim[rpm[last]:rpm[last + 1]], int(rpm[-1] % lim["threads"])
        if last != r and len(row) > over and rpm[-1] > lim["threads"] and rng.random() < 0.5:
            row = row[:len(row) - over]
        else:
            row = np.concatenate([row, rng.integers(0, n, lim["threads"] - over)])
        rpm, cim = FP.replace_row(rpm, cim, last, row)
    M, X, Y = FP.csr32(rpm, cim), FP.csr32(rpx, cix), FP.csr32(rpy, ciy)
    mrow = NM.row_of_entries(rpm)
    nnz_m = len(cim)
    P = dict(st=st, m=m, n=n, k=k, M=M, X=X, Y=Y, mrow=mrow, regime=regime, planted_row=r, lim=lim,
             vx=[values(rng, len(cix), regime) for _ in range(2)], vy=[values(rng, len(ciy), regime) for _ in range(2)],
             x_ascending=ascending(rpx, cix), y_ascending=ascending(rpy, ciy), exact_fill=bool(exact and rpm[-1] % lim["threads"] == 0))
    # the sampled entries: the planted row's, then drawn ones
    own = np.arange(rpm[r], rpm[r + 1]) if plant else np.zeros(0, I64)
    rest = np.setdiff1d(np.arange(nnz_m), own)
    P["sample"] = np.concatenate([own, rng.permutation(rest)[:max(0, SAMPLE - len(own))]]).astype(I64)
    if regime == "nonfinite" and nnz_m:                   # Inf / NaN / -0.0 at matched and at unmatched columns of sampled entries
        for rnd in range(2):
            vx, vy = P["vx"][rnd], P["vy"][rnd]
            for q, t in enumerate(P["sample"][:24]):
                i, j = mrow[t], cim[t]
                xs, ys = np.arange(rpx[i], rpx[i + 1]), np.arange(rpy[j], rpy[j + 1])
                hit = np.isin(cix[xs], ciy[ys])
                pairs_x, lone_x, lone_y = xs[hit], xs[~hit], ys[~np.isin(ciy[ys], cix[xs])]
                if q % 4 == 0 and len(pairs_x):           # every product of the entry is -0.0
                    vx[pairs_x] = -0.0
                    ys_hit = ys[np.isin(ciy[ys], cix[xs])]
                    vy[ys_hit] = np.abs(np.where(np.isfinite(vy[ys_hit]), vy[ys_hit], 1.0))
                elif q % 4 == 1 and len(lone_x):
                    vx[lone_x[0]] = np.inf
                elif q % 4 == 2 and len(lone_y):
                    vy[lone_y[-1]] = (np.inf, np.nan)[q // 4 % 2]
                elif q % 4 == 3 and len(pairs_x):
                    vx[pairs_x[-1]] = (np.inf, -np.inf, np.nan)[q // 4 % 3]
    P["perm"] = dict(rows=rng.permutation(m), cols=rng.permutation(n), key=rng.random(nnz_m))
    P["params"] = FP.params_of("mspgemm", case, st, m=m, n=n, k=k, nnz_m=nnz_m, nnz_x=len(cix), nnz_y=len(ciy), regime=regime,
                               x_ascending=P["x_ascending"], y_ascending=P["y_ascending"], planted_row=r, exact_fill=P["exact_fill"])
    return P


def permuted_mspgemm(P):
    """the same product with the mask's rows reordered (X's rows with them), its columns renamed (Y's rows with them) and
    the entries of every mask row shuffled -> (M, X, Y, src_m, src_x, src_y): entry u of the new mask is entry src_m[u]"""
    p, q, key = P["perm"]["rows"], P["perm"]["cols"], P["perm"]["key"]
    (rpm, cim), (rpx, cix), (rpy, ciy) = P["M"], P["X"], P["Y"]
    new_row = np.asarray(p, I64)[P["mrow"]]
    src_m = np.lexsort((key, new_row))
    M2 = FP.csr32(rowptr_of(new_row, P["m"]), np.asarray(q, I64)[cim[src_m]] if len(cim) else cim)
    rpx2, src_x = permute_rows(rpx, p)
    rpy2, src_y = permute_rows(rpy, q)
    return M2, FP.csr32(rpx2, cix[src_x]), FP.csr32(rpy2, ciy[src_y]), src_m, src_x, src_y


def ref_mspgemm(P):
    return [S.mspgemm_ref(P["m"], P["n"], P["k"], *P["M"], *P["X"], P["vx"][rnd], *P["Y"], P["vy"][rnd]) for rnd in range(2)]


def judge_accuracy(P, out, rnd=0):
    """judge (c): every sampled entry within gamma_K sum |x||y| of the exact sum of its K products (Fraction), or, with a
    non-finite operand among them, in the IEEE class numerics.py's rule predicts -> counts of what was met"""
    seen = dict(walk_x=0, walk_y=0, walk_tie=0, nopair_entries=0, judged_classes=0)
    (rpx, _), (rpy, _) = P["X"], P["Y"]
    for t in P["sample"]:
        xn, yn = rpx[P["mrow"][t] + 1] - rpx[P["mrow"][t]], rpy[P["M"][1][t] + 1] - rpy[P["M"][1][t]]
        seen["walk_x"] += int(xn < yn)
        seen["walk_y"] += int(xn > yn)
        seen["walk_tie"] += int(xn == yn >= 1)
        xs, ys = matched_pairs(P, t, rnd)
        K = len(xs)
        if K == 0:
            seen["nopair_entries"] += 1
            need(GN.bits(out[t:t + 1])[0] == 0, P, "an entry without a pair", "entry %d is %r, not +0.0" % (t, out[t]))
            continue
        if not (np.isfinite(xs).all() and np.isfinite(ys).all()):
            with np.errstate(invalid="ignore"):
                term = NM._stand_in(xs) * NM._stand_in(ys)
            nan = np.isnan(term).any() or ((term == np.inf).any() and (term == -np.inf).any())
            want = 1 if nan else 2 if (term == np.inf).any() else 3 if (term == -np.inf).any() else 0
            need(int(NM.class_of(out[t])) == want, P, "IEEE class", "entry %d is %r, class %d wanted" % (t, out[t], want))
            seen["judged_classes"] += 1
            continue
        need(np.isfinite(out[t]), P, "accuracy", "entry %d is %r from finite operands" % (t, out[t]))
        exact, scale = exact_sums(xs, ys)
        err = abs(Fraction(float(out[t])) - exact)
        need(err <= gamma(K) * scale, P, "accuracy", "entry %d of %d pairs: error %.3g over the bound %.3g" % (
            t, K, float(err), float(gamma(K) * scale)))
    return seen


def judge_mspgemm(P, ans):
    """ans: auto, general (two rounds each), perm (the permuted problem's first round)"""
    want = FP.wanted(P, ref_mspgemm)
    for mode in ("auto", "general"):
        for rnd in range(2):
            same_bits_or_raise(ans[mode][rnd], want[rnd], P, "mspgemm / %s, values %d" % (mode, rnd))
    src = permuted_mspgemm(P)[3]
    same_bits_or_raise(ans["perm"], np.asarray(ans["auto"][0])[src], P, "mspgemm under a permutation of the mask (contract (I))")
    return judge_accuracy(P, np.asarray(ans["auto"][0], F64))


def reference_answer_mspgemm(P):
    want = FP.wanted(P, ref_mspgemm)
    return dict(auto=[w.copy() for w in want], general=[w.copy() for w in want], perm=want[0][permuted_mspgemm(P)[3]])


def census_mspgemm(P, seen, **more):
    (rpm, _), (rpx, _) = P["M"], P["X"]
    xlen = np.diff(np.asarray(rpx, I64))
    cap = P["lim"]["lds_row"]
    used = np.unique(P["mrow"])
    out = FP.census_of(P["st"], x_ascending=P["x_ascending"], y_ascending=P["y_ascending"], forced=P["x_ascending"] and P["y_ascending"],
                       regime=P["regime"], k=P["k"], mask_dups=has_duplicates(rpm, P["M"][1], P["n"]), mask_unsorted=not ascending(*P["M"]),
                       unstaged_long_rows=int((xlen[used] > cap).sum()), workgroups=-(-len(P["mrow"]) // P["lim"]["threads"]),
                       exact_fill=P["exact_fill"], **wave_census(P["mrow"], xlen, cap))
    out.update(seen)
    out.update(more)
    return out


def case_mspgemm(case, rng, dev, max_rows):
    import torch
    P = draw_mspgemm(case, rng, max_rows)
    m, n, k = P["m"], P["n"], P["k"]
    nnz_m = len(P["M"][1])
    ans, path = {}, None
    for mode, kw in (("auto", dict()), ("general", dict(general=True))):
        plan = S.MaskedSpgemmPlan(m, n, k, *dev_csr(dev, *P["M"]), *dev_csr(dev, *P["X"]), *dev_csr(dev, *P["Y"]), **kw)
        try:
            info = plan.info()
            ans[mode] = []
            for rnd in range(2):                          # new values on the same plan, every entry of a preset `out` written
                out = plan.multiply(up(dev, P["vx"][rnd]), up(dev, P["vy"][rnd]), out=preset(dev, nnz_m, rnd))
                torch.cuda.synchronize()
                ans[mode].append(out.cpu().numpy())
        finally:
            plan.destroy()
        need(info["x_ascending"] == P["x_ascending"] and info["y_ascending"] == P["y_ascending"], P, "ascending flags", mode, info)
        need(info["path"] == ("sorted" if mode == "auto" and P["x_ascending"] and P["y_ascending"] else "general"), P, "path", mode, info)
        path = info["path"] if mode == "auto" else path
    M2, X2, Y2, _, src_x, src_y = permuted_mspgemm(P)
    plan = S.MaskedSpgemmPlan(m, n, k, *dev_csr(dev, *M2), *dev_csr(dev, *X2), *dev_csr(dev, *Y2))
    try:
        ans["perm"] = plan.multiply(up(dev, P["vx"][0][src_x]), up(dev, P["vy"][0][src_y]), out=preset(dev, nnz_m, 0)).cpu().numpy()
    finally:
        plan.destroy()
    torch.cuda.synchronize()
    return census_mspgemm(P, judge_mspgemm(P, ans), path=path)


# ---------------------------------------------------------------------------------------------------------------------
# mspgemm_spgemm: masked SpGEMM on SpGEMM's pattern gives SpgemmPlan.multiply's bits
# ---------------------------------------------------------------------------------------------------------------------
def draw_mspgemm_spgemm(case, rng, max_rows):
    P = FP.draw_spgemm(case, rng, max_rows)
    P["params"] = dict(P["params"], op="mspgemm_spgemm")
    (rpb, cib) = P["B"]
    cp, ri, perm = NM.csc_of(P["k"], P["n"], rpb, cib)    # B^T as the plan's Y: every column's entries in B's stored order
    P["Y"] = FP.csr32(cp, ri)
    P["vy"] = [P["vb"][rnd][perm] for rnd in range(2)]
    return P


def ref_mspgemm_spgemm(P):
    """SpGEMM's reference, and the masked contract's on the same pattern: the identity on the host"""
    want = FP.ref_spgemm(P)
    rp, ci = want["rowptr"], want["colidx"]
    want["masked"] = [S.mspgemm_ref(P["m"], P["n"], P["k"], rp, ci, *P["A"], P["va"][rnd], *P["Y"], P["vy"][rnd]) for rnd in range(2)]
    return want


def judge_mspgemm_spgemm(P, ans):
    """ans: mode -> dict(rowptr, colidx, val, val2 of SpgemmPlan; colptr, rowidx, valT, valT2 of TransposePlan; masked: path
    -> [values, values2])"""
    want = FP.wanted(P, ref_mspgemm_spgemm)
    for rnd in range(2):
        same_bits_or_raise(want["masked"][rnd], want["val" if rnd == 0 else "val2"], P, "the identity between the references")
    for mode, got in ans.items():
        FP.judge_spgemm(P, got, want, "spgemm / " + mode)
        need_equal(got["colptr"], P["Y"][0], P, "transpose colptr / " + mode)
        need_equal(got["rowidx"], P["Y"][1], P, "transpose rowidx / " + mode)
        for rnd, (key, vkey) in enumerate((("val", "valT"), ("val2", "valT2"))):
            same_bits_or_raise(got[vkey], P["vy"][rnd], P, "transposed values / " + mode)
            for path, outs in got["masked"].items():
                same_bits_or_raise(outs[rnd], got[key], P, "masked SpGEMM (%s) against SpgemmPlan.multiply / %s, values %d" % (path, mode, rnd))
                same_bits_or_raise(outs[rnd], want[key], P, "masked SpGEMM (%s) against the reference / %s, values %d" % (path, mode, rnd))


def reference_answer_mspgemm_spgemm(P):
    want = FP.wanted(P, ref_mspgemm_spgemm)
    one = lambda: dict(rowptr=want["rowptr"], colidx=want["colidx"], val=want["val"].copy(), val2=want["val2"].copy(), colptr=P["Y"][0],
                       rowidx=P["Y"][1], valT=P["vy"][0].copy(), valT2=P["vy"][1].copy(),
                       masked=dict(auto=[want["val"].copy(), want["val2"].copy()], general=[want["val"].copy(), want["val2"].copy()]))
    return {mode: one() for mode, _ in FP.SPGEMM_MODES}


def case_mspgemm_spgemm(case, rng, dev, max_rows):
    import torch
    P = draw_mspgemm_spgemm(case, rng, max_rows)
    m, k, n = P["m"], P["k"], P["n"]
    dA, dB = dev_csr(dev, *P["A"]), dev_csr(dev, *P["B"])
    dva, dvb = [up(dev, v) for v in P["va"]], [up(dev, v) for v in P["vb"]]
    seen = dict(rows_row=0, rows_general=0, chunks=0, masked_paths=set())
    ans = {}
    for mode, kw in FP.SPGEMM_MODES:
        plans = []
        try:
            c = S.SpgemmPlan(m, k, n, *dA, *dB, **kw)
            plans.append(c)
            info = c.info()
            rpc, cic = c.csr()
            got = dict(rowptr=rpc.cpu().numpy().copy(), colidx=cic.cpu().numpy().copy(), val=c.multiply(dva[0], dvb[0]).cpu().numpy(),
                       val2=c.multiply(dva[1], dvb[1]).cpu().numpy(), masked={})
            tp = S.TransposePlan(k, n, *dB, dvb[0])
            plans.append(tp)
            colptr, rowidx, vt = tp.csc()
            got.update(colptr=colptr.cpu().numpy().copy(), rowidx=rowidx.cpu().numpy().copy(), valT=vt.cpu().numpy().copy())
            vts = [vt.clone()]
            tp.update_values(dvb[1])
            vts.append(tp.csc()[2].clone())
            got["valT2"] = vts[1].cpu().numpy()
            for name, mkw in (("auto", dict()), ("general", dict(general=True))):
                mp = S.MaskedSpgemmPlan(m, n, k, rpc, cic, *dA, colptr, rowidx, **mkw)
                plans.append(mp)
                seen["masked_paths"].add(mp.info()["path"])
                got["masked"][name] = [mp.multiply(dva[rnd], vts[rnd], out=preset(dev, c.nnz_c, rnd)).cpu().numpy() for rnd in range(2)]
            torch.cuda.synchronize()
        finally:
            for p in reversed(plans):
                p.destroy()
        ans[mode] = got
        need(mode == "auto" or info["rows_row"] == 0, P, "rows_row", mode, info)
        if mode == "auto":
            seen.update(rows_row=info["rows_row"], rows_general=info["rows_general"])
        seen["chunks"] = max(seen["chunks"], info["chunks"])
    judge_mspgemm_spgemm(P, ans)
    return FP.census_of(P["st"], **seen)


# ---------------------------------------------------------------------------------------------------------------------
# geam: C = alpha * A + beta * B
# ---------------------------------------------------------------------------------------------------------------------
def _trim_to_edge(rows, stop):
    """the entries of rows[:stop] cut from the end down to a multiple of GEAM_WG -> how many are left"""
    total = sum(len(r) for r in rows[:stop])
    cut, i = total % GEAM_WG, stop - 1
    while cut:
        take = min(cut, len(rows[i]))
        rows[i] = rows[i][:len(rows[i]) - take]
        cut, i = cut - take, i - 1
    return total - total % GEAM_WG


def draw_geam(case, rng, max_rows):
    relation = GEAM_RELATIONS[case % len(GEAM_RELATIONS)]
    st = FP.structure(rng, max_rows, relation == "transpose", dict(scan=GEAM_SCAN_TILE - 1, wg=GEAM_WG), case)
    rows, cols, rpa, cia = st["rows"], st["cols"], st["rp"], st["ci"]
    if relation == "empty" or rows < 2:                   # an empty B stays empty
        st["plant"] = None
    plant = st["plant"]
    regime = REGIMES[case % 3]
    if rng.random() < 0.6:
        rpa, cia = clean_rows(rows, cols, rpa, cia)
    b_clean = bool(rng.random() < 0.7)
    if relation in ("independent", "disjoint"):
        rpb, cib = FP._random_b(rng, rows, cols, int(rng.integers(1, 9)), b_clean)
    elif relation == "subset":
        keep = rng.random(len(cia)) < 0.5
        rpb, cib = rowptr_of(NM.row_of_entries(rpa)[keep], rows), cia[keep]
    elif relation == "same":
        rpb, cib = rpa.copy(), cia.copy()
    elif relation == "transpose":
        rpb, cib, _ = GN.transpose_csr(rows, cols, rpa, cia, np.zeros(len(cia)))
    else:
        rpb, cib = np.zeros(rows + 1, I64), np.zeros(0, I64)
    a_sorted, b_sorted = ascending(rpa, cia), ascending(rpb, cib)
    ra, rb = split_rows(rpa, cia), split_rows(rpb, cib)
    order = lambda c, keep: np.sort(c) if keep else c
    edge = False
    if plant and plant["name"] == "scan":                 # nnz(B) == L exactly: one row resized, the trailing rows emptied for room
        L, r = plant["L"], int(rng.integers(rows))
        other, i = sum(len(x) for x in rb) - len(rb[r]), rows - 1
        while other >= L:
            if i != r:
                other -= len(rb[i])
                rb[i] = rb[i][:0]
            i -= 1
        cols = max(cols, L - other)
        rb[r] = order(FP.distinct(rng, 0, cols, L - other), b_sorted)
    elif plant:                                           # row r of both: L entries behind a run of empty rows that ends on a workgroup edge
        L, r = plant["L"], int(rng.integers(max(1, rows // 2), rows))
        run = min(int(rng.integers(1, 40)), r)
        cols = max(cols, L)
        left = []
        for side, keep in ((ra, a_sorted), (rb, b_sorted)):
            for i in range(r - run, r):
                side[i] = side[i][:0]
            left.append(_trim_to_edge(side, r - run))
            side[r] = order(FP.distinct(rng, 0, cols, L), keep)
        if relation == "same":
            rb = [x.copy() for x in ra]
            left[1] = left[0]
        edge = min(left) > 0
    (rpa, cia), (rpb, cib) = join_rows(ra), join_rows(rb)
    if relation == "disjoint":
        cia, cib, cols = 2 * cia, 2 * cib + 1, 2 * cols
    A, B = FP.csr32(rpa, cia), FP.csr32(rpb, cib)
    na, nb = len(cia), len(cib)
    pairs = [(a, b) for a in AN.SCALARS for b in AN.SCALARS]
    scal = lambda: tuple(float(v) for v in NM.log_uniform(rng, 2, 6)) if rng.random() < 0.15 else pairs[int(rng.integers(len(pairs)))]
    key_a = NM.row_of_entries(rpa) * max(cols, 1) + cia
    key_b = NM.row_of_entries(rpb) * max(cols, 1) + cib
    P = dict(st=st, rows=rows, cols=cols, A=A, B=B, relation=relation, regime=regime, scalars=[scal(), scal()],
             va=[values(rng, na, regime) for _ in range(2)], vb=[values(rng, nb, regime) for _ in range(2)],
             a_ascending=ascending(rpa, cia), b_ascending=ascending(rpb, cib), matched=int(np.isin(key_b, key_a).sum()),
             empty_run_on_edge=bool(edge), perm=rng.permutation(rows))
    P["params"] = FP.params_of("geam", case, st, rows=rows, cols=cols, nnz_a=na, nnz_b=nb, relation=relation, regime=regime,
                               scalars=P["scalars"], a_ascending=P["a_ascending"], b_ascending=P["b_ascending"], matched=P["matched"])
    return P


GEAM_KEYS = ("rowptr", "colidx", "dest_a", "dest_b")


def ref_geam(P):
    out = [S.geam_ref(P["rows"], P["cols"], *P["A"], P["va"][rnd], *P["B"], P["vb"][rnd], *P["scalars"][rnd]) for rnd in range(2)]
    return dict(rowptr=out[0][0], colidx=out[0][1], dest_a=out[0][3], dest_b=out[0][4], val=out[0][2], val2=out[1][2])


def permuted_geam(P):
    """A and B with row i moved to row perm[i] -> (A, B, src_a, src_b)"""
    rpa, sa = permute_rows(P["A"][0], P["perm"])
    rpb, sb = permute_rows(P["B"][0], P["perm"])
    return FP.csr32(rpa, P["A"][1][sa]), FP.csr32(rpb, P["B"][1][sb]), sa, sb


def judge_geam(P, ans):
    """ans: modes: name -> dict(rowptr, colidx, dest_a, dest_b, val, val2); coo: (rowptr, colidx, val) of coo_to_csr(dup="sum")
    over the scaled triplets; coo_a (B empty): its values over A's triplets alone, beside one: the plan's with alpha = 1;
    perm: dict(rowptr, colidx, val) of the row-permuted pair"""
    want = FP.wanted(P, ref_geam)
    for mode, got in ans["modes"].items():
        for key in GEAM_KEYS:
            need_equal(got[key], want[key], P, "geam / %s %s" % (mode, key))
        for key in ("val", "val2"):
            same_bits_or_raise(got[key], want[key], P, "geam / %s %s" % (mode, key))
    need_equal(ans["coo"][0], want["rowptr"], P, "coo_to_csr rowptr")
    need_equal(ans["coo"][1], want["colidx"], P, "coo_to_csr colidx")
    same_bits_or_raise(ans["coo"][2], want["val"], P, "coo_to_csr(dup=sum) of the scaled triplets")
    if "coo_a" in ans:
        same_bits_or_raise(ans["one"], ans["coo_a"], P, "alpha = 1 over an empty B against coo_to_csr(dup=sum) of A")
    rp2, src = permute_rows(want["rowptr"], P["perm"])   # contract (I): C's rows go where A's and B's went, bits unchanged
    need_equal(ans["perm"]["rowptr"], rp2, P, "rowptr of the row-permuted pair")
    need_equal(ans["perm"]["colidx"], want["colidx"][src], P, "colidx of the row-permuted pair")
    same_bits_or_raise(ans["perm"]["val"], want["val"][src], P, "values of the row-permuted pair (contract (I))")


def reference_answer_geam(P):
    want = FP.wanted(P, ref_geam)
    rp2, src = permute_rows(want["rowptr"], P["perm"])
    modes = ["auto", "general"] + (["scatter"] if P["a_ascending"] and P["b_ascending"] else [])
    ans = dict(modes={mode: {k: v.copy() for k, v in want.items()} for mode in modes}, coo=(want["rowptr"], want["colidx"], want["val"].copy()),
               perm=dict(rowptr=rp2, colidx=want["colidx"][src], val=want["val"][src]))
    if len(P["B"][1]) == 0:
        one = S.geam_ref(P["rows"], P["cols"], *P["A"], P["va"][0], *P["B"], P["vb"][0], 1.0, P["scalars"][0][1])[2]
        ans.update(one=one, coo_a=one.copy())
    return ans


def census_geam(P, **more):
    na, nb = len(P["A"][1]), len(P["B"][1])
    ratio = "b_empty" if nb == 0 else "a_empty" if na == 0 else "a_16x" if na >= 16 * nb else "b_16x" if nb >= 16 * na else "alike"
    return FP.census_of(P["st"], a_ascending=P["a_ascending"], b_ascending=P["b_ascending"], relation=P["relation"], regime=P["regime"],
                        matched=P["matched"], nnz_a=na, nnz_b=nb, scan_blocks=-(-(nb + 1) // GEAM_SCAN_TILE),
                        empty_run_on_edge=P["empty_run_on_edge"], nnz_ratio=ratio,
                        scalars_zero=any(v == 0 for pair in P["scalars"] for v in pair), **more)


def case_geam(case, rng, dev, max_rows):
    import torch
    P = draw_geam(case, rng, max_rows)
    rows, cols = P["rows"], P["cols"]
    dA, dB = dev_csr(dev, *P["A"]), dev_csr(dev, *P["B"])
    dva, dvb = [up(dev, v) for v in P["va"]], [up(dev, v) for v in P["vb"]]
    sorted_path = P["a_ascending"] and P["b_ascending"]
    ans = dict(modes={})
    for mode, kw in [("auto", dict()), ("general", dict(general=True))] + ([("scatter", dict(scatter=True))] if sorted_path else []):
        plan = S.GeamPlan(rows, cols, *dA, *dB, **kw)
        try:
            info = plan.info()
            got = dict(zip(GEAM_KEYS, (t.cpu().numpy().copy() for t in plan.csr() + plan.maps())))
            for rnd, key in enumerate(("val", "val2")):   # new values and new scalars on the same plan, into a preset `out`
                got[key] = plan.add(dva[rnd], dvb[rnd], *P["scalars"][rnd], out=preset(dev, plan.nnz_c, rnd)).cpu().numpy()
            if mode == "auto" and len(P["B"][1]) == 0:
                ans["one"] = plan.add(dva[0], dvb[0], 1.0, P["scalars"][0][1], out=preset(dev, plan.nnz_c, 0)).cpu().numpy()
        finally:
            plan.destroy()
        torch.cuda.synchronize()
        ans["modes"][mode] = got
        need(info["path"] == ("general" if mode == "general" or not sorted_path else "sorted"), P, "path", mode, info)
        need(info["a_ascending"] == P["a_ascending"] and info["b_ascending"] == P["b_ascending"], P, "ascending flags", mode, info)
        need(info["path"] != "sorted" or info["matched"] == P["matched"], P, "matched", mode, info)
    # the scaled triplets, A's before B's, rounded once on the host: the same bits
    (alpha, beta), row = P["scalars"][0], np.concatenate((NM.row_of_entries(P["A"][0]), NM.row_of_entries(P["B"][0]))).astype(I32)
    with np.errstate(all="ignore"):
        val = np.concatenate((np.float64(alpha) * P["va"][0], np.float64(beta) * P["vb"][0]))
    coo = S.coo_to_csr(rows, cols, up(dev, row), up(dev, np.concatenate((P["A"][1], P["B"][1]))), up(dev, val), dup="sum")
    ans["coo"] = tuple(t.cpu().numpy() for t in coo[:3])
    if len(P["B"][1]) == 0:
        ans["coo_a"] = S.coo_to_csr(rows, cols, up(dev, row), dA[1], dva[0], dup="sum")[2].cpu().numpy()
    A2, B2, sa, sb = permuted_geam(P)
    plan = S.GeamPlan(rows, cols, *dev_csr(dev, *A2), *dev_csr(dev, *B2))
    try:
        rp, ci = plan.csr()
        ans["perm"] = dict(rowptr=rp.cpu().numpy().copy(), colidx=ci.cpu().numpy().copy(),
                           val=plan.add(up(dev, P["va"][0][sa]), up(dev, P["vb"][0][sb]), *P["scalars"][0]).cpu().numpy())
    finally:
        plan.destroy()
    torch.cuda.synchronize()
    judge_geam(P, ans)
    return census_geam(P, path="sorted" if sorted_path else "general", scatter=bool(sorted_path))


# ---------------------------------------------------------------------------------------------------------------------
# grad: SpgemmOperator.multiply and autograd.csr_add in one graph
# ---------------------------------------------------------------------------------------------------------------------
def draw_grad(case, rng, max_rows):
    cap = S.mspgemm_limits()["lds_row"]
    side = "a_column" if case % 2 else "c_row"
    st = FP.structure(rng, max_rows, False, dict(lds_row=cap), case, grow=0 if case % 2 else None)
    m, k, rpa, cia = st["rows"], st["cols"], st["rp"], st["ci"]
    dup = ("a", "b", None)[case % 3]
    needs = GRAD_NEED[(case // 2) % 3]
    general = bool((case // 3) % 2)
    if m == 0 or k == 0:
        st["plant"] = None
    plant = st["plant"]
    L = plant["L"] if plant else 0
    n = int(rng.integers(1, max_rows + 1))
    if plant and side == "c_row":
        n = max(n, L)
    rpb, cib = FP._random_b(rng, k, n, int(rng.integers(1, 9)), dup != "b")
    if dup == "a" and len(cia) > 1:
        rpa, cia = FP._damage("dups", rng, m, rpa, cia)
    if plant and side == "c_row":                         # one A row names one B row of L distinct columns: a row of C, and of dC, of L
        r, rb = int(rng.integers(m)), int(rng.integers(k))
        new = FP.distinct(rng, 0, n, L)
        rpb, cib = FP.replace_row(rpb, cib, rb, np.sort(new) if ascending(rpb, cib) else new)
        rpa, cia = FP.replace_row(rpa, cia, r, [rb])
    elif plant:                                           # one column of A in L rows: a row of A^T of L
        was, c = ascending(rpa, cia), int(rng.integers(k))
        rows = [x[x != c] for x in split_rows(rpa, cia)]
        for i in FP.distinct(rng, 0, m, L):
            rows[i] = np.sort(np.append(rows[i], c)) if was else np.append(rows[i], c)
        rpa, cia = join_rows(rows)
        if rpb[c + 1] == rpb[c]:                          # B's row c, the mask row over it, is not empty
            rpb, cib = FP.replace_row(rpb, cib, c, FP.distinct(rng, 0, n, min(n, 3)))
    A, B = FP.csr32(rpa, cia), FP.csr32(rpb, cib)
    with_add = m > 0 and n > 0
    A2 = FP.csr32(*FP._random_b(rng, m, n, int(rng.integers(1, 6)), bool(rng.random() < 0.5))) if with_add else None
    v = lambda count: NM.log_uniform(rng, count, 6)
    va, vb = [v(len(cia)), v(len(cia))], [v(len(cib)), v(len(cib))]
    rpc, cic, _ = GN.reference(m, n, *A, va[0], *B, vb[0])
    P = dict(st=st, m=m, k=k, n=n, A=A, B=B, A2=A2, C=(rpc, cic), va=va, vb=vb, general=general, need=needs, with_add=with_add,
             side=side if plant else None, scalars=[(1.0, 1.0), (0.75, -3.0), (-1.0, 0.5), tuple(float(x) for x in NM.log_uniform(rng, 2, 6))][int(rng.integers(4))])
    nnz_s = len(cic)
    if with_add:
        P["va2"] = [v(len(A2[1])), v(len(A2[1]))]
        rps, cis, _, dest_c, dest_2 = S.geam_ref(m, n, rpc, cic, np.zeros(len(cic)), *A2, P["va2"][0], 1.0, 1.0)
        P["S"] = (rps, cis, dest_c, dest_2)
        nnz_s = len(cis)
    P["w"] = [v(nnz_s), v(nnz_s)]
    P["no_pairs"] = len(cia) == 0 or len(cib) == 0 or len(cic) == 0
    P["params"] = FP.params_of("grad", case, st, m=m, k=k, n=n, nnz_a=len(cia), nnz_b=len(cib), nnz_c=len(cic), general=general, need=needs,
                               dup=dup, side=P["side"], with_add=with_add, scalars=P["scalars"], no_pairs=P["no_pairs"])
    return P


def ref_grad(P):
    """per round: vc, vs, ga, gb, ga2 as the references give them (the gradients whether asked for or not)"""
    m, k, n, A, B = P["m"], P["k"], P["n"], P["A"], P["B"]
    rpc, cic = P["C"]
    alpha, beta = P["scalars"]
    out = []
    for rnd in range(2):
        w = P["w"][rnd]
        vc = GN.reference(m, n, *A, P["va"][rnd], *B, P["vb"][rnd])[2]
        one = dict(vc=vc, vs=vc, ga2=None)
        dC = w
        if P["with_add"]:
            one["vs"] = S.geam_ref(m, n, rpc, cic, vc, *P["A2"], P["va2"][rnd], alpha, beta)[2]
            dC, one["ga2"] = np.float64(alpha) * w[P["S"][2]], np.float64(beta) * w[P["S"][3]]    # one rounding each
        one["dC"] = dC
        one["ga"] = S.mspgemm_ref(m, k, n, *A, rpc, cic, dC, *B, P["vb"][rnd])
        At, Ct = GN.transpose_csr(m, k, *A, P["va"][rnd]), GN.transpose_csr(m, n, rpc, cic, dC)
        one["gb"] = S.mspgemm_ref(k, n, m, *B, *At, *Ct)
        out.append(one)
    return out


def dense_bound_applies(P):
    """the preconditions of tests/test_gpu_spgemm_autograd.py's dense bound (2 gamma_n, 2 gamma_m; derived there): small
    enough to densify, and no row with more stored entries than the inner dimension allows"""
    m, k, n = P["m"], P["k"], P["n"]
    if min(m, k, n) == 0 or max(m * n, m * k, k * n) > DENSE_CELLS or P["no_pairs"]:
        return False
    rpc, cic = P["C"]
    At, Ct = GN.transpose_csr(m, k, *P["A"], np.zeros(len(P["A"][1]))), GN.transpose_csr(m, n, rpc, cic, np.zeros(len(cic)))
    longest = lambda rp: int(np.diff(rp).max()) if len(rp) > 1 else 0
    return max(longest(P["B"][0]), longest(Ct[0])) + 1 <= n and max(longest(At[0]), longest(rpc)) + 1 <= m


def judge_grad(P, ans):
    """ans: rounds: per round dict(vc, vc_plan, vs, ga, gb, ga2), None for a gradient not asked for; csr: the operator's
    (rowptr_c, colidx_c); plans: (grad_a_plan made, grad_b_plan made); reused: the handles stayed"""
    want = FP.wanted(P, ref_grad)
    m, k, n = P["m"], P["k"], P["n"]
    need_equal(ans["csr"][0], P["C"][0], P, "rowptr_c")
    need_equal(ans["csr"][1], P["C"][1], P, "colidx_c")
    need_a, need_b = P["need"] in ("both", "a"), P["need"] in ("both", "b")
    need(tuple(ans["plans"]) == (need_a and not P["no_pairs"], need_b and not P["no_pairs"]), P, "the gradient plans made", ans["plans"])
    need(ans["reused"], P, "the second backward made new plans")
    dense = dense_bound_applies(P)
    for rnd, (got, ref) in enumerate(zip(ans["rounds"], want)):
        same_bits_or_raise(got["vc"], ref["vc"], P, "forward against the reference, round %d" % rnd)
        same_bits_or_raise(got["vc"], got["vc_plan"], P, "forward against SpgemmPlan.multiply, round %d" % rnd)
        same_bits_or_raise(got["vs"], ref["vs"], P, "csr_add forward against geam_ref, round %d" % rnd)
        for key, asked in (("ga", need_a), ("gb", need_b), ("ga2", P["with_add"])):
            need((got[key] is not None) == asked, P, "gradient " + key, "asked for" if asked else "not asked for")
            if asked:
                same_bits_or_raise(got[key], ref[key], P, "gradient %s, round %d" % (key, rnd))
        if dense:
            rpc, cic = P["C"]
            C_ = (rpc, cic, ref["dC"])
            D = lambda r, c, M, f=(lambda x: x): GN.to_dense(r, c, M[0], M[1], f(M[2]))
            A_, B_ = P["A"] + (P["va"][rnd],), P["B"] + (P["vb"][rnd],)
            ia, ja = NM.row_of_entries(A_[0]), np.asarray(A_[1], I64)
            ib, jb = NM.row_of_entries(B_[0]), np.asarray(B_[1], I64)
            g = lambda K: float(gamma(K))
            if need_a:
                exact, bound = (D(m, n, C_) @ D(k, n, B_).T)[ia, ja], 2 * g(n) * (D(m, n, C_, np.abs) @ D(k, n, B_, np.abs).T)[ia, ja]
                need((np.abs(got["ga"] - exact) <= bound).all(), P, "gradient ga against the dense product", float(np.abs(got["ga"] - exact).max()))
            if need_b:
                exact, bound = (D(m, k, A_).T @ D(m, n, C_))[ib, jb], 2 * g(m) * (D(m, k, A_, np.abs).T @ D(m, n, C_, np.abs))[ib, jb]
                need((np.abs(got["gb"] - exact) <= bound).all(), P, "gradient gb against the dense product", float(np.abs(got["gb"] - exact).max()))
    return dict(dense=dense)


def reference_answer_grad(P):
    want = FP.wanted(P, ref_grad)
    need_a, need_b = P["need"] in ("both", "a"), P["need"] in ("both", "b")
    rounds = [dict(vc=w["vc"].copy(), vc_plan=w["vc"].copy(), vs=w["vs"].copy(), ga=w["ga"].copy() if need_a else None,
                   gb=w["gb"].copy() if need_b else None, ga2=w["ga2"].copy() if P["with_add"] else None) for w in want]
    return dict(rounds=rounds, csr=P["C"], plans=(need_a and not P["no_pairs"], need_b and not P["no_pairs"]), reused=True)


def census_grad(P, **more):
    cap = S.mspgemm_limits()["lds_row"]
    (rpa, cia), (rpb, cib), (rpc, _) = P["A"], P["B"], P["C"]
    longest_c = int(np.diff(rpc).max()) if P["m"] else 0
    longest_col_a = int(np.bincount(cia, minlength=1).max()) if len(cia) else 0
    return FP.census_of(P["st"], general=P["general"], no_pairs=P["no_pairs"], dup_a=has_duplicates(rpa, cia, P["k"]),
                        dup_b=has_duplicates(rpb, cib, P["n"]), need=P["need"], long_x_a=longest_c > cap, long_x_b=longest_col_a > cap,
                        with_add=P["with_add"], side=P["side"], **more)


def case_grad(case, rng, dev, max_rows):
    import torch
    import sblas_amd.autograd as AG
    P = draw_grad(case, rng, max_rows)
    m, k, n = P["m"], P["k"], P["n"]
    need_a, need_b = P["need"] in ("both", "a"), P["need"] in ("both", "b")
    dA, dB = dev_csr(dev, *P["A"]), dev_csr(dev, *P["B"])
    op = AG.SpgemmOperator(m, k, n, *dA, *dB, general=P["general"])
    plan = S.SpgemmPlan(m, k, n, *dA, *dB, general=P["general"])
    geam = None
    ans = dict(rounds=[], reused=True)
    try:
        rpc, cic = op.csr()
        ans["csr"] = (rpc.cpu().numpy().copy(), cic.cpu().numpy().copy())
        need_equal(ans["csr"][0], P["C"][0], P, "rowptr_c")   # the sum below is built on it
        need_equal(ans["csr"][1], P["C"][1], P, "colidx_c")
        if P["with_add"]:
            geam = S.GeamPlan(m, n, rpc, cic, *dev_csr(dev, *P["A2"]))
        kept, paths = None, {}
        for rnd in range(2):
            va, vb = up(dev, P["va"][rnd]).requires_grad_(need_a), up(dev, P["vb"][rnd]).requires_grad_(need_b)
            vc = op.multiply(va, vb)
            vs, va2 = vc, None
            if P["with_add"]:
                va2 = up(dev, P["va2"][rnd]).requires_grad_(True)
                vs = AG.csr_add(geam, vc, va2, *P["scalars"])
            (up(dev, P["w"][rnd]) * vs).sum().backward()
            torch.cuda.synchronize()
            host = lambda t: None if t is None else t.detach().cpu().numpy()
            ans["rounds"].append(dict(vc=host(vc), vc_plan=host(plan.multiply(va.detach(), vb.detach())), vs=host(vs), ga=host(va.grad),
                                      gb=host(vb.grad), ga2=host(va2.grad) if va2 is not None else None))
            made = (op.grad_a_plan, op.grad_b_plan, op.transpose_a, op.transpose_c)
            handles = tuple(p.handle.value if p is not None else None for p in made)
            if rnd == 0:
                ans["plans"] = (op.grad_a_plan is not None, op.grad_b_plan is not None)
                need((op.transpose_a is not None) == (op.grad_b_plan is not None) == (op.transpose_c is not None), P, "the transposes made", handles)
            ans["reused"] = ans["reused"] and (kept is None or handles == kept)
            kept = handles
        for name, p in (("grad_a_path", op.grad_a_plan), ("grad_b_path", op.grad_b_plan)):
            paths[name] = p.info()["path"] if p is not None else None
            need(p is None or not P["general"] or paths[name] == "general", P, name, paths[name])
    finally:
        for p in (op, plan, geam):
            if p is not None:
                p.destroy()
    torch.cuda.synchronize()
    return census_grad(P, **paths, **judge_grad(P, ans))


DRAW = dict(mspgemm=draw_mspgemm, mspgemm_spgemm=draw_mspgemm_spgemm, geam=draw_geam, grad=draw_grad)
REF = dict(mspgemm=ref_mspgemm, mspgemm_spgemm=ref_mspgemm_spgemm, geam=ref_geam, grad=ref_grad)
JUDGE = dict(mspgemm=judge_mspgemm, mspgemm_spgemm=judge_mspgemm_spgemm, geam=judge_geam, grad=judge_grad)
ANSWER = dict(mspgemm=reference_answer_mspgemm, mspgemm_spgemm=reference_answer_mspgemm_spgemm, geam=reference_answer_geam,
              grad=reference_answer_grad)
CASE = dict(mspgemm=case_mspgemm, mspgemm_spgemm=case_mspgemm_spgemm, geam=case_geam, grad=case_grad)


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
