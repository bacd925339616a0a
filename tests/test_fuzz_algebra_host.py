"""The host half of tools/fuzz_algebra.py, without a GPU: the generators of the seed that tests/test_gpu_fuzz_algebra.py
commits to are run as they are there, and

- the host half of the census holds (test_gpu_fuzz_algebra.census_*_host): families, damage, degenerate shapes, every
  (limit, relation) pair, every turn value, both kinds of straddled wave, a tie of the walk, an exact fill, one, two and
  more blocks of GEAM's scan, an empty run on a workgroup edge;
- every generated problem is accepted by its own references: the answer the references give, in the form the device run
  returns it, passes every judge -- the Fraction bound of mspgemm's judge (c) included, on every sampled entry;
- S.geam_ref / S.mspgemm_ref equal the numpy restatements of the contracts on the first draws of each operation (the
  restatement of the masked product is quadratic in the row lengths: planted rows are cut short for this check alone);
- every judge refuses a spoiled answer, and accepts the same answer with the spoiling taken out (each spoiling is a
  function of the good answer; every check runs it with `spoil=False` first and must then be accepted);
- the two constants the tool names for GEAM's kernels are the ones the sources define."""
import os
import re

import numpy as np
import pytest

import geam_numerics as AN
import mspgemm_numerics as MN
import spgemm_numerics as GN
import test_gpu_fuzz_algebra as G
from conftest import ROOT

OPS = ["mspgemm", "mspgemm_spgemm", "geam", "grad"]
RESTATED = 15
SPOILED_MSPGEMM = 30                                      # the first cases of mspgemm get the spoiled answers: every kind occurs among them
RESTATE_ROW = 40                                          # the longest row the quadratic restatement is given


@pytest.fixture(scope="module")
def fuzz(sblas):
    return G.load()


_drawn = {}


def problems(fuzz, op):
    """the committed seed's draws of `op`, made once"""
    if op not in _drawn:
        _drawn[op] = [fuzz.DRAW[op](case, fuzz.case_rng(G.SEED, op, case), G.max_rows(op)) for case in range(G.CASES)]
    return _drawn[op]


def refused(fuzz, op, P, ans):
    try:
        fuzz.JUDGE[op](P, ans)
    except AssertionError:
        return True
    return False


def ulp_up(v):
    return np.nextafter(v, np.inf) if np.isfinite(v) else 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the generated cases and their census
# ---------------------------------------------------------------------------------------------------------------------
def test_mspgemm_cases_are_accepted_and_the_host_census_holds(fuzz):
    seen = []
    cap = fuzz.S.mspgemm_limits()["lds_row"]
    offset = dict(below=cap - 1, at=cap, above=cap + 1, far=2 * cap + 3)
    for P in problems(fuzz, "mspgemm"):
        (rpm, cim), (rpx, cix), (rpy, ciy) = P["M"], P["X"], P["Y"]
        assert len(rpm) == P["m"] + 1 == len(rpx) and len(rpy) == P["n"] + 1, P["params"]
        for ci, top in ((cim, P["n"]), (cix, P["k"]), (ciy, P["k"])):
            assert len(ci) == 0 or (0 <= ci.min() and ci.max() < top), P["params"]
        if P["st"]["plant"]:                              # the planted row: its length, where it begins, what lies over it
            r, L = P["planted_row"], offset[P["st"]["plant"]["rel"]]
            assert rpx[r + 1] - rpx[r] == L == len(np.unique(cix[rpx[r]:rpx[r + 1]])), P["params"]
            assert (rpm[r] - rpm[r - 1]) % 64 and rpm[r] % 64 and rpm[r + 1] - rpm[r] >= 130, P["params"]
            assert set(np.arange(rpm[r], rpm[r + 1])) <= set(P["sample"]), P["params"]
            named = np.diff(rpy)[np.unique(cim[rpm[r]:rpm[r + 1]])]
            assert {0, 1, 3, L - 1, L, L + 1} <= set(named), P["params"]
        if P["exact_fill"]:
            assert rpm[-1] > 0 and rpm[-1] % P["lim"]["threads"] == 0
        assert len(P["sample"]) <= max(fuzz.SAMPLE, 0 if P["planted_row"] is None else rpm[P["planted_row"] + 1] - rpm[P["planted_row"]])
        walks = fuzz.judge_mspgemm(P, fuzz.reference_answer_mspgemm(P))      # the Fraction bound on the reference's own output
        seen.append(fuzz.census_mspgemm(P, walks))
    G.census_mspgemm_host(fuzz, seen)
    G.census_mspgemm_walks(seen)


def test_the_exact_sums_are_those_of_fraction_arithmetic(fuzz):
    from fractions import Fraction
    rng = np.random.default_rng(77)
    for count, binades in ((1, 6), (3, 6), (40, 6), (300, 6), (25, 1800)):
        xs, ys = fuzz.NM.log_uniform(rng, count, binades), fuzz.NM.log_uniform(rng, count, binades)
        xs[0] = 5e-324 if binades > 6 else xs[0]
        ys[-1] = -0.0 if count > 1 else ys[-1]
        prods = [Fraction(float(x)) * Fraction(float(y)) for x, y in zip(xs, ys)]
        assert fuzz.exact_sums(xs, ys) == (sum(prods), sum(abs(p) for p in prods))


def test_mspgemm_spgemm_cases_are_accepted(fuzz):
    for P in problems(fuzz, "mspgemm_spgemm"):
        fuzz.judge_mspgemm_spgemm(P, fuzz.reference_answer_mspgemm_spgemm(P))   # the identity holds between the references
    seen = [fuzz.FP.census_of(P["st"]) for P in problems(fuzz, "mspgemm_spgemm")]
    G.census(fuzz, seen, ("acc_cap", "s_max"))


def test_geam_cases_are_accepted_and_the_host_census_holds(fuzz):
    seen = []
    for P in problems(fuzz, "geam"):
        (rpa, cia), (rpb, cib) = P["A"], P["B"]
        assert len(rpa) == P["rows"] + 1 == len(rpb), P["params"]
        for ci in (cia, cib):
            assert len(ci) == 0 or (0 <= ci.min() and ci.max() < P["cols"]), P["params"]
        plant = P["st"]["plant"]
        if plant and plant["name"] == "scan":
            assert len(cib) == plant["L"], P["params"]
        if plant and plant["name"] == "wg":
            assert plant["L"] in np.diff(rpa) and plant["L"] in np.diff(rpb), P["params"]
        if P["relation"] == "empty":
            assert len(cib) == 0
        if P["relation"] == "disjoint":
            assert P["matched"] == 0
        fuzz.judge_geam(P, fuzz.reference_answer_geam(P))
        seen.append(fuzz.census_geam(P))
    G.census_geam_host(fuzz, seen)


def test_grad_cases_are_accepted_and_the_host_census_holds(fuzz):
    seen = []
    for P in problems(fuzz, "grad"):
        extra = fuzz.judge_grad(P, fuzz.reference_answer_grad(P))
        seen.append(fuzz.census_grad(P, **extra))
        if P["no_pairs"]:                                 # every gradient of the product is the empty sum, of the right length
            for w in fuzz.FP.wanted(P, fuzz.ref_grad):
                assert len(w["ga"]) == len(P["A"][1]) and len(w["gb"]) == len(P["B"][1])
                assert not GN.bits(w["ga"]).any() and not GN.bits(w["gb"]).any()
    G.census_grad_host(fuzz, seen)
    assert any(s["dense"] for s in seen)


# ---------------------------------------------------------------------------------------------------------------------
# the library's scalar references against the numpy restatements
# ---------------------------------------------------------------------------------------------------------------------
def cut_rows(rp, ci, vals, longest=RESTATE_ROW):
    """the CSR with every row cut to its first `longest` entries"""
    keep = np.arange(len(ci)) - np.repeat(np.asarray(rp, np.int64)[:-1], np.diff(rp)) < longest
    rp2 = np.concatenate([[0], np.cumsum(np.minimum(np.diff(rp), longest))]).astype(np.int32)
    return (rp2, ci[keep]) + tuple(v[keep] for v in vals)


def test_the_references_equal_the_restatements_on_the_first_draws(fuzz):
    S = fuzz.S
    for P in problems(fuzz, "mspgemm")[:RESTATED]:
        M = cut_rows(*P["M"], ())
        X = cut_rows(*P["X"], (P["vx"][0],))
        Y = cut_rows(*P["Y"], (P["vy"][0],))
        assert GN.same_bits(S.mspgemm_ref(P["m"], P["n"], P["k"], *M, *X, *Y), MN.restate(M, X, Y)), P["params"]
    for P in problems(fuzz, "geam")[:RESTATED]:
        A, B = P["A"] + (P["va"][0],), P["B"] + (P["vb"][0],)
        got = S.geam_ref(P["rows"], P["cols"], *A, *B, *P["scalars"][0])
        want = AN.restate(P["rows"], A, B, *P["scalars"][0])
        for g, w in zip((got[0], got[1], got[3], got[4]), (want[0], want[1], want[3], want[4])):
            assert np.array_equal(g, w), P["params"]
        assert GN.same_bits(got[2], want[2]), P["params"]
    for P in problems(fuzz, "grad")[:RESTATED]:           # the gradient of A's values, on the operands autograd.py names
        rpc, cic = P["C"]
        dC = fuzz.FP.wanted(P, fuzz.ref_grad)[0]["dC"]
        M, X, Y = cut_rows(*P["A"], ()), cut_rows(rpc, cic, (dC,)), cut_rows(*P["B"], (P["vb"][0],))
        assert GN.same_bits(S.mspgemm_ref(P["m"], P["k"], P["n"], *M, *X, *Y), MN.restate(M, X, Y)), P["params"]


# ---------------------------------------------------------------------------------------------------------------------
# spoiled answers
# ---------------------------------------------------------------------------------------------------------------------
def check_spoiled(fuzz, op, P, make, what, tally):
    """make(ans, spoil) edits the reference's answer in place; False: it does not apply to this case.  With spoil=False it
    makes every step but the spoiling and must be accepted; with spoil=True it must be refused."""
    for spoil in (False, True):
        ans = fuzz.ANSWER[op](P)
        if make(ans, spoil) is False:
            return
        assert refused(fuzz, op, P, ans) == spoil, "%s: a spoiled answer is accepted, or a good one refused (spoil=%s): %s" % (what, spoil, P["params"])
    tally[what] = tally.get(what, 0) + 1


def pairs_of(fuzz, P, t):
    return fuzz.matched_pairs(P, t, 0)


def mspgemm_spoilings(fuzz, P):
    want = fuzz.FP.wanted(P, fuzz.ref_mspgemm)[0]
    counts = {int(t): len(pairs_of(fuzz, P, t)[0]) for t in P["sample"]}
    finite = [t for t, K in counts.items() if K and np.isfinite(want[t])]

    def put(t, value, modes=("auto", "general")):
        def make(ans, spoil):
            if spoil:
                for mode in modes:
                    ans[mode][0][t] = value(ans[mode][0][t]) if callable(value) else value
        return make

    if finite:
        yield "ulp", put(finite[0], ulp_up)
        yield "ulp / general", put(finite[-1], ulp_up, ("general",))      # the mode the accuracy bound does not look at: the bits tell
    three = [t for t in finite if counts[t] == 3 and P["regime"] == "log_uniform"]
    for t in three:                                       # (p1 + p2) + p3 against p1 + (p2 + p3)
        xs, ys = pairs_of(fuzz, P, t)
        p = xs * ys
        other = p[0] + (p[1] + p[2])
        if other != want[t]:
            yield "order", put(t, other)
            break
    long_ = [t for t in finite if counts[t] >= 100 and P["regime"] != "nonfinite"]
    if long_:                                             # the last pair of a long row dropped
        t = long_[0]
        xs, ys = pairs_of(fuzz, P, t)
        acc = xs[0] * ys[0]
        for x, y in zip(xs[1:-1], ys[1:-1]):
            acc = acc + x * y
        if acc != want[t]:
            yield "dropped", put(t, acc)
    if P["regime"] == "nonfinite":
        (rpx, _), (rpy, _) = P["X"], P["Y"]
        for t in finite:                                  # an Inf at an unmatched column of the entry's rows leaks in
            i, j = P["mrow"][t], P["M"][1][t]
            if np.isinf(P["vx"][0][rpx[i]:rpx[i + 1]]).any() or np.isinf(P["vy"][0][rpy[j]:rpy[j + 1]]).any():
                yield "leak", put(t, np.inf)
                break
        minus = [t for t in counts if GN.bits(want[t:t + 1])[0] == GN.bits(np.array([-0.0]))[0]]
        if minus:
            yield "minus_zero", put(minus[0], 0.0)
    if len(want):
        ok = np.flatnonzero(~np.isnan(want))
        if len(ok):
            yield "unwritten", put(int(ok[len(ok) // 2]), np.nan)
    src = fuzz.permuted_mspgemm(P)[3]
    movable = np.flatnonzero(np.isfinite(want[src]))
    if len(movable):
        def make(ans, spoil, u=int(movable[0])):
            if spoil:
                ans["perm"][u] = ulp_up(ans["perm"][u])
        yield "permuted", make


def test_mspgemm_judges_refuse_spoiled_answers(fuzz):
    tally = {}
    for P in problems(fuzz, "mspgemm")[:SPOILED_MSPGEMM]:
        for what, make in mspgemm_spoilings(fuzz, P):
            check_spoiled(fuzz, "mspgemm", P, make, what, tally)
    for what in ("ulp", "ulp / general", "order", "dropped", "leak", "minus_zero", "unwritten", "permuted"):
        assert tally.get(what, 0) >= 2, (what, tally)
    # a fused product: the contract's bits on the pairs mspgemm_numerics found, and the bits of either contraction
    for q, (x1, y1, x2, y2) in enumerate(MN.FMA_CASES):
        m, n, k, M, X, Y = MN.fma_case(q)
        want = fuzz.S.mspgemm_ref(m, n, k, *M, *X, *Y)
        for fused in (MN.fma(x2, y2, x1 * y1), MN.fma(x1, y1, x2 * y2)):
            assert fused != want[0] and not GN.same_bits(np.array([fused]), want)
        P = dict(m=m, n=n, k=k, M=M, X=X[:2], Y=Y[:2], vx=[X[2]] * 2, vy=[Y[2]] * 2, mrow=np.zeros(1, np.int64), sample=np.zeros(1, np.int64),
                 perm=dict(rows=np.zeros(1, np.int64), cols=np.zeros(1, np.int64), key=np.zeros(1)), params="fma %d" % q)
        good = fuzz.reference_answer_mspgemm(P)
        fuzz.judge_mspgemm(P, good)
        good["auto"][0][0] = MN.fma(x2, y2, x1 * y1)
        good["general"][0][0] = MN.fma(x2, y2, x1 * y1)
        good["perm"][0] = MN.fma(x2, y2, x1 * y1)
        assert refused(fuzz, "mspgemm", P, good)


def test_mspgemm_spgemm_judge_refuses_spoiled_answers(fuzz):
    tally = {}
    for P in problems(fuzz, "mspgemm_spgemm")[::3]:
        want = fuzz.FP.wanted(P, fuzz.ref_mspgemm_spgemm)
        if len(want["val"]) < 2:
            continue
        t = len(want["val"]) // 2

        def ulp(ans, spoil):
            if spoil:
                ans["chunks"]["masked"]["auto"][1][t] = ulp_up(ans["chunks"]["masked"]["auto"][1][t])

        def both(ans, spoil):                             # SpGEMM and the masked product wrong together: the reference still tells
            if spoil:
                ans["general"]["val"][t] = ans["general"]["masked"]["auto"][0][t] = ans["general"]["masked"]["general"][0][t] = ulp_up(want["val"][t])

        def swap(ans, spoil):
            pair = np.flatnonzero(np.diff(want["rowptr"]) >= 2)
            if len(pair) == 0:
                return False
            a = want["rowptr"][pair[0]]
            if spoil:
                ans["auto"]["colidx"] = want["colidx"].copy()
                ans["auto"]["colidx"][[a, a + 1]] = want["colidx"][[a + 1, a]]

        for what, make in (("ulp", ulp), ("both", both), ("swap", swap)):
            check_spoiled(fuzz, "mspgemm_spgemm", P, make, what, tally)
    for what in ("ulp", "both", "swap"):
        assert tally.get(what, 0) >= 3, (what, tally)


def geam_spoilings(fuzz, P):
    want = fuzz.FP.wanted(P, fuzz.ref_geam)
    val = want["val"]
    finite = np.flatnonzero(np.isfinite(val))
    modes = ["auto", "general"] + (["scatter"] if P["a_ascending"] and P["b_ascending"] else [])

    def put(mode, key, t, value):
        def make(ans, spoil):
            if spoil:
                ans["modes"][mode][key][t] = value(ans["modes"][mode][key][t]) if callable(value) else value
        return make

    for q, mode in enumerate(modes):
        if len(finite) > q:
            yield "ulp / " + mode, put(mode, "val2" if q == 1 and np.isfinite(want["val2"][finite[q]]) else "val", int(finite[q]), ulp_up)
    not_nan = np.flatnonzero(~np.isnan(val))
    if len(not_nan):
        yield "unwritten", put("auto", "val", int(not_nan[-1]), np.nan)
    minus = np.flatnonzero(GN.bits(val) == GN.bits(np.array([-0.0]))[0])
    if len(minus):
        yield "minus_zero", put(modes[-1], "val", int(minus[0]), 0.0)
    nb = len(P["B"][1])
    if nb:
        yield "dest_b", put("auto", "dest_b", nb // 2, lambda d: d + 1)
    pair = np.flatnonzero(np.diff(want["rowptr"]) >= 2)
    if len(pair):
        a = int(want["rowptr"][pair[len(pair) // 2]])

        def swap(ans, spoil):
            if spoil:
                ans["modes"]["general"]["colidx"][[a, a + 1]] = want["colidx"][[a + 1, a]]
        yield "colidx_c", swap
    if len(finite):
        def coo(ans, spoil, t=int(finite[0])):
            if spoil:
                ans["coo"][2][t] = ulp_up(ans["coo"][2][t])
        yield "coo", coo

        def perm(ans, spoil, t=int(finite[-1])):
            src = fuzz.permute_rows(want["rowptr"], P["perm"])[1]
            u = int(np.flatnonzero(src == t)[0])
            if spoil:
                ans["perm"]["val"][u] = ulp_up(ans["perm"]["val"][u])
        yield "row_permuted", perm
    if nb == 0 and len(finite):
        def one(ans, spoil, t=int(finite[0])):
            if spoil:
                ans["one"][t] = ulp_up(ans["one"][t])
        yield "empty_b", one


def test_geam_judge_refuses_spoiled_answers(fuzz):
    tally = {}
    for P in problems(fuzz, "geam"):
        for what, make in geam_spoilings(fuzz, P):
            check_spoiled(fuzz, "geam", P, make, what, tally)
    for what in ("ulp / auto", "ulp / general", "ulp / scatter", "unwritten", "minus_zero", "dest_b", "colidx_c", "coo", "row_permuted", "empty_b"):
        assert tally.get(what, 0) >= 2, (what, tally)
    # a fused product: geam_numerics' pair, on which either contraction changes the bits
    A, B = AN.csr_of_rows([([0], [AN.FMA_A])]), AN.csr_of_rows([([0], [AN.FMA_B])])
    want = fuzz.S.geam_ref(1, 1, *A, *B, AN.FMA_ALPHA, AN.FMA_BETA)[2]
    assert GN.bits(want)[0] == 0
    for fused in (MN.fma(AN.FMA_ALPHA, AN.FMA_A, AN.FMA_BETA * AN.FMA_B), MN.fma(AN.FMA_BETA, AN.FMA_B, AN.FMA_ALPHA * AN.FMA_A)):
        assert not GN.same_bits(np.array([fused]), want)
        P = dict(rows=1, cols=1, A=A[:2], B=B[:2], va=[A[2]] * 2, vb=[B[2]] * 2, scalars=[(AN.FMA_ALPHA, AN.FMA_BETA)] * 2,
                 perm=np.zeros(1, np.int64), a_ascending=True, b_ascending=True, params="fma")
        good = fuzz.reference_answer_geam(P)
        fuzz.judge_geam(P, good)
        good["modes"]["auto"]["val"][0] = fused
        assert refused(fuzz, "geam", P, good)


def grad_spoilings(fuzz, P):
    want = fuzz.FP.wanted(P, fuzz.ref_grad)
    need_a, need_b = P["need"] in ("both", "a"), P["need"] in ("both", "b")

    def put(rnd, key, t, value):
        def make(ans, spoil):
            if spoil:
                ans["rounds"][rnd][key][t] = value(ans["rounds"][rnd][key][t]) if callable(value) else value
        return make

    for key, asked in (("ga", need_a), ("gb", need_b), ("ga2", P["with_add"]), ("vs", True), ("vc", True)):
        if asked and len(want[1][key]):
            yield "ulp / " + key, put(1, key, len(want[1][key]) // 2, ulp_up)
    if need_a and not P["no_pairs"]:
        (rpa, cia) = P["A"]
        key = fuzz.NM.row_of_entries(rpa) * max(P["k"], 1) + cia
        _, first, count = np.unique(key, return_index=True, return_counts=True)
        twice = [int(f) for f, c in zip(first, count) if c > 1 and want[0]["ga"][f] != 0]
        if twice:                                         # a duplicated entry's gradient shared out instead of given whole
            yield "split", put(0, "ga", twice[0], lambda g: g / 2)

    def not_formed(ans, spoil):
        if P["no_pairs"]:
            return False
        if spoil:
            ans["plans"] = (True, True) if P["need"] != "both" else (True, False)
    yield "plans", not_formed

    def remade(ans, spoil):
        if spoil:
            ans["reused"] = False
    yield "reused", remade

    def unasked(ans, spoil):
        if P["need"] == "both":
            return False
        if spoil:
            key = "gb" if P["need"] == "a" else "ga"
            ans["rounds"][0][key] = want[0][key].copy()
    yield "unasked", unasked


def test_grad_judge_refuses_spoiled_answers(fuzz):
    tally = {}
    for P in problems(fuzz, "grad")[::2] + problems(fuzz, "grad")[1::6]:
        for what, make in grad_spoilings(fuzz, P):
            check_spoiled(fuzz, "grad", P, make, what, tally)
    for what in ("ulp / ga", "ulp / gb", "ulp / ga2", "ulp / vs", "ulp / vc", "split", "plans", "reused", "unasked"):
        assert tally.get(what, 0) >= 2, (what, tally)


# ---------------------------------------------------------------------------------------------------------------------
# the tool itself
# ---------------------------------------------------------------------------------------------------------------------
def test_case_k_is_a_function_of_seed_operation_and_k_alone(fuzz):
    for op in OPS:
        first = problems(fuzz, op)[3]["params"]
        again = fuzz.DRAW[op](3, fuzz.case_rng(G.SEED, op, 3), G.max_rows(op))["params"]
        assert again == first
        other = fuzz.DRAW[op](4, fuzz.case_rng(G.SEED + 1, op, 4), G.max_rows(op))["params"]
        assert other != problems(fuzz, op)[4]["params"]


def test_the_tool_names_the_constants_the_kernels_are_built_on(fuzz):
    def constant(path, pattern):
        with open(os.path.join(ROOT, "s-blas_amd", "csrc", path)) as f:
            found = re.search(pattern, f.read())
        assert found, (path, pattern)
        return found

    assert int(constant("geam.h", r"constexpr int GEAM_THREADS = (\d+);").group(1)) == fuzz.GEAM_WG
    threads = int(constant("radix_sort.h", r"constexpr int T_THREADS = (\d+);").group(1))
    items = int(constant("radix_sort.h", r"constexpr int SCAN_ITEMS = (\d+);").group(1))
    constant("radix_sort.h", r"constexpr int64_t SCAN_TILE = T_THREADS \* SCAN_ITEMS;")
    assert threads * items == fuzz.GEAM_SCAN_TILE
    assert fuzz.S.mspgemm_limits()["threads"] == 4 * fuzz.WAVE
    assert fuzz.FP is not None and fuzz.FAMILIES is fuzz.FP.FAMILIES and fuzz.DAMAGE is fuzz.FP.DAMAGE    # imported, not copied
