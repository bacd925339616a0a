"""The host half of tools/fuzz_plans.py, without a GPU: the generators of the seed that tests/test_gpu_fuzz_plans.py
commits to are run as they are there, and

- the host half of the census holds: every family, damage kind and degenerate shape occurs, and the planted row is in the
  generated structure with exactly the drawn length, below, at, above and far above every limit (the limits come from the
  library's *_limits() calls, which need no device);
- every generated problem is accepted by its reference: the references run on it and their answer passes the judge, the
  ILU(0) structure check (the library's host rule against ilu0_numerics.check) passes on the sound structure and names
  the numpy check's row on the damaged one, and the dominant values factor finitely;
- every judge refuses a spoiled answer: the reference's with one value moved by one ulp or two neighbouring values
  swapped (the bit-exact outputs), one index changed (the integer outputs), an error of twice the bound planted in one
  entry (the bounded outputs).  This is what shows that the GPU loop would notice a subtly wrong kernel."""
import numpy as np
import pytest

import test_gpu_fuzz_plans as G

SPOILED_EVERY = 6            # the spoiled answers are tried on every sixth case: the judges cost what the references cost

# per operation: the answer's outputs by the way they are judged (a path is a key, or a tuple of nested keys)
BITS = dict(transpose=["valT"], coo=[("sum", "val"), ("keep", "val"), ("plan", "val2")], spgemm=["val", "val2"],
            attention=["P", "dS"], sptrsv=["grid_x"], ilu0=["lu", "lu2"], color=["val_b", "round_trip"],
            pipeline=["val", "val_b", "lu", "rhs_b", "y", "x_fresh"])
INDEX = dict(transpose=["colptr", "rowidx", "perm"], coo=[("keep", "colidx"), ("sum", "runptr"), ("plan", "perm"), ("sum", "rowptr")],
             spgemm=["rowptr", "colidx"], color=["color", "perm", "color_ptr", "colidx_b", "src"],
             pipeline=["colidx", "perm", "colidx_b"])
BOUNDED = dict(transpose=["y", "C"], sddmm=["out"], sptrsv=["x"])


@pytest.fixture(scope="module")
def fuzz(sblas):
    return G.load()


def problems(fuzz, op):
    for case in range(G.PIPELINE_CASES if op == "pipeline" else G.CASES):
        yield case, fuzz.DRAW[op](case, fuzz.case_rng(G.SEED, op, case), G.max_rows(op))


def at(ans, path):
    for key in (path if isinstance(path, tuple) else (path,)):
        ans = ans[key]
    return ans


def with_(ans, path, value):
    """a copy of the answer with one output replaced"""
    path = path if isinstance(path, tuple) else (path,)
    out = dict(ans)
    if len(path) == 1:
        out[path[0]] = value
    else:
        out[path[0]] = with_(ans[path[0]], path[1:], value)
    return out


def refused(fuzz, op, P, ans):
    try:
        fuzz.JUDGE[op](P, ans)
    except AssertionError:
        return True
    return False


def one_ulp(a):
    a = np.array(a, np.float64)
    live = np.flatnonzero(np.isfinite(a.reshape(-1)))
    if len(live) == 0:
        return None
    i = live[len(live) // 2]
    a.reshape(-1)[i] = np.nextafter(a.reshape(-1)[i], np.inf)
    return a


def neighbours_swapped(a):
    a = np.array(a)
    flat = a.reshape(-1)
    differ = np.flatnonzero(flat[1:] != flat[:-1])
    if len(differ) == 0:
        return None
    i = differ[len(differ) // 2]
    flat[[i, i + 1]] = flat[[i + 1, i]]
    return a


def one_changed(a):
    a = np.array(a)
    if a.size == 0:
        return None
    a.reshape(-1)[a.size // 2] += 1
    return a


def twice_the_bound(a, bound):
    a, bound = np.array(a, np.float64), np.asarray(bound, np.float64)
    if a.size == 0 or not (bound > 0).any():
        return None
    i = int(np.argmax(bound))
    a.reshape(-1)[i] += 2.0 * bound.reshape(-1)[i]
    return a


def spoiled_answers(fuzz, op, P, ans):
    """(what, answer) for every way of spoiling that applies to this case"""
    if op == "sddmm" and P["nonfinite"]:                  # judged by IEEE class: a finite entry turned into a NaN
        live = np.flatnonzero(np.isfinite(ans["out"]))
        if len(live):
            bad = ans["out"].copy()
            bad[live[0]] = np.nan
            yield "class", with_(ans, "out", bad)
        return
    for path in BITS.get(op, []):
        for what, spoil in (("ulp", one_ulp), ("swap", neighbours_swapped)):
            bad = spoil(at(ans, path))
            if bad is not None:
                yield what, with_(ans, path, bad)
    for path in INDEX.get(op, []):
        bad = one_changed(at(ans, path))
        if bad is not None:
            yield "index", with_(ans, path, bad)
    for path in BOUNDED.get(op, []):
        bad = twice_the_bound(at(ans, path), ans["_bound"][path])
        if bad is not None:
            yield "bound", with_(ans, path, bad)
    if op == "softmax":
        yield from spoiled_softmax(fuzz, P, ans)
    if op == "attention":
        yield from spoiled_attention(fuzz, P, ans)


def spoiled_softmax(fuzz, P, ans):
    """twice each of the two bars, in one entry: the Decimal bound on a sampled row, numpy's allclose on any row"""
    XN = fuzz.XN
    rp, tol = P["rp"], fuzz.SOFTMAX_ALLCLOSE
    rows = [r for r in P["sample"] if rp[r + 1] > rp[r]]
    if not rows:
        return
    r = rows[-1]
    if not P["nonfinite"]:
        (p, d), = XN.forward_reference(rp, P["x"], P["scale"], [r]).values()
        rel, _ = XN.forward_bound_row(p, d)
        bad = ans["out"].copy()
        bad[rp[r]] += 2.0 * float(p[0]) * rel[0]
        yield "bound", with_(ans, "out", bad)
        i = int(np.argmax(ans["out"]))
        bad = ans["out"].copy()
        bad[i] += 2.0 * (tol["atol"] + tol["rtol"] * abs(bad[i]))
        yield "bound", with_(ans, "out", bad)
    i = int(np.argmax(np.abs(ans["dx"])))
    bad = ans["dx"].copy()
    bad[i] += 2.0 * (tol["atol"] + tol["rtol"] * abs(bad[i]))
    yield "bound", with_(ans, "dx", bad)


def spoiled_attention(fuzz, P, ans):
    AN = fuzz.AN
    rp, ci = P["rp"].astype(np.int64), P["ci"].astype(np.int64)
    rows = [r for r in P["sample"] if rp[r + 1] > rp[r]]
    if not rows:
        return
    r = rows[-1]
    lo, hi = rp[r], rp[r + 1]
    for key, w, Y in (("O", ans["P"], P["V"]), ("dQ", ans["dS"], P["K"])):
        _, mag = AN.exact_weighted_sum(w[lo:hi], Y[ci[lo:hi]])
        bound = float(AN.bound_factor(int(hi - lo)) * mag[0] + (hi - lo + 2) * AN.ETA)
        if bound > 0:
            bad = ans[key].copy()
            bad[r, 0] += 2.0 * bound
            yield "bound", with_(ans, key, bad)


def planted_lengths(fuzz, op, P):
    """the lengths among which the planted one must be, read off the generated structure"""
    if op == "transpose":
        return np.diff(P["csc"][0])
    if op == "coo":
        return np.diff(fuzz.REF[op](P)["sum"]["runptr"])
    if op == "spgemm":
        (rpa, cia), (rpb, cib) = P["A"], P["B"]
        if P["st"]["plant"]["name"] == "acc_cap":
            return np.diff(fuzz.wanted(P, fuzz.REF[op])["rowptr"])            # the entries of C's rows
        rpa, rpb = rpa.astype(np.int64), rpb.astype(np.int64)
        spans = []
        for i in range(P["m"]):                                                # the column span of a row's B rows, as the header words it
            named = [k for k in cia[rpa[i]:rpa[i + 1]] if rpb[k + 1] > rpb[k]]
            if named:
                spans.append(max(cib[rpb[k]:rpb[k + 1]].max() for k in named) - min(cib[rpb[k]:rpb[k + 1]].min() for k in named) + 1)
        return np.array(spans)
    if op == "color":
        return fuzz.CN.degrees(P["n"], P["rp"], P["ci"])
    return np.diff(P["rp"].astype(np.int64))


LIMITS = dict(transpose=("spmv_split", "spmm_split"), coo=("run",), spgemm=("acc_cap", "s_max"), sddmm=(), softmax=("workspace",),
              attention=("workspace",), sptrsv=("g4_max", "g16_max"), ilu0=("g4_max", "g16_max", "lds_max"),
              color=("g4_max", "g16_max", "window"))


def limit_values(fuzz, op):
    S = fuzz.S
    return dict(transpose=dict(spmv_split=S.SPMV_SPLIT_MIN, spmm_split=S.SPMM_SPLIT_MIN), coo=dict(run=fuzz.COO_RUN),
                spgemm=S.spgemm_limits(), softmax=dict(workspace=fuzz.softmax_limit()), attention=dict(workspace=fuzz.attention_limit()),
                sptrsv=S.sptrsv_limits(), ilu0=S.ilu0_limits(), color=S.color_limits()).get(op, {})


@pytest.mark.parametrize("op", ["transpose", "coo", "spgemm", "sddmm", "softmax", "attention", "sptrsv", "ilu0", "color"])
def test_generated_cases_are_accepted_and_spoiled_answers_refused(fuzz, op):
    seen, spoiled = [], {}
    values = limit_values(fuzz, op)
    offset = dict(below=lambda v: v - 1, at=lambda v: v, above=lambda v: v + 1, far=lambda v: 2 * v + 3)
    for case, P in problems(fuzz, op):
        st = P["st"]
        if st["plant"]:                                                      # the planted row is there, with exactly the drawn length
            want = offset[st["plant"]["rel"]](values[st["plant"]["name"]])
            assert st["plant"]["L"] == want
            assert want in planted_lengths(fuzz, op, P), P["params"]
        ans = fuzz.REF[op](P)
        fuzz.JUDGE[op](P, ans)                                               # raises with the parameters when the reference refuses
        if op == "ilu0":
            fuzz.judge_ilu0_structure(P)
            assert np.isfinite(P["val"][0]).all() and np.isfinite(ans["lu"]).all() and np.isfinite(ans["lu2"]).all(), P["params"]
        if op == "sptrsv":
            assert np.isfinite(P["val"]).all() and np.isfinite(ans["x"]).all(), P["params"]
        seen.append(fuzz.census_of(st))
        if case % SPOILED_EVERY == 0 or st["degenerate"] is None and case % SPOILED_EVERY == 1 or P.get("nonfinite"):
            for what, bad in spoiled_answers(fuzz, op, P, ans):
                assert refused(fuzz, op, P, bad), "a spoiled answer (%s) is accepted: %s" % (what, P["params"])
                spoiled[what] = spoiled.get(what, 0) + 1
    G.census(fuzz, seen, LIMITS[op])
    kinds = (["ulp", "swap"] if op in BITS else []) + (["index"] if op in INDEX else []) + \
            (["bound"] if op in BOUNDED or op in ("softmax", "attention") else []) + (["class"] if op == "sddmm" else [])
    for what in kinds:
        assert spoiled.get(what, 0) >= 3, (what, spoiled)


def test_pipeline_cases_are_accepted_and_spoiled_answers_refused(fuzz):
    spoiled = {}
    families = set()
    for case, P in problems(fuzz, "pipeline"):
        ans = fuzz.REF["pipeline"](P)
        fuzz.JUDGE["pipeline"](P, ans)
        families.add(P["st"]["family"])
        for what, bad in spoiled_answers(fuzz, "pipeline", P, ans):
            assert refused(fuzz, "pipeline", P, bad), "a spoiled answer (%s) is accepted: %s" % (what, P["params"])
            spoiled[what] = spoiled.get(what, 0) + 1
        x = ans["x"].copy()                                                  # the solves' bar: twice the residual bound of U's first row
        n, rpb, cib, lu = P["n"], ans["rowptr_b"], ans["colidx_b"], ans["lu"]
        _, bnd = fuzz.TN.residual_bound(n, rpb, cib, lu, ans["y"], x, False, False)
        x[0] += 2.0 * bnd[0] / abs(lu[rpb[0]:rpb[1]][cib[rpb[0]:rpb[1]] == 0][0])
        assert refused(fuzz, "pipeline", P, with_(ans, "x", x)), P["params"]
    assert families == {"grid5", "near_diagonal"}
    assert min(spoiled.get(k, 0) for k in ("ulp", "swap", "index")) >= G.PIPELINE_CASES


def test_case_k_is_a_function_of_seed_operation_and_k_alone(fuzz):
    """what `--op X --seed S --only K` relies on: the same parameters whatever ran before"""
    for op in ("sptrsv", "spgemm"):
        first = [fuzz.DRAW[op](case, fuzz.case_rng(G.SEED, op, case), G.max_rows(op))["params"] for case in range(5)]
        again = fuzz.DRAW[op](3, fuzz.case_rng(G.SEED, op, 3), G.max_rows(op))["params"]
        assert again == first[3]
        other = fuzz.DRAW[op](3, fuzz.case_rng(G.SEED + 1, op, 3), G.max_rows(op))["params"]
        assert other != first[3]


def test_a_longer_run_pairs_every_family_with_every_limit_and_length(fuzz):
    """the rotation of drawn_plant(): every round of the families meets every (limit, length) pair, and over as many
    rounds of the families as there are pairs every family has met every pair"""
    families = len(fuzz.FAMILIES)
    for names in (["a"], ["a", "b"], ["a", "b", "c"]):
        limits = {name: 100 * (i + 1) for i, name in enumerate(names)}
        pairs = {(name, rel) for name in names for rel in fuzz.RELATIONS}
        drawn = [fuzz.drawn_plant(limits, k) for k in range(families * len(pairs))]
        for start in range(0, len(drawn), families):
            assert {(d["name"], d["rel"]) for d in drawn[start:start + families]} == pairs
        for f in range(families):
            assert {(d["name"], d["rel"]) for d in drawn[f::families]} == pairs


def test_too_few_rows_are_refused_at_once(fuzz):
    """max_rows below the families' smallest size ends in an error, not in a loop of refused draws"""
    with pytest.raises(ValueError):
        fuzz.structure(np.random.default_rng(1), fuzz.MIN_ROWS - 1, False, None, 0)
    st = fuzz.structure(np.random.default_rng(1), fuzz.MIN_ROWS, True, None, 0)
    assert st["rows"] >= 1 and st["family"] == fuzz.FAMILIES[0]
