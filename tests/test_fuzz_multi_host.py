"""The host half of tools/fuzz_multi.py, without a GPU: the generators of the seed that tests/test_gpu_fuzz_multi.py commits
to are run as they are there, and

- every draw is sound: a pcg matrix is symmetric and strictly dominant (the doubled entries summed), the others strictly
  dominant by rows, one stored diagonal a row, a preconditioned pattern passes ilu0_numerics.check, the planted row has
  exactly the drawn length against SPMM_SPLIT_MIN, the planted n is exact, an exact guess leaves b - A x0 = 0, and the
  bounded product s * max_iter * dots per iteration is at most DOT_BUDGET;
- for every case without a preconditioner or with Jacobi, the lockstep composition over host parts that are separable by
  column (krylov_numerics.matvec per column, the pinned dot's restatement) equals s independent single compositions of
  tests/solver_compose.py field by field: the composition is held to the single loops before the device is held to it;
- with Jacobi the plain float64 host loop meets RTOL on a random column of every drawn matrix within MAX_ITER - 10
  iterations (GMRES(1) apart), which is where MAX_ITER comes from;
- the host half of the census holds at the committed CASES, the statuses' half over the cases the host can compose;
- every planted breakdown, as one column of a block, reaches its literal under the host composition and leaves the other
  columns what they are without it;
- every judge refuses an answer with one flipped bit, one wrong status and one wrong count."""
import math

import numpy as np
import pytest

import ilu0_numerics as IN
import krylov_numerics as KN
import numerics as NM
import test_fuzz_solvers_host as H
import test_gpu_fuzz_multi as G

SOLVERS = ["pcg_multi", "bicgstab_multi", "gmres_multi"]


@pytest.fixture(scope="module")
def fuzz(sblas):
    return G.load()


def problems(fuzz, op):
    for case in range(G.CASES[op]):
        yield case, fuzz.DRAW[op](case, fuzz.case_rng(G.SEED, op, case), G.max_rows(op))


def assert_sound_matrix(fuzz, base, P, conformed):
    n, rp, ci, st = P["n"], P["rp"], P["ci"], P["st"]
    assert len(rp) == n + 1 and rp[0] == 0 and rp[-1] == len(ci) and (np.diff(rp) >= 0).all(), P["params"]
    assert len(ci) == 0 or (0 <= ci.min() and ci.max() < n), P["params"]
    assert all(len(v) == len(ci) for v in P["val"]), P["params"]
    if P["size"] is not None:
        assert n == P["size"] and st["plant"] is None, P["params"]
    if st["degenerate"] and not conformed:
        assert P["precond"] is None, P["params"]
        return
    row = NM.row_of_entries(rp)
    assert (np.bincount(row[ci == row], minlength=n) == 1).all(), P["params"]          # one stored diagonal a row
    if st["plant"]:
        assert np.diff(rp.astype(np.int64))[P["planted_row"]] == st["plant"]["L"], P["params"]
        split = fuzz.S.SPMM_SPLIT_MIN
        assert st["plant"]["name"] == "spmm_split", P["params"]
        assert st["plant"]["L"] == dict(below=split - 1, at=split, above=split + 1, far=2 * split + 3)[st["plant"]["rel"]], P["params"]
    if P["precond"] is not None:
        assert IN.check(n, rp, ci)[1] is None, P["params"]
    for val in P["val"]:
        assert np.isfinite(val).all()
        key, v = H.summed(n, rp, ci, val)
        r, c = key // max(n, 1), key % max(n, 1)
        off = np.bincount(r, np.where(r == c, 0.0, np.abs(v)), minlength=n)
        assert (v[r == c] > off).all(), P["params"]                                    # strictly dominant, a positive diagonal
        if base == "pcg":
            mirror = np.searchsorted(key, c * n + r)
            assert (mirror < len(key)).all() and np.array_equal(key[mirror], c * n + r) and np.array_equal(v[mirror], v), P["params"]


def assert_sound(fuzz, op, P):
    assert_sound_matrix(fuzz, P["base"], P, False)
    n, s = P["n"], P["s"]
    assert P["B"].shape == P["X0"].shape == (n, s) and len(P["kinds"]) == s and "random" in P["kinds"], P["params"]
    assert s in fuzz.WIDTHS and 1 <= P["max_iter"] <= fuzz.MAX_ITER and fuzz.dot_product(P) <= fuzz.DOT_BUDGET, P["params"]
    assert P["budget"] in (fuzz.DOT_BUDGET, fuzz.DOT_BUDGET // 2, fuzz.DOT_BUDGET // 4), P["params"]
    assert fuzz.dot_product(P) <= P["budget"] or P["max_iter"] == 1, P["params"]       # a halved budget still leaves one iteration
    if P["base"] == "gmres":
        assert 1 <= P["restart"] <= P["restart_drawn"], P["params"]
        assert P["restart"] in (1, P["restart_drawn"]) or s * (P["restart"] + 2) <= P["budget"] < s * (P["restart"] + 3), P["params"]   # no further than one iteration needs
    if P["regime"] == "b" and P["atol"] == fuzz.B_NEAR * fuzz.RTOL * float(np.linalg.norm(P["B"][:, P["kinds"].index("random")])) and n:
        warm = [j for j, k in enumerate(P["kinds"]) if k.startswith("warm")]     # near: every other warm column is B_SCALE times a warm problem
        norms = [float(np.linalg.norm(P["B"][:, j])) for j in warm]
        assert all(norms[i] > 0.01 * fuzz.B_SCALE * norms[i + 1] for i in range(0, len(warm) - 1, 2)), P["params"]
    for j, kind in enumerate(P["kinds"]):
        b, x0 = P["B"][:, j], P["X0"][:, j]
        if kind == "zero":
            assert not b.any() and (x0.any() or n == 0), P["params"]
        elif kind == "nan":
            assert np.isnan(b).sum() == min(n, 1), P["params"]
        elif kind == "exact":
            assert P["integer"] and not np.any(b - KN.matvec(n, P["rp"], P["ci"], P["val"][0], x0)), P["params"]
        else:
            assert np.isfinite(b).all() and np.isfinite(x0).all(), P["params"]


def dinv_of(P, val):
    return 1.0 / val[P["ci"] == NM.row_of_entries(P["rp"])] if P["precond"] == "jacobi" else None


def host_answer(fuzz, P, val):
    """the case under the lockstep composition on host parts -> (the answers, rtol, atol, max_iter, expected)"""
    parts = fuzz.host_parts(P["n"], P["rp"], P["ci"], val, dinv_of(P, val))
    loop = lambda rtol, atol, max_iter: fuzz.compose(P["base"], parts, P["B"], P["X0"], P["restart"], rtol, atol, max_iter)
    rtol, atol, max_iter, expected = fuzz.stopping(P, loop)
    return loop(rtol, atol, max_iter), rtol, atol, max_iter, expected


def spoiled_blocks(want):
    """(what, answers) with one column spoiled in every way that applies"""
    j = len(want) // 2
    for what, bad in H.spoiled_answers(want[j]):
        yield what, want[:j] + [bad] + want[j + 1:]
    if len(want) > 1:                                                        # two columns' answers exchanged
        k = (j + 1) % len(want)
        if not KN.same_bits(want[j]["x"], want[k]["x"]):
            swapped = list(want)
            swapped[j], swapped[k] = want[k], want[j]
            yield "columns", swapped


@pytest.mark.parametrize("op", SOLVERS)
def test_generated_cases_are_sound_composed_like_the_single_loops_and_spoiled_answers_refused(fuzz, op):
    base = fuzz.BASE[op]
    seen, spoiled, jacobi_counts = [], {}, []
    for case, P in problems(fuzz, op):
        assert_sound(fuzz, op, P)
        record = fuzz.census_of(P)
        seen.append(record)
        if P["st"]["degenerate"] is None and not (base == "gmres" and P["restart"] == 1):
            # where MAX_ITER comes from: once it has Jacobi, a random column of every drawn matrix is solved by the plain
            # host loop of the same method within MAX_ITER - 10 iterations
            j = P["kinds"].index("random")
            Pj = dict(fuzz.column_problem(P, j), precond="jacobi", restart=P["restart_drawn"])
            its, _ = fuzz.FS.host_solution(Pj, P["val"][0], fuzz.RTOL, 0.0)
            assert its <= fuzz.MAX_ITER - 10 < fuzz.FS.HOST_LIMIT, (its, P["params"])
            jacobi_counts.append(its)
        if P["precond"] not in (None, "jacobi"):
            continue
        solves = []
        for which, val in enumerate(P["val"]):
            want, rtol, atol, max_iter, expected = host_answer(fuzz, P, val)
            fuzz.judge_expectation(P, want, expected, first=not which)
            bar = 0
            if which == 0:                                                   # the lockstep loop against s single loops, field by field
                alone = [fuzz.single(P, val, j, rtol, atol, max_iter, dinv_of(P, val)) for j in range(P["s"])]
                fuzz.JUDGE[op](P, want, alone, "the lockstep composition against the single ones")
                for what, bad in spoiled_blocks(want):
                    assert H.refused(fuzz.JUDGE[op], P, bad, want), "a spoiled answer (%s) is accepted: %s" % (what, P["params"])
                    spoiled[what] = spoiled.get(what, 0) + 1
                bar = len(fuzz.judge_bar(P, val, want, want, rtol, atol))
            solves.append(fuzz.summary(P, want, rtol, atol, max_iter, bar))
        record["solves"] = solves
    G.host_census(fuzz, seen, op)
    # the statuses' half over the cases the host can compose (no seat): the residual bar's share in full, the freeze at least once
    G.status_census([s for s in seen if "solves" in s], op, G.BAR_CASES, 1, mixed=op != "pcg_multi")
    print("%s: host iterations with Jacobi on a random column: max %d over %d matrices" % (op, max(jacobi_counts), len(jacobi_counts)))
    for what in ("ulp", "swap", "iterations", "status", "rnorm", "columns"):
        assert spoiled.get(what, 0) >= 10, (what, spoiled)


def test_the_block_operations_draws_are_sound_and_their_judges_refuse_a_flipped_bit(fuzz):
    seen = []
    for case, P in problems(fuzz, "sptrsm_tiled"):
        T, L = P["T"], P["L"]
        assert P["B"].shape == (T["n"], P["s"]) and P["R"].shape == (L["n"], P["s"]) and 0 <= P["column"] < P["s"], P["params"]
        assert IN.check(L["n"], L["rp"], L["ci"])[1] is None, P["params"]
        seen.append(fuzz.FP.census_of(P["st"], s=P["s"], layout=P["layout"], lower=T["lower"], unit=T["unit"], schedule=P["schedule"],
                                      ilu_family=L["st"]["family"],
                                      ilu_planted=(L["st"]["plant"]["name"], L["st"]["plant"]["rel"]) if L["st"]["plant"] else None))
        if P["B"].size:
            fuzz.judge_sptrsm_tiled(P, P["B"], P["B"])
            assert H.refused(fuzz.judge_sptrsm_tiled, P, H.one_ulp(P["B"]), P["B"]), P["params"]
    G.sptrsm_census(fuzz, seen)
    seen = []
    for case, P in problems(fuzz, "amg_multi"):
        assert_sound_matrix(fuzz, P["base"], P, True)
        assert [r.shape for r in P["R"]] == [(P["n"], P["s"]), (P["n"], P["s2"])] and 1 <= P["s2"] <= P["s"], P["params"]
        assert P["n"] == 0 or any(not P["R"][0][:, j].any() for j in range(P["s"])), P["params"]
        seen.append(fuzz.FP.census_of(P["st"], n=P["n"], size=P["size"], base=P["base"], precond=P["precond"], s=P["s"], s2=P["s2"],
                                      layout=P["layout"]))
        if P["R"][0].size:
            assert H.refused(fuzz.judge_amg_multi, P, H.one_ulp(P["R"][0]), P["R"][0]), P["params"]
    G.amg_census(fuzz, seen)


def test_the_turns_have_no_common_factor_and_fit_a_run(fuzz):
    lengths = sorted([len(v) for v in fuzz.TURNS.values()] + [len(v) for v in fuzz.FS.TURNS.values()])
    assert all(math.gcd(a, b) == 1 for i, a in enumerate(lengths) for b in lengths[i + 1:]), lengths
    assert max(lengths) < fuzz.RUN and max(G.CASES.values()) <= fuzz.RUN
    assert all(fuzz.UNCHANGED[name] is fuzz.FS.TURNS[name] for name in fuzz.UNCHANGED)
    for start in (0, 17, 1000):                                              # any RUN consecutive cases meet every value
        met = [fuzz.turn(k) for k in range(start, start + fuzz.RUN)]
        assert {t["width"] for t in met} == set(fuzz.WIDTHS) and {t["layout"] for t in met} == set(fuzz.LAYOUTS)
        assert {t["size"] for t in met} == set(fuzz.SIZES) | {None} and {t["precond"] for t in met} == set(fuzz.PRECONDS)
        assert {t["amg"] for t in met} == set(fuzz.AMG_DOORS) and {t["restart"] for t in met} == set(fuzz.RESTARTS)
        assert {t["regime"] for t in met} == set(fuzz.REGIMES) and {t["check_every"] for t in met} == set(fuzz.CHECK_EVERY)
    lim = fuzz.S.krylov_multi_limits()
    tile, top = lim["tile"], lim["max_rhs"]
    assert set(fuzz.WIDTHS) == {1, 2, top} | {w for k in (1, 2, 4, 8) for w in (k * tile - 1, k * tile, k * tile + 1) if w <= top}
    assert fuzz.SIZES == [lim["cell"] - 1, lim["cell"], lim["cell"] + 1, 2 * lim["cell"] + 5]
    assert fuzz.DOT_BUDGET >= top * max(fuzz.DOTS.values())                 # one iteration of every method fits at every width
    for s in fuzz.WIDTHS:
        for layout in fuzz.LAYOUTS:
            (ldb, ob), (ldx, ox) = fuzz.MP.layout_of(layout, s)
            assert ldb >= s and ldx >= s
            if layout == "odd":
                assert (ldb, ldx, ox % 2) == (s + 1, s + 3, 1)
            if layout == "even":
                assert ldb % 2 == ldx % 2 == ob % 2 == ox % 2 == 0 and ldb > s


def test_case_k_is_a_function_of_seed_operation_and_k_alone(fuzz):
    for op in fuzz.OPS:
        first = [fuzz.DRAW[op](case, fuzz.case_rng(G.SEED, op, case), G.max_rows(op))["params"] for case in range(4, 8)]
        again = fuzz.DRAW[op](6, fuzz.case_rng(G.SEED, op, 6), G.max_rows(op))["params"]
        assert again == first[2]
        assert fuzz.DRAW[op](6, fuzz.case_rng(G.SEED + 1, op, 6), G.max_rows(op))["params"] != first[2]


def test_every_planted_breakdown_reaches_its_literal_inside_a_block(fuzz):
    named = set()
    for plant in fuzz.PLANTS:
        want = fuzz.host_plant(plant)
        column = want[fuzz.PLANT_COLUMN]
        fuzz.FS.judge_plant(plant, column)
        named.add((plant["op"], column["breakdown"]))
        # every column is what the single composition makes of it alone: the planted one reaches no other
        n, rp, ci, val, dinv, B, X0 = fuzz.plant_block(plant)
        P = dict(fuzz.FS.plant_params(plant), base=plant["op"], n=n, rp=rp, ci=ci, B=B, X0=X0, restart=plant.get("restart"))
        alone = [fuzz.single(P, val, j, fuzz.FS.PLANT_KW["rtol"], fuzz.FS.PLANT_KW["atol"], fuzz.FS.PLANT_KW["max_iter"], dinv) for j in range(B.shape[1])]
        fuzz.judge(plant["op"] + "_multi", P, want, alone, "the planted block against the single compositions")
        assert H.refused(fuzz.FS.judge_plant, plant, dict(column, iterations=column["iterations"] + 1))
    assert named >= {("pcg", "(p, q)"), ("pcg", "rho"), ("bicgstab", "(r^, v)"), ("bicgstab", "(t, t)"), ("bicgstab", "omega"),
                     ("bicgstab", "rho"), ("bicgstab", None), ("gmres", "givens"), ("gmres", "beta")}
