"""The host half of tools/fuzz_spmm.py, without a GPU: the generators of the seed that tests/test_gpu_fuzz_spmm.py commits
to are run as they are there, and

- the host half of the census holds (test_gpu_fuzz_spmm.census_host): structures, case mix and switches, every kernel of
  the host rule, every staged width, two and three column chunks, split rows of several pieces, every kind of SpMV plan
  item, and the planted row is in the block with exactly the drawn length;
- every generated problem is accepted by its own reference: the grid's expected result passes the grid judge, the
  double-double reference rounded to the value type passes the bound, and the class prediction passes on an answer computed
  by a plain numpy loop;
- every judge refuses a spoiled answer: the expected grid result with one value moved by one ulp or two neighbouring unequal
  values swapped, the general reference with an error of twice its bound planted in one entry, one non-finite output's
  class changed and one finite output made NaN, one value outside the row block changed, one padding value changed, for
  beta = 0 a NaN left in the block, and a twin that differs in one bit.  This is what shows that the GPU loop would notice
  a subtly wrong kernel."""
import os

import numpy as np
import pytest

import numerics as N
import test_gpu_fuzz_spmm as G
import test_gpu_parity

OPS = ["spmm", "spmm_typed", "spmv"]
SPOILED_EVERY = 3            # the spoiled answers are tried on every third case, shifted by one after every three: the regimes
                             # turn with case % 3 too; and on every case with beta = 0 or a planted row far above its limit


@pytest.fixture(scope="module")
def fuzz(sblas):
    return G.load()


def problems(fuzz, op):
    for case in range(G.CASES):
        yield case, fuzz.DRAW[op](case, fuzz.case_rng(G.SEED, op, case), G.max_rows(op), G.cap(fuzz, op))


def refused(fuzz, op, P, ans):
    try:
        fuzz.JUDGE[op](P, ans)
    except AssertionError:
        return True
    return False


def block_of(fuzz, P, buf):
    return buf[fuzz.block_index(P).reshape(-1)].reshape(P["m"], P["n"])


def spoiled_answers(fuzz, P, good):
    """(what, answer) for every way of spoiling that applies to this case; `good` is the references' own buffer"""
    idx = fuzz.block_index(P).reshape(-1)
    X = block_of(fuzz, P, good)
    vt = P["vt"]

    def with_entry(i, value):
        bad = good.copy()
        bad[idx[i]] = value
        return dict(buf=bad)

    if P["regime"] == "grid" and X.size:
        flat = X.reshape(-1)
        i = flat.size // 2
        yield "ulp", with_entry(i, np.nextafter(flat[i], vt(np.inf)))
        differ = np.flatnonzero(flat[1:] != flat[:-1])
        if len(differ):
            i = differ[len(differ) // 2]
            bad = good.copy()
            bad[idx[[i, i + 1]]] = flat[[i + 1, i]]
            yield "swap", dict(buf=bad)
    if P["regime"] != "grid" and X.size:
        judged = P["mask"] if P.get("mask") is not None else np.ones(X.shape, bool)
        bnd = np.where(judged, P["bnd"], 0.0)
        if (bnd > 0).any():
            i = int(np.argmax(bnd))
            hi, lo = P["ref"]
            # twice the bound on top of the exact reference, in the value type's arithmetic rounded away from it
            want = float(hi.reshape(-1)[i]) + float(lo.reshape(-1)[i]) + 2.0 * float(bnd.reshape(-1)[i])
            value = vt(want)
            if float(value) < want:
                value = np.nextafter(value, vt(np.inf))
            if np.isfinite(value):
                yield "bound", with_entry(i, value)
    if P["regime"] == "nonfinite" and X.size:
        tainted = np.flatnonzero(~np.isfinite(X.reshape(-1)))
        if len(tainted):
            i = tainted[0]
            yield "class", with_entry(i, vt(1.0) if np.isnan(X.reshape(-1)[i]) or X.reshape(-1)[i] < 0 else vt(-np.inf))
        finite = np.flatnonzero(np.isfinite(X.reshape(-1)))
        if len(finite):
            yield "nan", with_entry(finite[len(finite) // 2], vt(np.nan))
    if P["beta"] == 0 and np.isfinite(X).any():          # C's NaN still there, where the answer is finite
        yield "nan_left", with_entry(np.flatnonzero(np.isfinite(X.reshape(-1)))[-1], vt(np.nan))
    outside = np.ones(good.shape, bool)
    outside[idx] = False
    pad = fuzz.padding_index(P) if P["op"] != "spmv" else np.zeros(0, np.int64)
    if len(pad):
        bad = good.copy()
        bad[pad[len(pad) // 2]] += vt(1.0)
        yield "padding", dict(buf=bad)
        outside[pad] = False
    rows_outside = np.flatnonzero(outside)
    if len(rows_outside):
        bad = good.copy()
        i = rows_outside[len(rows_outside) // 2]
        bad[i] = np.nextafter(bad[i], vt(np.inf))
        yield "outside", dict(buf=bad)
    if X.size and np.isfinite(X).any():
        twin = X.copy()
        i = np.flatnonzero(np.isfinite(twin.reshape(-1)))[0]
        twin.reshape(-1)[i] = np.nextafter(twin.reshape(-1)[i], vt(np.inf))
        yield "twin", dict(buf=good, twin=twin)


KINDS = ["ulp", "swap", "bound", "class", "nan", "nan_left", "outside", "twin"]


@pytest.mark.parametrize("op", OPS)
def test_generated_cases_are_accepted_and_spoiled_answers_refused(fuzz, op):
    seen, spoiled = [], {}
    limits = fuzz.limits_of(op)
    offset = dict(below=lambda v: v - 1, at=lambda v: v, above=lambda v: v + 1, far=lambda v: 2 * v + 3)
    for case, P in problems(fuzz, op):
        st = P["st"]
        a, b = P["block"]
        assert 0 <= a <= b <= P["rows"] and P["m"] == b - a and len(P["sub_rp"]) == P["m"] + 1 and P["sub_rp"][0] == 0, P["params"]
        assert P["sub_rp"][-1] == P["nnz"] == len(P["sub_ci"]) and (P["nnz"] == 0 or (0 <= P["sub_ci"].min() and P["sub_ci"].max() < P["cols"]))
        assert P["nnz"] * P["n"] <= G.cap(fuzz, op) or P["n"] == 1, P["params"]
        if st["plant"]:                                                      # the planted row is in the block, with exactly the drawn length
            want = offset[st["plant"]["rel"]](limits[st["plant"]["name"]])
            assert st["plant"]["L"] == want
            assert a <= st["planted_row"] < b and np.diff(P["sub_rp"])[st["planted_row"] - a] == want, P["params"]
        good = fuzz.reference_answer(P)
        fuzz.JUDGE[op](P, dict(buf=good))                                    # raises with the parameters when the reference refuses
        fuzz.JUDGE[op](P, dict(buf=good, twin=block_of(fuzz, P, good)))
        seen.append(fuzz.census_of(P))
        if (case + case // SPOILED_EVERY) % SPOILED_EVERY == 0 or st["plant"] and st["plant"]["rel"] == "far" or P["beta"] == 0:
            for what, bad in spoiled_answers(fuzz, P, good):
                assert refused(fuzz, op, P, bad), "a spoiled answer (%s) is accepted: %s" % (what, P["params"])
                spoiled[what] = spoiled.get(what, 0) + 1
    G.census_host(fuzz, op, seen)
    for what in KINDS + ([] if op == "spmv" else ["padding"]):
        assert spoiled.get(what, 0) >= 3, (what, spoiled)
    assert not any(name in os.environ for name in fuzz.SWITCHES)             # draw() leaves no switch behind


def test_case_k_is_a_function_of_seed_operation_and_k_alone(fuzz):
    """what `--op X --seed S --only K` relies on: the same parameters whatever ran before"""
    for op in OPS:
        first = [fuzz.DRAW[op](case, fuzz.case_rng(G.SEED, op, case), G.max_rows(op))["params"] for case in range(5)]
        again = fuzz.DRAW[op](3, fuzz.case_rng(G.SEED, op, 3), G.max_rows(op))["params"]
        assert again == first[3]
        other = fuzz.DRAW[op](4, fuzz.case_rng(G.SEED + 1, op, 4), G.max_rows(op))["params"]
        assert other != first[4]


def test_the_tool_reads_the_lists_the_kernel_tests_use(fuzz):
    """the selections are those of test_gpu_parity / test_gpu_numerics, the regimes those of test_gpu_numerics"""
    assert fuzz.SPMM_VARIANTS == test_gpu_parity.SPMM_VARIANTS and len(fuzz.SPMM_VARIANTS) == 7
    assert fuzz.SPMV_VARIANTS == fuzz.TG.SPMV_VARIANTS and len(fuzz.SPMV_VARIANTS) == 12
    assert fuzz.GRID == ["R1", "R2", "R3sub", "R3over"] and set(fuzz.FP.FAMILIES) < set(fuzz.FAMILIES)
    assert [(np.dtype(v), np.dtype(i)) for v, i in fuzz.TYPED] == [(np.dtype(v), np.dtype(i)) for v, i in fuzz.TG.TYPED]


def test_switches_are_unset_again_on_every_path(fuzz):
    with pytest.raises(RuntimeError):
        with fuzz.switched({"SBLAS_SPMM_VARIANT": "mfma", "SBLAS_SPMM_MIN_LDBT": "64"}):
            assert os.environ["SBLAS_SPMM_VARIANT"] == "mfma" and fuzz.S.lib().sblas_hip_spmm_ldbt(9) == 64
            raise RuntimeError("a failing case")
    assert not any(name in os.environ for name in fuzz.SWITCHES) and fuzz.S.lib().sblas_hip_spmm_ldbt(9) == 16


def test_the_library_states_its_column_chunks(fuzz):
    """staged_widths() reads the chunk width off the workspace query: 300 columns under a limit just above a 128-column
    copy are walked as 128 + 128 + 44 (staged 128, 128, 64), and whole without the limit"""
    m = cols = 700
    assert fuzz.staged_widths(m, cols, 5000, 300) == (300, [384])
    with fuzz.switched({"SBLAS_SPMM_MAX_BT_BYTES": 8 * (cols + 1) * 128 + 8}):
        assert fuzz.staged_widths(m, cols, 5000, 300) == (128, [128, 128, 64])
        assert fuzz.staged_widths(m, cols, 5000, 256) == (128, [128, 128])
        assert fuzz.staged_widths(m, cols, 5000, 130) == (128, [128, 8])
        assert fuzz.staged_widths(m, cols, 5000, 64) == (64, [64])


def test_too_few_rows_are_refused_at_once(fuzz):
    with pytest.raises(ValueError):
        fuzz.structure(np.random.default_rng(1), fuzz.MIN_ROWS - 1, None, 0)
