"""The oracle (oracle/sblas_oracle.c, a CPU restatement of the reference) against every known answer the
reference's own code has produced for this path: SURVEY.md 8(c) values (tests/golden/ash85_golden.json)
and the reference's own loader (compiled from source into oracle/_ref, or its committed outputs) on ash85 and
tests/golden/loader_cases/."""
import json
import os

import numpy as np
import pytest

from conftest import ASH85, GOLDEN


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLDEN, "ash85_golden.json")) as f:
        return json.load(f)


def seq_sum(a):
    s = 0.0
    for x in a:
        s += float(x)
    return s


def test_loader_ash85_known_answers(oracle, ash85, gold):
    g = gold["loader"]
    assert (ash85["m"], ash85["n"], ash85["nnz"], ash85["sym"]) == (g["m"], g["n"], g["nnz"], g["symmetric"])
    rp, ci, v = ash85["rowptr"], ash85["colidx"], ash85["val"]
    assert rp[:9].tolist() == g["rowptr_head"] and rp[85] == g["rowptr_last"]
    assert ci[rp[0]:rp[1]].tolist() == g["row0_cols"]
    assert ci[rp[1]:rp[2]].tolist() == g["row1_cols"]
    assert ci[rp[84]:rp[85]].tolist() == g["row84_cols"]
    lens = np.diff(rp)
    assert lens.min() == g["row_len_min"] and lens.max() == g["row_len_max"]
    assert v.sum() == g["val_sum"] and (v == 1.0).all()
    assert all((np.diff(ci[rp[r]:rp[r + 1]]) > 0).all() for r in range(85))


def stored_reference_loader_outputs():
    """path -> what the reference's own loader returned on it, as committed by tests/golden/make_loader_fixtures.py
    (loader_expected.json for loader_cases/, ash85_ref_loader.json for ash85)."""
    with open(os.path.join(GOLDEN, "loader_expected.json")) as f:
        exp = {os.path.join(GOLDEN, "loader_cases", k + ".mtx"): e for k, e in json.load(f).items() if not k.startswith("_")}
    with open(os.path.join(GOLDEN, "ash85_ref_loader.json")) as f:
        exp[ASH85] = json.load(f)["ash85"]
    return {p: (e["m"], e["n"], e["nnz"], e["symmetric"], np.array(e["rowptr"], np.int32), np.array(e["colidx"], np.int32),
                np.array([float.fromhex(x) for x in e["val"]], np.float64)) for p, e in exp.items()}


def test_loader_restatement_equals_reference_loader(oracle):
    """Bit-exact: our restatement vs the reference's own mmio loader, ash85 + the loader_cases files.  The reference's
    arrays come from the loader itself where build() made oracle/_ref, else from the fixtures it wrote; where both
    exist they must agree, so the fixtures stay what the loader returns."""
    stored = stored_reference_loader_outputs()
    paths = [ASH85] + sorted(os.path.join(GOLDEN, "loader_cases", f) for f in os.listdir(os.path.join(GOLDEN, "loader_cases")))
    assert sorted(paths) == sorted(stored)
    live = oracle.ref_loader() is not None
    for p in paths:
        a, b = oracle.read_mtx(p), (oracle.read_mtx_ref(p) if live else stored[p])
        for got in (a, stored[p]) if live else (a,):
            assert got[:4] == b[:4], p
            for x, y in zip(got[4:], b[4:]):
                assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), p


def test_loader_restatement_against_committed_reference_outputs(oracle):
    """Same check from the committed fixtures alone (works where the reference tree and oracle/_ref are absent)."""
    with open(os.path.join(GOLDEN, "loader_expected.json")) as f:
        exp = json.load(f)
    for name, e in exp.items():
        if name.startswith("_"):
            continue
        m, n, nnz, sym, rp, ci, v = oracle.read_mtx(os.path.join(GOLDEN, "loader_cases", name + ".mtx"))
        assert (m, n, nnz, sym) == (e["m"], e["n"], e["nnz"], e["symmetric"]), name
        assert rp.tolist() == e["rowptr"] and ci.tolist() == e["colidx"], name
        assert [float(x).hex() for x in v] == e["val"], name


@pytest.mark.parametrize("key", ["spmm_n64_a1_b1", "spmm_n256_a3_b4"])
def test_spmm_cpu_known_answers(oracle, ash85, gold, key):
    g = gold[key]
    N = g["N"]
    B = oracle.rand0to1(85 * N)          # DenseMatrix(K, N, col_major): srand(211), rand()/RAND_MAX, linear fill
    C = np.full(85 * N, g["C0"])
    oracle.spmm(85, 85, N, ash85["rowptr"], ash85["colidx"], ash85["val"], B, C, g["alpha"], g["beta"])
    assert B[-1] == g["B_last"]
    if "B_first" in g:
        assert B[0] == g["B_first"] and B[1] == g["B_second"]
    assert C[0] == g["C_first"] and C[1] == g["C_second"] and C[-1] == g["C_last"]
    assert seq_sum(C) == g["C_sum"]     # exact: same values, same left-to-right summation


@pytest.mark.parametrize("key", ["spmv_a1_b1", "spmv_a3_b4"])
def test_spmv_cpu_known_answers(oracle, ash85, gold, key):
    g = gold[key]
    x, y = np.ones(85), np.ones(85)
    oracle.spmv(85, ash85["rowptr"], ash85["colidx"], ash85["val"], x, y, g["alpha"], g["beta"])
    assert (y[0], y[1], y[84], seq_sum(y)) == (g["y_first"], g["y_second"], g["y_last"], g["y_sum"])


def test_segment_tables_known_answers(oracle, ash85, gold):
    rp = ash85["rowptr"]
    for g_str, table in gold["segments"].items():
        g = int(g_str)
        got = [list(oracle.partition_nnz(rp, 85, 523, g, i)[:3]) for i in range(g)]
        assert got == table
    for i_str, head in gold["rebased_heads_g4"].items():
        s, e, k, reb, _ = oracle.partition_nnz(rp, 85, 523, 4, int(i_str))
        assert reb[:6].tolist() == head and reb[-1] == gold["rebased_tails_g4"][i_str] and len(reb) == e - s + 2
    for g_str, dims in gold["dense_segments_n64"].items():
        g = int(g_str)
        assert [oracle.partition_dense(64, g, i)[1] for i in range(g)] == dims


def test_method2_emulation_matches_verifier(oracle, ash85, gold):
    """g-way nnz partition + zero Ccopy + sum + axpby, all on the CPU, reproduces the verifier to the
    bound the survey measured with the reference's own partitioner (<= 7.1e-15 abs at g=8)."""
    rp, ci, v = ash85["rowptr"], ash85["colidx"], ash85["val"]
    N = 64
    B = oracle.rand0to1(85 * N)
    ref = np.ones(85 * N)
    oracle.spmm(85, 85, N, rp, ci, v, B, ref, 1.0, 1.0)
    for g in (1, 2, 4, 8):
        total = np.zeros(85 * N)
        for i in range(g):
            s, e, k, reb, avg = oracle.partition_nnz(rp, 85, 523, g, i)
            part = np.zeros(85 * N)
            m_i = e - s + 1
            view = np.zeros(m_i * N)
            lo = i * avg
            oracle.spmm(m_i, 85, N, reb, ci[lo:lo + k].copy(), v[lo:lo + k].copy(), B, view, 1.0, 1.0)
            part.reshape(N, 85)[:, s:s + m_i] = view.reshape(N, m_i)
            total += part
        C = np.ones(85 * N)
        oracle.lib().orc_axpby(C.size, 1.0, total, 1.0, C)
        assert np.abs(C - ref).max() <= max(gold["method2_emulation_max_abs_diff"][str(g)] * 2, 1e-14)


def test_float_ceil_quirk_is_documented_not_inherited(oracle):
    """matrix.h:360 uses ceil((float)nnz/g); above 2^24 that drops nonzeros (Queen_4147, SURVEY hazards)."""
    L = oracle.lib()
    assert L.orc_avg_nnz_float(523, 4) == L.orc_avg_nnz_exact(523, 4) == 131
    assert L.orc_avg_nnz_float(28715634, 4) == L.orc_avg_nnz_exact(28715634, 4)
    assert L.orc_avg_nnz_float(316548962, 8) == 39568620 and L.orc_avg_nnz_exact(316548962, 8) == 39568621
