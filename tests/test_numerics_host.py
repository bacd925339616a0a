"""The numerics checkers of tests/numerics.py, checked on the host before they judge a kernel: the double-double
reference and the exact grids against rational arithmetic, the rounding bound against the CPU oracle (it must accept
every correct result and reject a wrong one), and the IEEE-class predictor against the oracle's own Inf / NaN."""
import math
from fractions import Fraction

import numpy as np
import pytest

import numerics as N


def _structure(m=40, k=37, avg=6, seed=0, dup=True):
    """A small CSR structure with empty rows, unsorted rows, duplicates (when dup) and one long row."""
    from sblas_amd import synth
    rp, ci, v = synth.random_csr(m, k, avg, seed=seed, empty_every=7, long_row=(3, 60))
    if dup:
        ci = ci.copy()
        ci[rp[5]:rp[6]] = ci[rp[5]]                    # one row that repeats a single column
    return rp.astype(np.int32), ci.astype(np.int32)


def _general(rng, rp, ci, k, n, regime, dtype=np.float64):
    m, nnz = len(rp) - 1, len(ci)
    if regime == "spread60":
        f = lambda s: N.log_uniform(rng, s, 60, dtype)
    elif regime == "subnormal":                       # products and sums straddle the subnormal range
        f = lambda s: N.log_uniform(rng, s, 20, dtype, center=-530 if dtype == np.float64 else -70)
    elif regime == "overflow":
        f = lambda s: N.log_uniform(rng, s, 8, dtype, center=495 if dtype == np.float64 else 56)
    else:                                             # "cancel": pairs of nearly opposite terms (numerics.cancelling_pairs)
        f = lambda s: (rng.standard_normal(s) * 1e3).astype(dtype)
    A, B, C = f(nnz), f((k, n)), f((m, n))
    if regime == "cancel":
        B[1::2] = B[0::2][: k // 2]
        lead, follow, lone = N.cancelling_pairs(rp, ci, k)
        A[follow] = -A[lead] * (1 + 2.0 ** -40 * (dtype == np.float64))
        A[lone] *= 1e-6
        C *= 1e-6
    return A, B, C


def _frac_err(hi, lo, exact):
    return abs(Fraction(float(hi)) + Fraction(float(lo)) - exact)


DD_REGIMES = ["cancel", "spread60", "subnormal", "overflow"]
DD_SCALARS = [(0.1, 0.0), (-1 / 3, 0.3), (7.3e5, -2 / 7)]


@pytest.mark.parametrize("regime", DD_REGIMES)
@pytest.mark.parametrize("alpha,beta", DD_SCALARS)
def test_double_double_reference_matches_fractions(oracle, regime, alpha, beta):
    rp, ci = _structure(seed=3)
    k, n = 37, 3
    rng = np.random.default_rng(10 * DD_REGIMES.index(regime) + DD_SCALARS.index((alpha, beta)))
    if regime == "overflow":
        alpha = math.copysign(min(abs(alpha), 1.0), alpha)       # keep the result finite
    A, B, C = _general(rng, rp, ci, k, n, regime)
    hi, lo = N.reference_dd(rp, ci, A, B, C, alpha, beta)
    exact = N.exact_fraction(rp, ci, A, B, C, alpha, beta)
    S = N.abs_sum(rp, ci, A, B, C, alpha, beta)
    if regime == "cancel":                            # many results are far below their sums of magnitudes
        ratio = np.array([float(abs(exact[i][j])) for i in range(len(rp) - 1) for j in range(n)]) / np.maximum(S.ravel(), 1e-300)
        assert (ratio[S.ravel() > 0] < 1e-4).mean() > 0.25, np.sort(ratio)
    for i in range(len(rp) - 1):
        for j in range(n):
            err = _frac_err(hi[i, j], lo[i, j], exact[i][j])
            assert err <= Fraction(2.0 ** -100) * Fraction(float(S[i, j])) + 2 * Fraction(N.eta(np.float64)), (i, j)


GRID_REGIMES = {
    "cancel": dict(cancel=True, alpha=-2.0, beta=0.0),
    "cancel_beta": dict(cancel=True, alpha=1.0, beta=-0.5),
    "spread": dict(spread=24, alpha=0.25, beta=2.0),
    "subnormal": dict(scale=-537, alpha=1.0, beta=1.0),
    "overflow": dict(scale=480, alpha=-1.0, beta=0.25),
}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("regime", sorted(GRID_REGIMES))
def test_grid_expectation_is_exact(regime, dtype):
    kw = dict(GRID_REGIMES[regime])
    if dtype == np.float32:
        kw.update({"spread": dict(spread=8), "subnormal": dict(scale=-75, scale_b=-74),
                   "overflow": dict(scale=50)}.get(regime, {}))
    rp, ci = _structure(seed=5)
    g = N.grid_problem(rp, ci, 37, 4, dtype=dtype, seed=2, **kw)
    assert g.expected.dtype == np.dtype(dtype) and np.isfinite(g.expected).all()
    exact = N.exact_fraction(rp, ci, g.A, g.B, g.C, g.alpha, g.beta)
    for i in range(len(rp) - 1):
        for j in range(4):
            assert Fraction(float(g.expected[i, j])) == exact[i][j], (i, j)
    if regime == "spread" and dtype == np.float64:
        prods = np.log2(np.abs(g.A[rp[3]:rp[4], None] * g.B[ci[rp[3]:rp[4]]]))     # the 60-entry row
        assert np.ptp(prods) >= 20
    if regime == "subnormal":
        assert (np.abs(g.expected[g.expected != 0]) < np.finfo(dtype).tiny).any()
    if regime == "overflow":
        assert np.abs(g.expected).max() > (2.0 ** 990 if dtype == np.float64 else 2.0 ** 110)


def test_grid_cancelling_pairs_leave_small_outputs():
    from sblas_amd import synth
    rp, ci, v = synth.banded(300, 20, 40)
    g = N.grid_problem(rp, ci, 300, 3, cancel=True, alpha=1.0, beta=0.0, seed=1)
    assert g.worst >= 2 ** 40                                   # partial sums near 2^43 grid units ...
    assert np.abs(np.ldexp(g.expected, -g.e0)).max() < 2.0 ** 26   # ... outputs 2^17 times smaller


def test_grid_precondition_fires_on_an_oversized_grid():
    from sblas_amd import synth
    rp, ci, v = synth.banded(100, 40, 60)
    with pytest.raises(AssertionError, match="grid precondition"):
        N.grid_problem(rp, ci, 100, 2, bits=26, spread=4)
    with pytest.raises(AssertionError, match="grid precondition"):
        N.grid_problem(rp, ci, 100, 2, dtype=np.float32, bits=12)
    with pytest.raises(AssertionError, match="smallest subnormal"):
        N.grid_problem(rp, ci, 100, 2, scale=-538, alpha=1.0, beta=0.0)


def _oracle_run(oracle, kind, vt, it, rp, ci, A, B, C, alpha, beta):
    """The host oracle's result of one product, as an m x n array."""
    m, k, n = len(rp) - 1, B.shape[0], B.shape[1]
    rp, ci = rp.astype(it), ci.astype(it)
    A, B, C = A.astype(vt), B.astype(vt), C.astype(vt)
    typed = not (vt == np.float64 and it == np.int32)
    if kind == "spmv":
        x, y = np.ascontiguousarray(B[:, 0]), np.ascontiguousarray(C[:, 0]).copy()
        (oracle.spmv_typed if typed else oracle.spmv)(m, rp, ci, A, x, y, alpha, beta)
        return y[:, None]
    Bf, Cf = np.ascontiguousarray(B.T).reshape(-1), np.ascontiguousarray(C.T).reshape(-1).copy()
    (oracle.spmm_typed if typed else oracle.spmm)(m, k, n, rp, ci, A, Bf, Cf, alpha, beta)
    return Cf.reshape(n, m).T


TYPES = [(np.float64, np.int32), (np.float64, np.int64), (np.float32, np.int32), (np.float32, np.int64)]


@pytest.mark.parametrize("kind", ["spmm", "spmv"])
@pytest.mark.parametrize("vt,it", TYPES)
@pytest.mark.parametrize("regime", ["cancel", "spread60", "subnormal", "overflow", "grid_cancel", "grid_spread"])
def test_bound_accepts_the_host_oracle(oracle, kind, vt, it, regime):
    rp, ci = _structure(m=120, k=90, avg=10, seed=11)
    k, n = 90, 1 if kind == "spmv" else 5
    rng = np.random.default_rng(7)
    if regime.startswith("grid"):
        kw = dict(cancel=True) if regime == "grid_cancel" else dict(spread=24 if vt == np.float64 else 6)
        g = N.grid_problem(rp, ci, k, n, dtype=vt, alpha=2.0, beta=-0.5, seed=3, **kw)
        A, B, C, alpha, beta = g.A, g.B, g.C, g.alpha, g.beta
    else:
        A, B, C = _general(rng, rp, ci, k, n, regime, vt)
        alpha, beta = (-1 / 3, 0.3) if regime != "overflow" else (0.7, -2 / 7)
    got = _oracle_run(oracle, kind, vt, it, rp, ci, A, B, C, alpha, beta)
    assert np.isfinite(got).all()
    res = N.check_general(got, rp, ci, A, B, C, alpha, beta, vt)
    assert res, res
    if regime.startswith("grid"):
        assert (got == g.expected).all()


@pytest.mark.parametrize("vt", [np.float64, np.float32])
def test_bound_rejects_one_perturbed_output(oracle, vt):
    rp, ci = _structure(m=120, k=90, avg=10, seed=12)
    rng = np.random.default_rng(1)
    A, B, C = _general(rng, rp, ci, 90, 4, "spread60", vt)
    got = _oracle_run(oracle, "spmm", vt, np.int64 if vt == np.float32 else np.int32, rp, ci, A, B, C, 0.1, 0.3)
    a32, b32 = (float(np.float32(0.1)), float(np.float32(0.3))) if vt == np.float32 else (0.1, 0.3)
    bnd = N.bound(rp, ci, A, B, C, a32, b32, vt)
    assert N.check_general(got, rp, ci, A, B, C, 0.1, 0.3, vt)
    bad = got.astype(np.float64)
    bad[17, 2] += 64 * bnd[17, 2]
    res = N.check_bound(bad, N.reference_dd(rp, ci, A, B, C, a32, b32), bnd)
    assert not res and res.where == (17, 2) and res.count == 1 and res.worst > 32, res


def test_bound_rejects_a_float32_alpha(oracle):
    """An ABI or epilogue that demotes alpha to float: the oracle run with float32(alpha) must fail the fp64 bound."""
    rp, ci = _structure(m=120, k=90, avg=10, seed=13)
    rng = np.random.default_rng(2)
    for regime in ("spread60", "cancel"):
        A, B, C = _general(rng, rp, ci, 90, 4, regime)
        for alpha, beta in ((0.1, 0.0), (-1 / 3, 0.3), (7.3e5 + 0.1, -2 / 7)):      # (7.3e5 itself is a float)
            got = _oracle_run(oracle, "spmm", np.float64, np.int32, rp, ci, A, B, C, float(np.float32(alpha)), beta)
            res = N.check_general(got, rp, ci, A, B, C, alpha, beta, np.float64)
            assert not res, (regime, alpha, res)


def _plant_nonfinite(rng, rp, ci, A, B, C, where):
    A, B, C = A.copy(), B.copy(), C.copy()
    specials = [np.inf, -np.inf, np.nan]
    if where == "A":
        idx = rng.choice(len(A), 6, replace=False)
        A[idx] = rng.choice(specials, 6)
    elif where == "B":
        B[rng.choice(B.shape[0], 4, replace=False), rng.integers(0, B.shape[1], 4)] = rng.choice(specials, 4)
        B[0, 0], B[-1, -1] = np.inf, np.nan
    else:
        C[rng.integers(0, C.shape[0], 5), rng.integers(0, C.shape[1], 5)] = rng.choice(specials, 5)
    return A, B, C


@pytest.mark.parametrize("where", ["A", "B", "C"])
@pytest.mark.parametrize("kind", ["spmm", "spmv"])
def test_class_predictor_agrees_with_the_oracle(oracle, where, kind):
    rp, ci = _structure(m=150, k=100, avg=8, seed=21)
    n = 1 if kind == "spmv" else 6
    rng = np.random.default_rng(4)
    A, B, C = _general(rng, rp, ci, 100, n, "spread60")
    B[rng.integers(0, 100, 10), rng.integers(0, n, 10)] = 0.0              # 0 * Inf = NaN must be predicted
    A, B, C = _plant_nonfinite(rng, rp, ci, A, B, C, where)
    for alpha, beta in ((1.5, 0.5), (-0.1, -2.0)) + (((2.0, 0.0),) if where != "C" else ()):
        got = _oracle_run(oracle, kind, np.float64, np.int32, rp, ci, A, B, C, alpha, beta)
        ok, msg = N.check_classes(got, rp, ci, A, B, C, alpha, beta)
        assert ok, msg
        mask = N.finite_mask_inputs(rp, ci, A, B, C, beta)
        assert np.isfinite(got[mask]).all() and mask.sum() > 0
        cls = N.predict_class(rp, ci, A, B, C, alpha, beta)
        assert (cls != 0).any()
        A0, B0, C0 = N.sanitized(A, B, C, beta)
        assert N.check_general(np.where(mask, got, 0.0), rp, ci, A0, B0, C0, alpha, beta, np.float64, mask=mask)
