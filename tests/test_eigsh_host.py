"""The eigenvalue plan's host rule (eigsh_rule.cpp; no GPU): the Jacobi loop, the whole Ritz step and the rotation -- built
from the very functions the device compiles -- against their restatements in Python (tests/eigsh_numerics.py) with ==,
the Jacobi loop against LAPACK, the method itself as a numpy loop over the host references, the limits, the launch counts,
the refusals of the Python layer that need no GPU, and the rule check under the host sanitizers.

Measured here on the CPU (the figures DESIGN.md 3.40 quotes), over the finite matrices of eigsh_numerics.ritz_cases():
  |theta - eigvalsh(T)| <= 4.36 eps |T|_F, |Y^T Y - I| <= 181 eps, |T Y - Y Theta|_F <= 11.54 eps |T|_F, at most 8 sweeps
  but for the matrix graded over sixteen decades, which runs into the cap of 24.  The bounds below are four times these:
  LAPACK's own error is of the same order.
  The numpy loop over the host references, rtol 1e-10, the library's hashed start vector: every named case converges in
  at most 57 restarts (the cap is 300); the largest residual is 0.42 of 2 max(rtol |theta|, atol) + n eps |A|_F, that is
  0.84 of the bound with the factor 1 -- too close to the edge to tighten, so the factor stays 2."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import eigsh_numerics as EN
import krylov_numerics as KN
from conftest import ROOT

EIG_BOUND, ORTH_BOUND, RES_BOUND = 4 * 4.36, 4 * 181.0, 4 * 11.54
STATUS = {0: "running", 1: "converged", 2: "breakdown", 3: "limit"}


def test_limits_and_launches(sblas):
    lim = sblas.eigsh_limits()
    assert (lim["max_ncv"], lim["default_ncv"], lim["ld"], lim["max_sweeps"], lim["block_slots"]) == (64, 20, 64, EN.MAX_SWEEPS, 16)
    assert lim["t"] == 0 and lim["y"] == 64 * 64 and lim["theta"] == 2 * 64 * 64 and lim["q"] == lim["rho"] + 64
    assert lim["matrix_doubles"] == lim["c"] + 72 and lim["rotate_rows"] == 256
    text = open(os.path.join(ROOT, "include", "sblas_hip_eigsh.h")).read()
    assert "#define SBLAS_EIGSH_MATRIX_DOUBLES %d\n" % lim["matrix_doubles"] in text
    for ncv, keep in ((20, 12), (8, 4), (64, 37), (64, 63), (2, 1)):
        got = sblas.eigsh_launches(ncv, keep)
        # a step: SpMV, dots, fold, project, dots, fold, project, fold, normalise; start: v0, fold, normalise and keep steps
        assert got == dict(step=9, start=3 + 9 * keep, cycle=9 * (ncv - keep) + 2, tail=2)
    for ncv, keep in ((65, 12), (20, 20), (20, 0), (1, 1)):
        with pytest.raises(sblas.SblasError):
            sblas.eigsh_launches(ncv, keep)


def test_refusals_that_need_no_gpu(sblas):
    E = sblas.SblasError
    size = sblas._eigsh_sizes
    assert size(1000, 4, None, None, "LA") == (20, 12) and size(1000, 30, None, None, "SA") == (61, 45)
    assert size(1000, 40, None, None, "LM") == (64, 52) and size(10, 4, None, None, "LA") == (9, 6)
    assert size(1000, 4, 20, 4, "LA") == (20, 4) and size(1000, 4, 20, 19, "LA") == (20, 19) and size(66, 63, 64, 63, "LA") == (64, 63)
    for n, k, ncv, keep, which, word in ((1000, 20, 20, None, "LA", "below ncv"), (1000, 4, 65, None, "LA", "at most 64"),
                                         (20, 4, 20, None, "LA", "below n"), (1000, 4, 20, 3, "LA", "keep"),
                                         (1000, 4, 20, 20, "LA", "keep"), (1000, 4, None, None, "BE", "which"),
                                         (1000, 0, None, None, "LA", "at least 1"), (1000, 4.0, None, None, "LA", "integer"),
                                         (1000, True, None, None, "LA", "integer"), (4, 4, None, None, "LA", "below ncv")):
        with pytest.raises(E, match=word):
            size(n, k, ncv, keep, which)
        with pytest.raises(E, match=word):                                   # create refuses before it looks at a tensor
            sblas.EigshPlan(n, None, None, k, ncv=ncv, which=which, keep=keep)
    for call in (lambda: sblas.eigsh_jacobi_ref(np.zeros((65, 65))), lambda: sblas.eigsh_jacobi_ref(np.zeros((2, 3))),
                 lambda: sblas.eigsh_ritz_ref(np.eye(3), 1.0, 2, 1), lambda: sblas.eigsh_ritz_ref(np.eye(3), 1.0, 1, 64),
                 lambda: sblas.eigsh_ritz_ref(np.eye(3), 1.0, 1, 2, which="XX"), lambda: sblas.eigsh_rotate_ref(np.zeros((3, 5)), np.zeros((3, 1))),
                 lambda: sblas.eigsh_rotate_ref(np.zeros((4, 5)), np.zeros((3, 4)))):
        with pytest.raises(E):
            call()
    assert set(sblas.EXPORTS_EIGSH) >= {"sblas_hip_eigsh_rotate_f64", "sblas_hip_eigsh_ritz_f64", "sblas_hip_eigsh_plan_create"}
    for name in sblas.EXPORTS_EIGSH:
        getattr(sblas.lib(), name)


def test_the_librarys_defaults_are_the_python_layers(sblas):
    import ctypes as C
    for n, k in ((1000, 1), (1000, 4), (1000, 9), (1000, 10), (1000, 30), (1000, 32), (1000, 63), (10, 4), (22, 4), (3, 1), (66, 40)):
        out = (C.c_int64 * 2)()
        assert sblas.lib().sblas_eigsh_sizes(n, k, 0, 0, out) == 0 and (int(out[0]), int(out[1])) == sblas._eigsh_sizes(n, k, None, None, "LA")
        for keep in (k, int(out[0]) - 1):
            assert sblas.lib().sblas_eigsh_sizes(n, k, int(out[0]), keep, out) == 0 and int(out[1]) == keep
    for n, k, ncv, keep in ((1000, 20, 20, 0), (1000, 4, 65, 0), (20, 4, 20, 0), (1000, 4, 20, 3), (1000, 4, 20, 20), (1000, 0, 0, 0), (4, 4, 0, 0)):
        out = (C.c_int64 * 2)()
        assert sblas.lib().sblas_eigsh_sizes(n, k, ncv, keep, out) == 1, (n, k, ncv, keep)


def test_step_ref_stores_the_column_and_reads_beta(sblas):
    rng = np.random.default_rng(3)
    for j in (0, 1, 19, 63):
        h, T = rng.standard_normal(j + 1), rng.standard_normal((64, 64))
        want = T.copy()
        want[:j + 1, j] = want[j, :j + 1] = h
        got = sblas.eigsh_step_ref(j, h, 0.5, T=T, matvecs=7)
        assert KN.same_bits(got["T"], want)
        assert (got["columns"], got["matvecs"], got["beta"], got["forms"], got["invariant"], got["status"]) == (j + 1, 8, 0.5, True, False, "running")
        got = sblas.eigsh_step_ref(j, h, 0.0, T=T)                          # an invariant subspace: the column counts, nothing is divided
        assert (got["columns"], got["forms"], got["invariant"], got["status"]) == (j + 1, False, True, "running")
        for beta in (np.inf, np.nan):
            got = sblas.eigsh_step_ref(j, h, beta, T=T)
            assert (got["columns"], got["forms"], got["status"], got["breakdown"], got["matvecs"]) == (j, False, "breakdown", "beta", 1)
    for call in (lambda: sblas.eigsh_step_ref(64, np.zeros(65), 1.0), lambda: sblas.eigsh_step_ref(2, np.zeros(2), 1.0),
                 lambda: sblas.eigsh_step_ref(2, np.zeros(3), 1.0, T=np.zeros((2, 2)))):
        with pytest.raises(sblas.SblasError):
            call()


@pytest.mark.parametrize("mm", EN.RITZ_SIZES)
def test_jacobi_ref_is_the_written_rule_and_meets_lapack(sblas, mm):
    worst = [0.0, 0.0, 0.0]
    for n_kind, kind in enumerate(("random", "diagonal", "identity", "rank_one", "arrow")):
        for scale in (1.0, 1e150, 1e-150):
            T = EN.small_matrix(kind, mm, 100 * mm + n_kind) * scale
            got = sblas.eigsh_jacobi_ref(T)
            theta, Y, sweeps = EN.jacobi_py(T)
            assert KN.same_bits(got["theta"], theta) and KN.same_bits(got["Y"], Y) and got["sweeps"] == sweeps, (kind, scale)
            assert sweeps < EN.MAX_SWEEPS and (kind not in ("diagonal", "identity") or sweeps == 0)
            unit = T / scale                                                  # the norms below would overflow or underflow
            nrm = np.linalg.norm(unit)
            e = np.abs(np.sort(got["theta"] / scale) - np.linalg.eigvalsh(unit)).max() / (EN.EPS * nrm)
            o = np.abs(got["Y"].T @ got["Y"] - np.eye(mm)).max() / EN.EPS
            r = np.linalg.norm(unit @ got["Y"] - got["Y"] * (got["theta"] / scale)) / (EN.EPS * nrm)
            worst = [max(worst[0], e), max(worst[1], o), max(worst[2], r)]
    print("mm = %d: |theta - lapack| %.3g eps |T|, |Y^T Y - I| %.3g eps, |T Y - Y Theta| %.3g eps |T|" % ((mm,) + tuple(worst)))
    assert worst[0] <= EIG_BOUND and worst[1] <= ORTH_BOUND and worst[2] <= RES_BOUND, worst


def test_ritz_ref_is_the_written_step(sblas):
    seen, worst = {}, [0.0, 0.0, 0.0]
    for label, T, beta, k, keep, which, kw in EN.ritz_cases():
        got = sblas.eigsh_ritz_ref(T, beta, k, keep, which, **kw)
        py = dict(kw)
        if "status" in py:
            py["status"] = STATUS[py["status"]]
        EN.same_ritz(got, EN.ritz_py(T, beta, k, keep, which, **py))
        seen[got["status"]] = seen.get(got["status"], 0) + 1
        mm = T.shape[0]
        if got["act"]:
            order = EN.order_py(got["theta"], which)
            assert order == list(range(mm)), (label, "the Ritz values come in the order of which")
            assert got["kk"] == min(keep, mm) and got["columns"] == got["kk"] and got["restarts"] == kw.get("restarts", 0) + 1
            if np.isfinite(T).all() and label.split("-")[0] == "mixed":     # the graded matrix: the cap ends the loop, the answer holds
                nrm = np.linalg.norm(T)
                e = np.abs(np.sort(got["theta"]) - np.linalg.eigvalsh(T)).max() / (EN.EPS * nrm)
                Y = got["Y"][:mm, :mm]
                worst = [max(worst[0], e), max(worst[1], np.abs(Y.T @ Y - np.eye(mm)).max() / EN.EPS), 0.0]
        else:
            assert got["restarts"] == kw.get("restarts", 0) and (got["status"] == "breakdown") == (kw.get("status", 0) == 0)
    assert worst[0] <= EIG_BOUND and worst[1] <= ORTH_BOUND, worst
    assert set(seen) == {"running", "converged", "breakdown", "limit"}, seen
    # the named outcomes
    arrow = EN.small_matrix("arrow", 20, 3)
    ref = lambda **kw: sblas.eigsh_ritz_ref(arrow, kw.pop("beta", 1.0), 4, 12, "LA", **kw)
    assert ref(beta=0.0, invariant=True)["status"] == "converged" and (ref(beta=0.0, invariant=True)["residuals"] == 0.0).all()
    short = sblas.eigsh_ritz_ref(arrow[:3, :3], 0.0, 4, 12, "LA", invariant=True)
    assert (short["status"], short["breakdown"], short["mm"], short["kk"], short["act"]) == ("breakdown", "invariant", 3, 3, 1)
    assert ref(restarts=1, max_restarts=2)["status"] == "limit" and ref(restarts=0, max_restarts=2)["status"] == "running"
    assert ref(beta=np.nan)["status"] == "running" and ref(beta=np.nan)["converged"] == 0      # a NaN never converges
    bad = arrow.copy()
    bad[5, 5] = np.nan
    got = sblas.eigsh_ritz_ref(bad, 1.0, 4, 12, "LA")
    assert (got["status"], got["breakdown"], got["act"], got["restarts"]) == ("breakdown", "t", 0, 0)
    assert KN.same_bits(got["T"][:20, :20], bad)                            # nothing else changes


@pytest.mark.parametrize("n", [1, 37])
def test_rotate_ref_is_the_written_order(sblas, n):
    rng = np.random.default_rng(n)
    for mm in (1, 2, 3, 20, 63, 64):
        V = rng.standard_normal((mm + 1, n)) * 10.0 ** rng.integers(-3, 4, (mm + 1, n))
        for keep in sorted({1, max(mm - 1, 1), mm}):
            Q = rng.standard_normal((mm, keep))
            got = sblas.eigsh_rotate_ref(V, Q)
            assert KN.same_bits(got, EN.rotate_py(V, Q)), (mm, keep)
            assert KN.same_bits(got[keep], V[mm]) and KN.same_bits(got[keep + 1:], V[keep + 1:])


@pytest.mark.parametrize("name,which,k,ncv", EN.CASES)
def test_the_numpy_loop_over_the_host_references_finds_the_eigenpairs(sblas, name, which, k, ncv):
    """|theta_i - lambda_i| <= |A x_i - theta_i x_i| + n eps |A|_F: a symmetric matrix has an eigenvalue within the residual
    of any Ritz value, and the second term is LAPACK's documented error.  |A x_i - theta_i x_i| <= 2 max(rtol |theta_i|,
    atol) + n eps |A|_F: the estimate |beta y| the test was met with is the residual in exact arithmetic."""
    A = EN.dense(name)
    n = A.shape[0]
    out = EN.numpy_eigsh(A, k, ncv, which, sblas.cheby_start_ref(n, seed=0), rtol=1e-10, ritz_ref=sblas)
    assert out["status"] == "converged" and out["restarts"] <= 300 and out["converged"] == k, out
    worst = EN.check_pairs(A, np.linalg.eigvalsh(A), which, out["theta"], np.stack(out["V"][:k]), 1e-10, 0.0)
    print("%s %s k=%d ncv=%d: %d restarts, %d matvecs, worst ratios %.3g %.3g" % (name, which, k, ncv, out["restarts"], out["matvecs"], worst[0], worst[1]))


def test_the_numpy_loop_at_its_edges(sblas):
    A = EN.dense("grid")
    n = A.shape[0]
    v0 = sblas.cheby_start_ref(n, seed=0)
    lim = EN.numpy_eigsh(A, 4, 20, "SA", v0, rtol=1e-10, max_restarts=2, ritz_ref=sblas)
    assert (lim["status"], lim["restarts"]) == ("limit", 2)
    assert EN.numpy_eigsh(A, 4, 20, "SA", np.zeros(n), ritz_ref=sblas)["breakdown"] == "v0"
    e = np.zeros(n)
    e[7] = 3.0                                                              # an eigenvector of a diagonal matrix: beta == 0 at once
    D = np.diag(np.arange(1.0, n + 1.0))
    one = EN.numpy_eigsh(D, 1, 20, "LA", e, ritz_ref=sblas)
    assert (one["status"], one["columns"], one["matvecs"]) == ("converged", 1, 1) and one["theta"][0] == 8.0
    two = EN.numpy_eigsh(D, 2, 20, "LA", e, ritz_ref=sblas)
    assert (two["status"], two["breakdown"], two["columns"]) == ("breakdown", "invariant", 1)
    bad = A.copy()
    bad[3, 3] = np.nan
    assert EN.numpy_eigsh(bad, 4, 20, "LA", v0, ritz_ref=sblas)["breakdown"] == "beta"


def test_the_rule_check_runs_clean_under_the_sanitizers(tmp_path):
    """tools/eigsh_rule_check.cpp, host code only and a program of its own, under the address and undefined-behaviour
    sanitizers of every host compiler there is"""
    found = [p for p in (shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++", shutil.which("g++")) if p and os.path.exists(p)]
    assert found, "no host compiler"
    src = [os.path.join(ROOT, "tools", "eigsh_rule_check.cpp"), os.path.join(ROOT, "s-blas_amd", "csrc", "eigsh_rule.cpp")]
    for k, cxx in enumerate(found):
        exe = str(tmp_path / ("eigsh_rule_check_%d" % k))
        subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-w", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                              + src + ["-o", exe])
        done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        assert done.returncode == 0, done.stdout.decode()
        assert b"eigsh rule check: ok" in done.stdout
