"""The per-matrix SpMV plan (sblas_hip_spmv_plan_*) on the GPU: oracle parity, bit-identity with the unplanned call
where the plan picks the same kernel, determinism of split rows, refusals, graph capture and the header layer."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ASH85, ROOT

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "s-blas_amd", "bin")


def _families():
    from sblas_amd import synth
    return {
        "nd24k_like": lambda: synth.nd24k_like(0.05)[1],
        "banded7": lambda: synth.banded(40000, 7, 2000),
        "banded48": lambda: synth.banded(12000, 48, 2000),
        "banded73": lambda: synth.banded(12000, 73, 2000),
        "queen_like": lambda: synth.queen_like(12000),
        "powerlaw": lambda: synth.powerlaw(60000, avg=3.2, max_len=5000),
        "powerlaw_split": lambda: synth.powerlaw(250000, avg=3.2, max_len=250000),
        "mixed": lambda: synth.mixed_banded(12000),
        "interleaved": lambda: synth.mixed_banded(12000, interleave=300),
        "random": lambda: synth.random_csr(9000, 7000, 20, empty_every=5, long_row=(4321, 210000)),
        "random_short": lambda: synth.random_csr(9000, 9000, 2, empty_every=3),
    }


# every 256-row tile has the matrix average (queen_like is not such a matrix: its rows near the first and last rows
# lose the clusters the band clips, and those tiles ask for the stream kernel)
UNIFORM = ["nd24k_like", "banded7", "banded48", "banded73"]
_cache = {}


def matrix(name):
    if name not in _cache:
        _cache[name] = _families()[name]()
    return _cache[name]


def upload(cuda, rp, ci, v):
    import torch
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    return d(rp), d(ci), d(v)


def square_cols(rp, ci):
    return max(len(rp) - 1, int(ci.max()) + 1 if len(ci) else 0)


def rel_err(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


@pytest.mark.parametrize("name", sorted(_families()))
def test_planned_call_matches_the_oracle(sblas, oracle, cuda, name):
    import torch
    rp, ci, v = matrix(name)
    rows, cols = len(rp) - 1, square_cols(rp, ci)
    R, Cx, V = upload(cuda, rp, ci, v)
    plan = sblas.SpmvPlan(rows, cols, R, Cx)
    info = plan.info()
    assert info["active"]
    if name in ("powerlaw_split", "random"):
        assert info["split_rows"] >= 1 and info["split_pieces"] >= 200000 // sblas.SPMV_SPLIT_PIECE
    rng = np.random.default_rng(7)
    xh = rng.random(cols) * 2 - 1
    x = torch.from_numpy(xh).to(cuda)
    for alpha, beta in ((1.0, 0.0), (2.5, -0.75), (-1.0, 1.0), (0.0, 3.0)):
        y0 = rng.random(rows)
        y = torch.from_numpy(y0.copy()).to(cuda)
        plan(V, x, alpha, beta, y)
        ref = oracle.spmv(rows, rp, ci, v, xh, y0.copy(), alpha, beta)
        assert rel_err(y.cpu().numpy(), ref) < 1e-10, (name, alpha, beta)
    # beta = 0 never reads y
    y = torch.full((rows,), float("nan"), dtype=torch.float64, device=cuda)
    plan(V, x, 1.5, 0.0, y)
    ref = oracle.spmv(rows, rp, ci, v, xh, np.zeros(rows), 1.5, 0.0)
    got = y.cpu().numpy()
    assert np.isfinite(got).all() and rel_err(got, ref) < 1e-10
    plan.destroy()


@pytest.mark.parametrize("name", UNIFORM)
def test_uniform_families_are_bit_identical_to_the_unplanned_call(sblas, cuda, name):
    import torch
    rp, ci, v = matrix(name)
    rows, cols = len(rp) - 1, square_cols(rp, ci)
    R, Cx, V = upload(cuda, rp, ci, v)
    plan = sblas.SpmvPlan(rows, cols, R, Cx)
    info = plan.info()
    assert info["split_rows"] == 0
    used = [k for k in ("lanes", "stream4096", "stream6144", "segmented", "lds") if info[k]]
    assert len(used) == 1, info
    x = torch.rand(cols, dtype=torch.float64, device=cuda)
    y0 = torch.rand(rows, dtype=torch.float64, device=cuda)
    a, b = y0.clone(), y0.clone()
    sblas.spmv(rows, cols, R, Cx, V, x, 1.25, 0.5, a)
    plan(V, x, 1.25, 0.5, b)
    assert torch.equal(a, b)


def test_split_rows_are_deterministic_and_follow_new_values(sblas, oracle, cuda):
    import torch
    rp, ci, v = matrix("powerlaw_split")
    rows, cols = len(rp) - 1, square_cols(rp, ci)
    R, Cx, V = upload(cuda, rp, ci, v)
    plan = sblas.SpmvPlan(rows, cols, R, Cx)
    assert plan.info()["split_rows"] >= 1
    x = torch.rand(cols, dtype=torch.float64, device=cuda)
    y1 = torch.zeros(rows, dtype=torch.float64, device=cuda)
    y2 = torch.zeros(rows, dtype=torch.float64, device=cuda)
    plan(V, x, 1.0, 0.0, y1)
    plan(V, x, 1.0, 0.0, y2)
    assert torch.equal(y1, y2)
    # new values and a new x: the plan covers the structure only
    v2 = np.random.default_rng(11).random(len(v)) * 4 - 2
    xh = np.random.default_rng(12).random(cols)
    V.copy_(torch.from_numpy(v2))
    x.copy_(torch.from_numpy(xh))
    plan(V, x, 1.0, 0.0, y1)
    ref = oracle.spmv(rows, rp, ci, v2, xh, np.zeros(rows), 1.0, 0.0)
    assert rel_err(y1.cpu().numpy(), ref) < 1e-10


def test_mismatched_calls_are_refused(sblas, cuda):
    import torch
    rp, ci, v = matrix("banded48")
    rows, cols = len(rp) - 1, square_cols(rp, ci)
    R, Cx, V = upload(cuda, rp, ci, v)
    plan = sblas.SpmvPlan(rows, cols, R, Cx)
    x = torch.ones(cols, dtype=torch.float64, device=cuda)
    y = torch.zeros(rows, dtype=torch.float64, device=cuda)
    assert plan.spmv(V, x, 1.0, 0.0, y, rows=rows - 1) == 1
    assert plan.spmv(V, x, 1.0, 0.0, y, nnz=len(ci) - 1) == 1
    assert plan.spmv(V, x, 1.0, 0.0, y) == 0


def test_pinned_variant_gives_an_inactive_plan_that_still_computes(sblas, oracle, cuda, monkeypatch):
    import torch
    rp, ci, v = matrix("queen_like")
    rows, cols = len(rp) - 1, square_cols(rp, ci)
    R, Cx, V = upload(cuda, rp, ci, v)
    monkeypatch.setenv("SBLAS_SPMV_VARIANT", "plain")
    sblas.reload_env()
    try:
        plan = sblas.SpmvPlan(rows, cols, R, Cx)
        assert not plan.info()["active"]
        xh = np.random.default_rng(2).random(cols)
        y = torch.zeros(rows, dtype=torch.float64, device=cuda)
        plan(V, torch.from_numpy(xh).to(cuda), 2.0, 0.0, y)
        ref = oracle.spmv(rows, rp, ci, v, xh, np.zeros(rows), 2.0, 0.0)
        assert rel_err(y.cpu().numpy(), ref) < 1e-10
    finally:
        monkeypatch.delenv("SBLAS_SPMV_VARIANT")
        sblas.reload_env()


def test_validate_refuses_a_bad_structure_at_plan_creation(sblas, cuda, monkeypatch):
    rp, ci, v = matrix("banded7")
    rows = len(rp) - 1
    bad = ci.copy()
    bad[100] = rows + 5  # a column outside the matrix
    R, Cx, V = upload(cuda, rp, bad, v)
    monkeypatch.setenv("SBLAS_VALIDATE", "1")
    sblas.reload_env()
    try:
        with pytest.raises(sblas.SblasError):
            sblas.SpmvPlan(rows, rows, R, Cx)
    finally:
        monkeypatch.delenv("SBLAS_VALIDATE")
        sblas.reload_env()


def test_planned_call_replays_in_a_graph_with_a_new_x(sblas, oracle, cuda):
    import torch
    rp, ci, v = matrix("random")
    rows, cols = len(rp) - 1, square_cols(rp, ci)
    R, Cx, V = upload(cuda, rp, ci, v)
    plan = sblas.SpmvPlan(rows, cols, R, Cx)
    x = torch.rand(cols, dtype=torch.float64, device=cuda)
    y = torch.zeros(rows, dtype=torch.float64, device=cuda)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        plan(V, x, 1.0, 0.0, y, stream=s)      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan(V, x, 1.0, 0.0, y)
    xh = np.random.default_rng(4).random(cols)
    x.copy_(torch.from_numpy(xh))
    g.replay()
    torch.cuda.synchronize()
    ref = oracle.spmv(rows, rp, ci, v, xh, np.zeros(rows), 1.0, 0.0)
    assert rel_err(y.cpu().numpy(), ref) < 1e-10


@pytest.mark.parametrize("gpus", [1, 2])
def test_header_layer_runs_planned_under_the_switch(sblas, cuda, gpus):
    for alpha, beta in ((1.0, 1.0), (3.0, 4.0)):
        p = subprocess.run([os.path.join(BIN, "spmv_test"), ASH85, str(alpha), str(beta), str(gpus)], capture_output=True,
                           text=True, timeout=600, env=dict(os.environ, SBLAS_SPMV_PLAN="1"))
        out = p.stdout + p.stderr
        assert p.returncode == 0 and "Validation = True" in out, out[-1500:]
        assert out.count("SpMV plan: active") == gpus, out[-1500:]
    # without the switch: no plan
    p = subprocess.run([os.path.join(BIN, "spmv_test"), ASH85, "1", "1", str(gpus)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "Validation = True" in p.stdout and "SpMV plan" not in p.stdout
