"""Split SpMM plans (sblas_hip_spmm_plan_create_split) on the GPU: oracle parity for every staged width and order pair,
alpha / beta, a row block with range staging, bit-identity of the rows that are not split, determinism, graph replay,
long rows the LDS-tiled kernel owns, and the header layer under SBLAS_SPMM_SPLIT=1."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "s-blas_amd", "bin")
COL, ROW = 0, 1
_cache = {}


def matrix(name):
    """(rows, cols, rp, ci, v)"""
    if name not in _cache:
        from sblas_amd import synth
        if name == "powerlaw":      # columns ascending and distinct; a 250 000-entry row and a few more of 16 384+
            rp, ci, v = synth.powerlaw(250000, avg=40, max_len=250000)
            _cache[name] = (250000, 250000, rp, ci, v)
        elif name == "random":      # unsorted columns, duplicates (210 000 draws over 250 000 columns); the columns are
            # spread so thin that every panel goes to the direct kernels (over a few thousand columns the long row's panel
            # would be the LDS-tiled kernel's, and not split: test_long_row_in_an_lds_tiled_panel_is_not_split)
            rp, ci, v = synth.random_csr(9000, 250000, 30, long_row=(4321, 210000))
            _cache[name] = (9000, 250000, rp, ci, v)
        elif name == "banded_long":  # a band every panel of which the LDS-tiled kernel takes, one long row inside it
            _cache[name] = banded_long_row()
    return _cache[name]


def banded_long_row(rows=40000, half=32, r0=20000, reps=12):
    """rows of 64 consecutive columns around the diagonal; row r0 lists 2000 columns around r0, each `reps` times"""
    lens = np.full(rows, 2 * half, np.int64)
    lens[r0] = 2000 * reps
    rp = np.zeros(rows + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    ci = np.empty(int(rp[-1]), np.int32)
    other = np.arange(rows) != r0
    centre = np.clip(np.arange(rows), half, rows - half)[other]
    idx = (rp[:-1][other][:, None] + np.arange(2 * half)[None, :]).ravel()
    ci[idx] = (centre[:, None] + np.arange(-half, half)[None, :]).ravel()
    ci[rp[r0]:rp[r0 + 1]] = np.repeat(np.arange(r0 - 1000, r0 + 1000, dtype=np.int32), reps)   # ascending, duplicated
    v = np.random.default_rng(5).random(len(ci)) * 2 - 1
    return rows, rows, rp.astype(np.int32), ci, v


@pytest.fixture(scope="module")
def env(sblas, oracle, cuda):
    import torch
    return sblas, oracle, torch, cuda


def upload(torch, cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def rel_err(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def workspace(S, torch, cuda, rows, cols, nnz, n):
    return torch.empty(S.spmm_workspace_bytes(rows, cols, nnz, n) // 8 + 1, dtype=torch.float64, device=cuda)


def split_rows_of(S, rp, **kw):
    return S.spmm_split_classify(rp, **kw)[1][:, 0]


@pytest.fixture
def env_switch():
    """set SBLAS_* switches for one test; the library re-reads them"""
    import sblas_amd as S
    saved = {}

    def set_(name, value):
        saved.setdefault(name, os.environ.get(name))
        os.environ[name] = str(value)
        S.reload_env()
    yield set_
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    S.reload_env()


@pytest.mark.parametrize("name,n", [("powerlaw", 128), ("powerlaw", 64), ("random", 64)])
def test_split_plan_matches_the_oracle(env, name, n):
    S, O, torch, cuda = env
    rows, cols, rp, ci, v = matrix(name)
    R, Cx, V = upload(torch, cuda, rp, ci, v)
    plan = S.SpmmPlan(rows, cols, R, Cx, n, split=True)
    info = plan.split_info()
    assert info["split_rows"] >= 1 and info["pieces"] >= 200000 // S.SPMM_SPLIT_PIECE, info
    rng = np.random.default_rng(3)
    Bh = rng.random(cols * n) * 2 - 1
    B, = upload(torch, cuda, Bh)
    ws = workspace(S, torch, cuda, rows, cols, len(ci), n)
    for alpha, beta in ((1.0, 0.0), (2.5, -0.75)):
        C0 = rng.random(rows * n)
        C, = upload(torch, cuda, C0)
        plan.spmm(V, B, cols, n, alpha, beta, C, rows, ws)
        ref = O.spmm_omp(rows, cols, n, rp, ci, v, Bh, C0.copy(), alpha, beta)
        assert rel_err(C.cpu().numpy(), ref) < 1e-10, (name, n, alpha, beta)
    plan.destroy()


@pytest.mark.parametrize("n", [1, 8, 16, 32, 64, 128, 256, 300])
def test_every_width_and_order_pair(env, env_switch, n):
    S, O, torch, cuda = env
    rows, cols, rp, ci, v = matrix("random")
    if n == 300:   # three column chunks: 128 + 128 (planned, split) and 44 (another staged width: unplanned)
        env_switch("SBLAS_SPMM_MAX_BT_BYTES", (cols + 1) * 8 * 128)
    R, Cx, V = upload(torch, cuda, rp, ci, v)
    plan = S.SpmmPlan(rows, cols, R, Cx, n, split=True)
    assert plan.info()["active"] and plan.split_info()["split_rows"] == 1, (plan.info(), plan.split_info())
    rng = np.random.default_rng(n)
    Bh = rng.random((cols, n)) * 2 - 1     # logical cols x n
    C0 = rng.random((rows, n))
    ref = O.spmm_omp(rows, cols, n, rp, ci, v, Bh.ravel(order="F").copy(), C0.ravel(order="F").copy(), 1.5, 0.5)
    ref = ref.reshape(n, rows).T
    ws = workspace(S, torch, cuda, rows, cols, len(ci), n)
    for ob in (COL, ROW):
        for oc in (COL, ROW):
            B, = upload(torch, cuda, Bh.ravel(order="F" if ob == COL else "C"))
            C, = upload(torch, cuda, C0.ravel(order="F" if oc == COL else "C"))
            plan.spmm_ordered(V, B, cols if ob == COL else n, ob, n, 1.5, 0.5, C, rows if oc == COL else n, oc, ws)
            got = C.cpu().numpy().reshape((n, rows) if oc == COL else (rows, n))
            got = got.T if oc == COL else got
            assert rel_err(got, ref) < 1e-10, (n, ob, oc)
    plan.destroy()


def test_beta_zero_never_reads_c_and_alpha_zero_scales(env):
    S, O, torch, cuda = env
    rows, cols, rp, ci, v = matrix("powerlaw")
    n = 64
    R, Cx, V = upload(torch, cuda, rp, ci, v)
    plan = S.SpmmPlan(rows, cols, R, Cx, n, split=True)
    assert plan.split_info()["split_rows"] >= 1
    Bh = np.random.default_rng(9).random(cols * n)
    B, = upload(torch, cuda, Bh)
    ws = workspace(S, torch, cuda, rows, cols, len(ci), n)
    C = torch.full((rows * n,), float("nan"), dtype=torch.float64, device=cuda)
    plan.spmm(V, B, cols, n, 1.25, 0.0, C, rows, ws)
    got = C.cpu().numpy()
    ref = O.spmm_omp(rows, cols, n, rp, ci, v, Bh, np.zeros(rows * n), 1.25, 0.0)
    assert np.isfinite(got).all() and rel_err(got, ref) < 1e-10
    C0 = np.random.default_rng(10).random(rows * n)
    C, = upload(torch, cuda, C0)
    plan.spmm(V, B, cols, n, 0.0, 2.0, C, rows, ws)
    assert np.array_equal(C.cpu().numpy(), 2.0 * C0)
    plan.destroy()


def test_row_block_with_range_staging(env):
    """a method-2 row block: rows [r0, r1) of the power-law matrix, all of its columns -- range staging pays"""
    S, O, torch, cuda = env
    rows, cols, rp, ci, v = matrix("powerlaw")
    longest = int(np.argmax(np.diff(rp)))
    r0 = max(0, longest - 10000)
    r1 = r0 + 20000
    brp = (rp[r0:r1 + 1] - rp[r0]).astype(np.int32)
    bci, bv = ci[rp[r0]:rp[r1]], v[rp[r0]:rp[r1]]
    n = 128
    R, Cx, V = upload(torch, cuda, brp, bci, bv)
    plan = S.SpmmPlan(r1 - r0, cols, R, Cx, n, split=True)
    assert plan.info()["stage_range"] and plan.split_info()["split_rows"] >= 1, (plan.info(), plan.split_info())
    Bh = np.random.default_rng(12).random(cols * n) - 0.5
    B, = upload(torch, cuda, Bh)
    C0 = np.random.default_rng(13).random((r1 - r0) * n)
    C, = upload(torch, cuda, C0)
    ws = workspace(S, torch, cuda, r1 - r0, cols, len(bci), n)
    plan.spmm(V, B, cols, n, 1.0, 1.0, C, r1 - r0, ws)
    ref = O.spmm_omp(r1 - r0, cols, n, brp, bci, bv, Bh, C0.copy(), 1.0, 1.0)
    assert rel_err(C.cpu().numpy(), ref) < 1e-10
    plan.destroy()


@pytest.mark.parametrize("split_min,piece", [(0, 0), (5000, 1000)])
def test_split_info_agrees_with_the_host_classifier(env, split_min, piece):
    S, O, torch, cuda = env
    rows, cols, rp, ci, v = matrix("powerlaw")
    n = 128
    R, Cx, V = upload(torch, cuda, rp, ci, v)
    plan = S.SpmmPlan(rows, cols, R, Cx, n, split=True, split_min=split_min, piece=piece)
    info = plan.split_info()
    # uniform random columns over 250 000: every panel goes to the direct kernels, so no panel is masked out
    pieces, srows = S.spmm_split_classify(rp, split_min=split_min, piece=piece)
    lens = np.diff(rp.astype(np.int64))
    assert info == dict(split_rows=len(srows), pieces=len(pieces), split_nnz=int(lens[srows[:, 0]].sum()),
                        partial_bytes=len(pieces) * plan.info()["ldbt"] * 8), info
    plain = S.SpmmPlan(rows, cols, R, Cx, n)
    assert plain.split_info() == dict(split_rows=0, pieces=0, split_nnz=0, partial_bytes=0)
    assert {k: x for k, x in plain.info().items()} == plan.info()
    plan.destroy()
    plain.destroy()


@pytest.mark.parametrize("name,n", [("powerlaw", 128), ("powerlaw", 32), ("random", 8), ("random", 16)])
def test_unsplit_rows_are_bit_identical_and_calls_repeat(env, name, n):
    S, O, torch, cuda = env
    rows, cols, rp, ci, v = matrix(name)
    R, Cx, V = upload(torch, cuda, rp, ci, v)
    plain = S.SpmmPlan(rows, cols, R, Cx, n)
    plan = S.SpmmPlan(rows, cols, R, Cx, n, split=True)
    assert plan.split_info()["split_rows"] >= 1
    B = torch.rand(cols * n, dtype=torch.float64, device=cuda)
    C0 = torch.rand(rows * n, dtype=torch.float64, device=cuda)
    ws = workspace(S, torch, cuda, rows, cols, len(ci), n)
    a, b, c = C0.clone(), C0.clone(), C0.clone()
    plain.spmm(V, B, cols, n, 1.5, -0.5, a, rows, ws)
    plan.spmm(V, B, cols, n, 1.5, -0.5, b, rows, ws)
    plan.spmm(V, B, cols, n, 1.5, -0.5, c, rows, ws)
    assert torch.equal(b, c)
    A, Bs = a.cpu().numpy().reshape(n, rows), b.cpu().numpy().reshape(n, rows)
    split = np.zeros(rows, bool)
    split[split_rows_of(S, rp)] = True
    assert np.array_equal(A[:, ~split], Bs[:, ~split])
    assert rel_err(Bs[:, split], A[:, split]) < 1e-12
    plan.destroy()
    plain.destroy()


def test_no_split_rows_is_the_plain_plan(env):
    S, O, torch, cuda = env
    from sblas_amd import synth
    rows, (rp, ci, v) = synth.nd24k_like(0.2)
    n = 64
    R, Cx, V = upload(torch, cuda, rp, ci, v)
    plain = S.SpmmPlan(rows, rows, R, Cx, n)
    plan = S.SpmmPlan(rows, rows, R, Cx, n, split=True)
    assert plan.split_info()["split_rows"] == 0 and plan.info() == plain.info()
    B = torch.rand(rows * n, dtype=torch.float64, device=cuda)
    a, b = torch.ones(rows * n, dtype=torch.float64, device=cuda), torch.ones(rows * n, dtype=torch.float64, device=cuda)
    ws = workspace(S, torch, cuda, rows, rows, len(ci), n)
    plain.spmm(V, B, rows, n, 1.0, 1.0, a, rows, ws)
    plan.spmm(V, B, rows, n, 1.0, 1.0, b, rows, ws)
    assert torch.equal(a, b)


def test_graph_replay_equals_the_eager_call(env):
    S, O, torch, cuda = env
    rows, cols, rp, ci, v = matrix("powerlaw")
    n = 64
    R, Cx, V = upload(torch, cuda, rp, ci, v)
    plan = S.SpmmPlan(rows, cols, R, Cx, n, split=True)
    assert plan.split_info()["split_rows"] >= 1
    B = torch.rand(cols * n, dtype=torch.float64, device=cuda)
    C = torch.zeros(rows * n, dtype=torch.float64, device=cuda)
    ws = workspace(S, torch, cuda, rows, cols, len(ci), n)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        plan.spmm(V, B, cols, n, 1.0, 0.0, C, rows, ws, stream=s)   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.spmm(V, B, cols, n, 1.0, 0.0, C, rows, ws)
    B.copy_(torch.rand(cols * n, dtype=torch.float64, device=cuda))
    g.replay()
    torch.cuda.synchronize()
    eager = torch.zeros_like(C)
    plan.spmm(V, B, cols, n, 1.0, 0.0, eager, rows, ws)
    torch.cuda.synchronize()
    assert torch.equal(C, eager)
    del g
    plan.destroy()


def test_long_row_in_an_lds_tiled_panel_is_not_split(env):
    S, O, torch, cuda = env
    rows, cols, rp, ci, v = matrix("banded_long")
    n = 64
    assert len(split_rows_of(S, rp)) == 1            # long enough to split, if its panel went to the direct kernels
    R, Cx, V = upload(torch, cuda, rp, ci, v)
    plain = S.SpmmPlan(rows, cols, R, Cx, n)
    plan = S.SpmmPlan(rows, cols, R, Cx, n, split=True)
    assert plan.info()["windowed"] > 0 and plan.split_info()["split_rows"] == 0, (plan.info(), plan.split_info())
    B = torch.rand(cols * n, dtype=torch.float64, device=cuda)
    a = torch.zeros(rows * n, dtype=torch.float64, device=cuda)
    b = torch.zeros(rows * n, dtype=torch.float64, device=cuda)
    ws = workspace(S, torch, cuda, rows, cols, len(ci), n)
    plain.spmm(V, B, cols, n, 1.0, 0.0, a, rows, ws)
    plan.spmm(V, B, cols, n, 1.0, 0.0, b, rows, ws)
    assert torch.equal(a, b)
    ref = O.spmm_omp(rows, cols, n, rp, ci, v, B.cpu().numpy(), np.zeros(rows * n), 1.0, 0.0)
    assert rel_err(b.cpu().numpy(), ref) < 1e-10


# Every direct kernel a plan can pick, forced through its SKIP instantiation, with a non-default split_min / piece (the
# long row in 1000-entry pieces): the switch or matrix average that selects each branch of spmm_rowpanel.
BRANCHES = {
    # name: (rows, avg, long row, n, switches)
    "rows8": (9000, 30, 210000, 8, {"SBLAS_ROWS8_MIN_AVG": "1"}),       # 8 staged columns, a wave per row
    "narrow8": (9000, 30, 210000, 8, {}),                               # 8 staged columns, lane groups (avg 53 < 256)
    "narrow16": (20000, 14, 100000, 16, {}),                            # 16 staged columns, short rows (avg 19 < 24)
    "narrow32": (20000, 9, 100000, 32, {}),                             # 32 staged columns, short rows (avg 14 < 16)
    "dpp16": (9000, 30, 210000, 16, {}),                                # 16 staged columns, row per wave
    "dpp64_n32": (9000, 30, 210000, 32, {"SBLAS_SPMM_MIN_LDBT": "64"}),  # 64 staged columns, 32-column sweep
    "dpp64": (9000, 60, 210000, 64, {}),                                # 64 staged columns, row per wave (avg 83 >= 56)
    "rows64": (9000, 30, 210000, 64, {}),                               # 64 staged columns, four rows per wave (avg 53)
    "dpp128": (9000, 30, 210000, 128, {}),                              # 128-column tiles
}


@pytest.mark.parametrize("branch", sorted(BRANCHES))
def test_every_direct_kernel_skips_split_rows(env, env_switch, branch):
    S, O, torch, cuda = env
    from sblas_amd import synth
    rows, avg, long_len, n, switches = BRANCHES[branch]
    cols = 250000
    for k, val in switches.items():
        env_switch(k, val)
    rp, ci, v = synth.random_csr(rows, cols, avg, long_row=(4321, long_len))
    R, Cx, V = upload(torch, cuda, rp, ci, v)
    plain = S.SpmmPlan(rows, cols, R, Cx, n)
    plan = S.SpmmPlan(rows, cols, R, Cx, n, split=True, split_min=5000, piece=1000)
    info = plan.split_info()
    assert plan.info()["active"] and info["split_rows"] == 1 and info["pieces"] == -(-long_len // 1000), (plan.info(), info)
    if "SBLAS_SPMM_MIN_LDBT" in switches:
        assert plan.info()["ldbt"] == 64
    rng = np.random.default_rng(21)
    Bh = rng.random(cols * n) * 2 - 1
    C0 = rng.random(rows * n)
    B, a, b = upload(torch, cuda, Bh, C0, C0)
    ws = workspace(S, torch, cuda, rows, cols, len(ci), n)
    plain.spmm(V, B, cols, n, 1.5, -0.5, a, rows, ws)
    plan.spmm(V, B, cols, n, 1.5, -0.5, b, rows, ws)
    ref = O.spmm_omp(rows, cols, n, rp, ci, v, Bh, C0.copy(), 1.5, -0.5)
    got = b.cpu().numpy()
    assert rel_err(got, ref) < 1e-10
    split = np.zeros(rows, bool)
    split[split_rows_of(S, rp, split_min=5000, piece=1000)] = True
    assert np.array_equal(a.cpu().numpy().reshape(n, rows)[:, ~split], got.reshape(n, rows)[:, ~split])
    plan.destroy()
    plain.destroy()


def write_mtx(path, rows, cols, rp, ci, v):
    r = np.repeat(np.arange(rows), np.diff(rp))
    with open(path, "w") as f:
        f.write("%%%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (rows, cols, len(ci)))
        np.savetxt(f, np.column_stack([r + 1, ci + 1, v]), fmt="%d %d %.17g")


@pytest.mark.parametrize("width", [64, 128])
def test_header_layer_under_the_switch(env, tmp_path, width):
    S, O, torch, cuda = env
    from sblas_amd import synth
    # the long row's columns spread over 250 000: its panel is the direct kernels', so the split plan does split it
    rows, cols = 3000, 250000
    rp, ci, v = synth.random_csr(rows, cols, 25, long_row=(1234, 40000))
    R, Cx = upload(torch, cuda, rp, ci)
    plan = S.SpmmPlan(rows, cols, R, Cx, width, split=True)
    assert plan.split_info()["split_rows"] == 1, (plan.info(), plan.split_info())
    plan.destroy()
    path = str(tmp_path / "long_row.mtx")
    write_mtx(path, rows, cols, rp, ci, v)
    for switch in ("1", "0"):
        p = subprocess.run([os.path.join(BIN, "plan_test"), path, str(width), "1", "3"], capture_output=True, text=True,
                           timeout=600, env=dict(os.environ, SBLAS_SPMM_SPLIT=switch))
        out = p.stdout + p.stderr
        assert p.returncode == 0 and "plan_test: PASS" in out and "MISMATCH" not in out, out[-1500:]
        # calls 1 and 2 of both methods run planned; the driver reports the rows their plans split
        planned = re.findall(r"method \d call \d: ok, 1 of 1 GPUs planned, (\d+) split rows", out)
        assert len(planned) == 4, out[-1500:]
        assert all(int(k) == (1 if switch == "1" else 0) for k in planned), out[-1500:]
