"""Masked SpGEMM on the GPU (MaskedSpgemmPlan, masked_spgemm) against the library's scalar reference mspgemm_ref, which
tests/test_mspgemm_host.py pins to the numpy restatement of the contract.  Every case runs as create makes it and with
general=True; both must give the reference's values bit for bit (spgemm_numerics.same_bits: equal bits; where the
reference holds a NaN, a NaN), hence each other's.  Then the identity with SpgemmPlan on the device, the path rule,
contract (I), the plan's behaviour under new values and graph replay, and the refusals.  Every size at which a kernel
takes another branch is read from mspgemm_limits()."""
import ctypes as C

import numpy as np
import pytest

import mspgemm_numerics as MN
import spgemm_numerics as GN

pytestmark = pytest.mark.gpu

INVALID = 1
HOST_CASES = MN.host_cases()
_gpu_cases = {}
_ref = {}


@pytest.fixture(scope="module")
def env(sblas, cuda):
    import torch
    return sblas, torch, cuda


def gpu_cases(S):
    if not _gpu_cases:
        _gpu_cases.update(MN.gpu_cases(S.mspgemm_limits()))
    return _gpu_cases


def up(torch, cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def reference(S, name, case):
    if name not in _ref:
        m, n, k, M, X, Y = case
        _ref[name] = S.mspgemm_ref(m, n, k, M[0], M[1], X[0], X[1], X[2], Y[0], Y[1], Y[2])
    return _ref[name]


def run_case(env, name, case, ref=None):
    """both plans against the reference -> {route: values} as numpy"""
    S, torch, cuda = env
    m, n, k, M, X, Y = case
    ref = reference(S, name, case) if ref is None else ref
    dM, dX, dY = up(torch, cuda, *M), up(torch, cuda, *X), up(torch, cuda, *Y)
    xa, ya = MN.ascending(X[0], X[1]), MN.ascending(Y[0], Y[1])
    out = {}
    for route, kw in (("auto", dict()), ("general", dict(general=True))):
        plan = S.MaskedSpgemmPlan(m, n, k, dM[0], dM[1], dX[0], dX[1], dY[0], dY[1], **kw)
        info = plan.info()
        val = plan.multiply(dX[2], dY[2])
        torch.cuda.synchronize()
        got = val.cpu().numpy().copy()
        plan.destroy()
        assert info["path"] == ("sorted" if route == "auto" and xa and ya else "general"), (name, route)
        assert info["x_ascending"] == xa and info["y_ascending"] == ya and info["general"] == (route == "general"), (name, route)
        assert (info["m"], info["n"], info["k"], info["nnz_m"], info["nnz_x"], info["nnz_y"]) == (m, n, k, len(M[1]), len(X[1]), len(Y[1]))
        assert info["launches"] == (1 if len(M[1]) else 0), (name, route)
        if not GN.same_bits(got, ref):
            bad = np.flatnonzero(GN.bits(got) != GN.bits(ref))
            pytest.fail("%s / %s: %d of %d values differ from the reference, first at %d: %r vs %r"
                        % (name, route, len(bad), len(ref), bad[0], got[bad[0]], ref[bad[0]]))
        out[route] = got
    return out


# ---------------------------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HOST_CASES))
def test_the_host_cases(env, name):
    run_case(env, name, HOST_CASES[name])


GPU_CASE_NAMES = ["x_row_lengths", "long_mask_row", "long_y_row", "long_x_row", "straddle", "exact_workgroup", "rect_big",
                  "x_row_lengths_unsorted", "straddle_unsorted", "rect_big_unsorted"]


@pytest.mark.parametrize("name", GPU_CASE_NAMES)
def test_the_shapes_at_which_a_kernel_takes_another_branch(env, name):
    cases = gpu_cases(env[0])
    assert sorted(cases) == sorted(GPU_CASE_NAMES)
    run_case(env, name, cases[name])


def test_the_x_rows_stand_at_the_limits(env):
    lim = env[0].mspgemm_limits()
    m, n, k, M, X, Y = gpu_cases(env[0])["x_row_lengths"]
    lens = set(np.diff(X[0]).tolist())
    assert {0, 1, 63, 64, 65, lim["lds_row"] - 1, lim["lds_row"], lim["lds_row"] + 1} <= lens
    assert np.diff(M[0]).max() > 64 and len(gpu_cases(env[0])["long_mask_row"][3][1]) > 2 * lim["threads"]


def test_special_values_on_both_paths(env):
    for k, name in enumerate(("rect", "unsorted", "dup_x", "dup_y", "dup_mask")):
        m, n, kk, M, X, Y = HOST_CASES[name]
        Xs, Ys = MN.special_values(X, Y, 3540 + k)
        run_case(env, name + "_special", (m, n, kk, M, Xs, Ys))


def test_an_inf_at_an_unmatched_column_never_reaches_the_output(env):
    inf = np.inf
    M = MN.pattern_of_rows([[0, 1, 2, 3]])
    X = MN.csr_of_rows([([0, 2, 5], [inf, 2.0, 0.0])])
    Y = MN.csr_of_rows([([1, 2], [inf, 3.0]), ([3, 5], [np.nan, inf]), ([0], [0.0]), ([0, 2], [-1.0, 1e308])])
    got = run_case(env, "classes", (1, 4, 6, M, X, Y))
    for out in got.values():
        assert out[0] == 6.0 and np.isnan(out[1]) and np.isnan(out[2]) and np.isnan(out[3])


def test_zeros_keep_their_sign_and_no_pair_is_plus_zero(env):
    for out in run_case(env, "no_pair", HOST_CASES["no_pair"]).values():
        assert out[2] == 0.0 and not np.signbit(out[2]) and out[1] == -1.0
    for out in run_case(env, "minus_zero", HOST_CASES["minus_zero"]).values():
        assert out[0] == 0.0 and np.signbit(out[0]) and out[1] == 0.0 and np.signbit(out[1])
    for out in run_case(env, "dup_order", HOST_CASES["dup_order"]).values():
        assert out[0] == 0.0 and out[1] == 0.0                                # (1e16 + 1) + -1e16, twice


@pytest.mark.parametrize("q", range(len(MN.FMA_CASES)))
def test_no_product_is_fused_into_the_add(env, q):
    """mspgemm_numerics.FMA_CASES: either contraction would change the last bit.  On one entry and on a thousand: the
    same pair under a mask that fills several workgroups."""
    x1, y1, x2, y2 = MN.FMA_CASES[q]
    want = x1 * y1 + x2 * y2
    for out in run_case(env, "fma%d" % q, MN.fma_case(q)).values():
        assert GN.bits(out)[0] == GN.bits(np.array([want]))[0]
    m, n, k, M, X, Y = MN.fma_case(q)
    many = (np.array([0, 1000], np.int32), np.zeros(1000, np.int32))
    for out in run_case(env, "fma%d_many" % q, (m, n, k, many, X, Y)).values():
        assert (GN.bits(out) == GN.bits(np.array([want]))[0]).all()


def test_ash85_on_the_pattern_of_a_times_its_transpose(env, ash85):
    A = (ash85["rowptr"].astype(np.int32), ash85["colidx"].astype(np.int32), ash85["val"].astype(np.float64))
    m, k = ash85["m"], ash85["n"]
    At = GN.transpose_csr(m, k, *A)
    rpc, cic, vc = GN.reference(m, m, A[0], A[1], A[2], At[0], At[1], At[2])
    got = run_case(env, "ash85", (m, m, k, (rpc, cic), A, A))
    assert len(cic) > len(A[1])
    if MN.ascending(A[0], A[1]):                                              # then (A^T)^T in the stable order is A itself
        assert GN.same_bits(got["auto"], vc)


# ---------------------------------------------------------------------------------------------------------------------
# the identity with SpGEMM, on the device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sorted", "unsorted_dups"])
def test_on_the_product_s_pattern_the_plan_gives_spgemm_s_bits(env, kind):
    S, torch, cuda = env
    rng = np.random.default_rng(3550)
    m, k, n = 150, 120, 170
    if kind == "sorted":
        A, B = GN.random_csr(rng, m, k, 5, empty_every=7), GN.random_csr(rng, k, n, 5, empty_every=5)
    else:
        A = MN.add_dups(rng, GN.random_csr(rng, m, k, 5, sort=False, empty_every=7))
        B = MN.add_dups(rng, GN.random_csr(rng, k, n, 5, sort=False, empty_every=5))
    dA, dB = up(torch, cuda, *A), up(torch, cuda, *B)
    tp = S.TransposePlan(k, n, dB[0], dB[1], dB[2])
    colptr, rowidx, val_t = tp.csc()
    products = []
    for spgemm_general in (False, True):
        c = S.SpgemmPlan(m, k, n, dA[0], dA[1], dB[0], dB[1], general=spgemm_general)
        rpc, cic = c.csr()
        val_c = c.multiply(dA[2], dB[2])
        for general in (False, True):
            plan = S.MaskedSpgemmPlan(m, n, k, rpc, cic, dA[0], dA[1], colptr, rowidx, general=general)
            assert plan.info()["path"] == ("sorted" if kind == "sorted" and not general else "general")
            out = plan.multiply(dA[2], val_t)
            torch.cuda.synchronize()
            assert c.nnz_c > 1000 and GN.same_bits(out.cpu().numpy(), val_c.cpu().numpy()), (kind, spgemm_general, general)
            plan.destroy()
        products.append(val_c.cpu().numpy())
        c.destroy()
    assert GN.same_bits(products[0], products[1])
    tp.destroy()


def test_one_duplicate_or_one_descent_sends_the_plan_to_the_general_path(env):
    S, torch, cuda = env
    m, n, k, M, X, Y = HOST_CASES["rect"]
    dM = up(torch, cuda, *M)

    def path(X, Y):
        dX, dY = up(torch, cuda, X[0], X[1]), up(torch, cuda, Y[0], Y[1])
        plan = S.MaskedSpgemmPlan(m, n, k, dM[0], dM[1], dX[0], dX[1], dY[0], dY[1])
        info = plan.info()
        plan.destroy()
        return info["path"], info["x_ascending"], info["y_ascending"]

    def with_dup(A):                                                          # the last row with two entries: its second = its first
        rp, ci, v = A[0], A[1].copy(), A[2]
        i = max(r for r in range(len(rp) - 1) if rp[r + 1] - rp[r] >= 2)
        ci[rp[i] + 1] = ci[rp[i]]
        return rp, ci, v

    def with_swap(A):                                                         # the first row with two entries, its first two swapped
        rp, ci, v = A[0], A[1].copy(), A[2]
        i = min(r for r in range(len(rp) - 1) if rp[r + 1] - rp[r] >= 2)
        ci[rp[i]], ci[rp[i] + 1] = ci[rp[i] + 1], ci[rp[i]]
        return rp, ci, v

    assert path(X, Y) == ("sorted", True, True)
    assert path(with_dup(X), Y) == ("general", False, True) and path(X, with_dup(Y)) == ("general", True, False)
    assert path(with_swap(X), Y) == ("general", False, True) and path(X, with_swap(Y)) == ("general", True, False)
    # the mask's order is nobody's business
    dX, dY = up(torch, cuda, X[0], X[1]), up(torch, cuda, Y[0], Y[1])
    Mu = with_swap((M[0], M[1], None))
    dMu = up(torch, cuda, Mu[0], Mu[1])
    plan = S.MaskedSpgemmPlan(m, n, k, dMu[0], dMu[1], dX[0], dX[1], dY[0], dY[1])
    assert plan.info()["path"] == "sorted"
    plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# (I): an entry's bits are its two rows' alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["straddle", "x_row_lengths", "rect_big_unsorted"])
def test_an_entry_s_bits_do_not_depend_on_where_it_stands(env, name):
    S, torch, cuda = env
    m, n, k, M, X, Y = gpu_cases(S)[name]
    ref = reference(S, name, gpu_cases(S)[name])
    rng = np.random.default_rng(3560)
    # the mask's entries permuted inside their rows: out is permuted, no bit changes
    perm = np.concatenate([M[0][i] + rng.permutation(M[0][i + 1] - M[0][i]) for i in range(m)]).astype(np.int64)
    run_case(env, name + "_permuted", (m, n, k, (M[0], M[1][perm]), X, Y), ref=ref[perm])
    # 37 entries put in front (a new first row, a copy of X's last row under it): every entry moves to another lane,
    # wave and workgroup
    front = rng.integers(0, n, 37).astype(np.int32)
    M2 = (np.concatenate(([0], M[0] + 37)).astype(np.int32), np.concatenate((front, M[1])))
    last = slice(X[0][m - 1], X[0][m])
    X2 = (np.concatenate(([0], X[0] + (X[0][m] - X[0][m - 1]))).astype(np.int32), np.concatenate((X[1][last], X[1])),
          np.concatenate((X[2][last], X[2])))
    got = run_case(env, name + "_shifted", (m + 1, n, k, M2, X2, Y))
    for out in got.values():
        assert GN.same_bits(out[37:], ref)


def test_value_arrays_one_element_off_16_byte_alignment(env):
    S, torch, cuda = env
    m, n, k, M, X, Y = gpu_cases(S)["straddle"]
    ref = reference(S, "straddle", gpu_cases(S)["straddle"])
    dM, dX, dY = up(torch, cuda, *M), up(torch, cuda, *X), up(torch, cuda, *Y)
    pad = lambda t: torch.cat((torch.zeros(1, dtype=torch.float64, device=cuda), t))[1:]
    for general in (False, True):
        plan = S.MaskedSpgemmPlan(m, n, k, dM[0], dM[1], dX[0], dX[1], dY[0], dY[1], general=general)
        ox, oy, oo = pad(dX[2]), pad(dY[2]), torch.empty(len(M[1]) + 1, dtype=torch.float64, device=cuda)[1:]
        assert ox.data_ptr() % 16 == 8 and oy.data_ptr() % 16 == 8 and oo.data_ptr() % 16 == 8
        plan.multiply(ox, oy, out=oo)
        torch.cuda.synchronize()
        assert GN.same_bits(oo.cpu().numpy(), ref)
        plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["straddle", "straddle_unsorted"])
def test_multiply_again_with_new_values_and_replayed_from_a_graph(env, name):
    S, torch, cuda = env
    m, n, k, M, X, Y = gpu_cases(S)[name]
    rng = np.random.default_rng(3570)
    dM, dX, dY = up(torch, cuda, *M), up(torch, cuda, *X), up(torch, cuda, *Y)
    plan = S.MaskedSpgemmPlan(m, n, k, dM[0], dM[1], dX[0], dX[1], dY[0], dY[1])
    assert plan.info()["path"] == ("general" if name.endswith("unsorted") else "sorted")
    held = plan.info()["bytes"]
    ref = lambda vx, vy: S.mspgemm_ref(m, n, k, M[0], M[1], X[0], X[1], vx, Y[0], Y[1], vy)
    first = plan.multiply(dX[2], dY[2])
    vx2, vy2 = rng.random(len(X[1])) - 0.5, rng.random(len(Y[1])) - 0.5
    second = plan.multiply(*up(torch, cuda, vx2, vy2))
    out = torch.full((len(M[1]) + 3,), -7.0, dtype=torch.float64, device=cuda)
    given = plan.multiply(dX[2], dY[2], out=out)
    torch.cuda.synchronize()
    assert given.data_ptr() == out.data_ptr() and (out[len(M[1]):] == -7.0).all()
    assert GN.same_bits(first.cpu().numpy(), ref(X[2], Y[2])) and GN.same_bits(second.cpu().numpy(), ref(vx2, vy2))
    assert torch.equal(out[:len(M[1])].view(torch.int64), first.view(torch.int64))
    # captured once, replayed after the value tensors are overwritten in place
    bufx, bufy = dX[2].clone(), dY[2].clone()
    gout = torch.empty(len(M[1]), dtype=torch.float64, device=cuda)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            plan.multiply(bufx, bufy, out=gout)
    for _ in range(2):
        nx, ny = rng.random(len(X[1])) * 2 - 1, rng.random(len(Y[1])) * 2 - 1
        bufx.copy_(torch.from_numpy(nx)), bufy.copy_(torch.from_numpy(ny))
        gout.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        eager = plan.multiply(bufx, bufy)
        torch.cuda.synchronize()
        assert GN.same_bits(gout.cpu().numpy(), ref(nx, ny)) and torch.equal(gout.view(torch.int64), eager.view(torch.int64))
    assert plan.info()["bytes"] == held                                       # multiply allocates nothing in the library
    # the one-shot call
    one = S.masked_spgemm((m, n, dM[0], dM[1]), (m, k) + tuple(dX), (n, k) + tuple(dY))
    assert torch.equal(one.view(torch.int64), first.view(torch.int64))
    plan.destroy()


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(env):
    S, torch, cuda = env
    L = S.lib()
    m, n, k, M, X, Y = HOST_CASES["rect"]

    def create(M, X, Y, m=m, n=n, k=k, null=(), flags=0, out=True):
        d = up(torch, cuda, M[0], M[1], X[0], X[1], Y[0], Y[1])
        ptrs = [None if j in null else t.data_ptr() for j, t in enumerate(d)]
        h = C.c_void_p()
        rc = L.sblas_hip_mspgemm_plan_create(-1, None, m, n, k, *ptrs, flags, C.byref(h) if out else None)
        torch.cuda.synchronize()
        assert rc == 0 or not h.value                                         # no plan is made
        if rc == 0:
            L.sblas_hip_mspgemm_plan_destroy(h)
        return rc

    assert create(M, X, Y) == 0 and create(M, X, Y, flags=1) == 0
    for which, cols in ((0, n), (1, k), (2, k)):
        for mutate in ("late", "down", "col_high", "col_negative"):
            ops = [[a.copy() for a in op] for op in (M, X, Y)]
            if mutate == "late":
                ops[which][0][0] = 1                                          # rowptr does not start at 0
            elif mutate == "down":
                ops[which][0][1] = ops[which][0][2] + 1                       # rowptr steps down
            elif mutate == "col_high":
                ops[which][1][3] = cols                                       # a mask column = n, an X or Y column = k
            else:
                ops[which][1][5] = -1
            for flags in (0, 1):
                assert create(*ops, flags=flags) == INVALID, (which, mutate)
    for null in range(6):
        assert create(M, X, Y, null=(null,)) == INVALID, null
    assert create(M, X, Y, out=False) == INVALID
    assert create(M, X, Y, m=-1) == INVALID and create(M, X, Y, k=1 << 31) == INVALID and create(M, X, Y, flags=2) == INVALID
    # numeric: the argument path
    dM, dX, dY = up(torch, cuda, *M), up(torch, cuda, *X), up(torch, cuda, *Y)
    plan = S.MaskedSpgemmPlan(m, n, k, dM[0], dM[1], dX[0], dX[1], dY[0], dY[1])
    out = torch.empty(len(M[1]), dtype=torch.float64, device=cuda)
    num = L.sblas_hip_mspgemm_plan_numeric
    assert num(None, None, dX[2].data_ptr(), dY[2].data_ptr(), out.data_ptr()) == INVALID
    assert num(plan.handle, None, None, dY[2].data_ptr(), out.data_ptr()) == INVALID
    assert num(plan.handle, None, dX[2].data_ptr(), None, out.data_ptr()) == INVALID
    assert num(plan.handle, None, dX[2].data_ptr(), dY[2].data_ptr(), None) == INVALID
    assert num(plan.handle, None, dX[2].data_ptr(), dY[2].data_ptr(), out.data_ptr()) == 0
    assert L.sblas_hip_mspgemm_plan_info(None, (C.c_int64 * 12)()) == INVALID
    with pytest.raises(S.SblasError, match="out has"):
        plan.multiply(dX[2], dY[2], out=out[:-1])
    with pytest.raises(S.SblasError, match="entries"):
        plan.multiply(dX[2][:-1], dY[2])                                      # short value arrays
    with pytest.raises(S.SblasError, match="entries"):
        plan.multiply(dX[2], dY[2][:-1])
    with pytest.raises(S.SblasError, match="float64"):
        plan.multiply(dX[2].float(), dY[2])
    with pytest.raises(S.SblasError, match="GPU tensor"):
        plan.multiply(dX[2].cpu(), dY[2])
    with pytest.raises(S.SblasError, match="row pointers end"):
        S.MaskedSpgemmPlan(m, n, k, dM[0], dM[1], dX[0], dX[1][:-1], dY[0], dY[1])
    with pytest.raises(S.SblasError, match="row pointers end"):
        S.MaskedSpgemmPlan(m, n, k, dM[0], dM[1][:-1], dX[0], dX[1], dY[0], dY[1])
    with pytest.raises(S.SblasError, match="GPU tensor"):
        S.MaskedSpgemmPlan(m, n, k, dM[0], dM[1], dX[0].cpu(), dX[1], dY[0], dY[1])
    plan.destroy()
    torch.cuda.synchronize()


def test_a_plan_used_on_another_current_device_is_refused(env):
    S, torch, cuda = env
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    m, n, k, M, X, Y = HOST_CASES["rect"]
    dM, dX, dY = up(torch, cuda, *M), up(torch, cuda, *X), up(torch, cuda, *Y)
    plan = S.MaskedSpgemmPlan(m, n, k, dM[0], dM[1], dX[0], dX[1], dY[0], dY[1])
    out = torch.empty(len(M[1]), dtype=torch.float64, device=cuda)
    with torch.cuda.device(1):
        assert S.lib().sblas_hip_mspgemm_plan_numeric(plan.handle, None, dX[2].data_ptr(), dY[2].data_ptr(), out.data_ptr()) == INVALID
    with pytest.raises(S.SblasError, match="rowptr_m on"):
        S.MaskedSpgemmPlan(m, n, k, dM[0], dM[1], dX[0].to("cuda:1"), dX[1], dY[0], dY[1])
    with pytest.raises(S.SblasError, match="the plan on"):
        plan.multiply(dX[2].to("cuda:1"), dY[2])
    plan.destroy()
