"""Autograd for SpGEMM (sblas_amd.autograd.SpgemmOperator) on the GPU: the forward is SpgemmPlan.multiply's, both
gradients are the masked SpGEMM's -- held to mspgemm_ref bit for bit on the operands the module docstring names, and to
float64 dense torch within a bound derived from the sums' lengths --, torch's gradcheck, which halves are formed, plan
reuse, and a graph that runs through csr_add and CsrOperator.matvec."""
import numpy as np
import pytest

import mspgemm_numerics as MN
import spgemm_numerics as GN

pytestmark = pytest.mark.gpu

_cases = {}


@pytest.fixture(scope="module")
def env(sblas, cuda):
    import torch
    import sblas_amd.autograd as AG
    return sblas, torch, cuda, AG


def up(torch, cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def starve_a_row(A, B):
    """B with the rows emptied that A's first non-empty row names: that row of A then names only empty rows of B"""
    rp, ci, v = B
    i = min(r for r in range(len(A[0]) - 1) if A[0][r + 1] > A[0][r])
    named = set(A[1][A[0][i]:A[0][i + 1]].tolist())
    rows = [([], []) if r in named else (ci[rp[r]:rp[r + 1]], v[rp[r]:rp[r + 1]]) for r in range(len(rp) - 1)]
    return MN.csr_of_rows(rows)


def cases(ash85):
    """name -> (m, k, n, A, B)"""
    if _cases:
        return _cases
    rng = np.random.default_rng(3600)
    m, k, n = 60, 45, 80
    A, B = GN.random_csr(rng, m, k, 4, empty_every=7), GN.random_csr(rng, k, n, 4, empty_every=6)
    Au, Bu = GN.random_csr(rng, m, k, 4, sort=False, empty_every=7), GN.random_csr(rng, k, n, 4, sort=False, empty_every=6)
    _cases["sorted"] = (m, k, n, A, B)
    _cases["dup_a"] = (m, k, n, MN.add_dups(rng, Au), B)
    _cases["dup_b"] = (m, k, n, A, MN.add_dups(rng, Bu))
    _cases["starved_row"] = (m, k, n, A, starve_a_row(A, B))
    H = (ash85["rowptr"].astype(np.int32), ash85["colidx"].astype(np.int32), rng.random(ash85["nnz"]) * 2 - 1)
    hm, hk = ash85["m"], ash85["n"]
    Ht = GN.transpose_csr(hm, hk, *H)
    Ht = (Ht[0], Ht[1], rng.random(len(Ht[1])) * 2 - 1)
    _cases["ash85_sorted"] = (hm, hk, hm, H, Ht)
    _cases["ash85_dup_a"] = (hm, hk, hm, MN.add_dups(rng, MN.shuffle_rows(rng, H)), Ht)
    _cases["ash85_dup_b"] = (hm, hk, hm, H, MN.add_dups(rng, MN.shuffle_rows(rng, Ht)))
    _cases["ash85_starved_row"] = (hm, hk, hm, H, starve_a_row(H, Ht))
    return _cases


NAMES = ["sorted", "dup_a", "dup_b", "starved_row", "ash85_sorted", "ash85_dup_a", "ash85_dup_b", "ash85_starved_row"]


def gamma(K):
    u = 2.0 ** -53
    return K * u / (1 - K * u)


def stored(rowptr, colidx):
    return MN.rows_of(rowptr).astype(np.int64), np.asarray(colidx, np.int64)


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_forward_and_both_gradients(env, ash85, name, general):
    S, torch, cuda, AG = env
    m, k, n, A, B = cases(ash85)[name]
    dA, dB = up(torch, cuda, *A), up(torch, cuda, *B)
    op = AG.SpgemmOperator(m, k, n, dA[0], dA[1], dB[0], dB[1], general=general)
    plan = S.SpgemmPlan(m, k, n, dA[0], dA[1], dB[0], dB[1], general=general)
    rpc_t, cic_t = op.csr()
    assert torch.equal(rpc_t, plan.csr()[0]) and torch.equal(cic_t, plan.csr()[1])
    va, vb = dA[2].clone().requires_grad_(True), dB[2].clone().requires_grad_(True)
    vc = op.multiply(va, vb)
    assert vc.requires_grad and bool((vc.detach() == plan.multiply(dA[2], dB[2])).all())
    rng = np.random.default_rng(3601)
    dC = rng.random(op.nnz_c) * 2 - 1
    vc.backward(torch.from_numpy(dC).to(cuda))
    torch.cuda.synchronize()
    ga, gb = va.grad.cpu().numpy(), vb.grad.cpu().numpy()
    rpc, cic = rpc_t.cpu().numpy(), cic_t.cpu().numpy()
    if name.endswith("starved_row"):
        i = min(r for r in range(m) if A[0][r + 1] > A[0][r])
        assert rpc[i + 1] == rpc[i] and (ga[A[0][i]:A[0][i + 1]] == 0.0).all()  # an empty row of C: no pair, +0.0
    # the masked products of the module docstring, bit for bit
    want_a = S.mspgemm_ref(m, k, n, A[0], A[1], rpc, cic, dC, B[0], B[1], B[2])
    At, Ct = GN.transpose_csr(m, k, *A), GN.transpose_csr(m, n, rpc, cic, dC)
    want_b = S.mspgemm_ref(k, n, m, B[0], B[1], At[0], At[1], At[2], Ct[0], Ct[1], Ct[2])
    assert GN.same_bits(ga, want_a) and GN.same_bits(gb, want_b), name
    # float64 dense torch, within 2 gamma_K (|dC| |B|^T) and 2 gamma_K (|A|^T |dC|): one gamma_K for the pinned left-to-right
    # sum, one for the dense product's, K the inner dimension.  A stored duplicate is one more term on our side and one
    # more rounding (the densified sum) on the other; both stay inside gamma_K while a row's stored entries + 1 <= K.
    assert max(np.diff(B[0]).max(), np.diff(Ct[0]).max()) + 1 <= n and max(np.diff(At[0]).max(), np.diff(rpc).max()) + 1 <= m
    dense = lambda r, c, M: torch.from_numpy(GN.to_dense(r, c, *M)).to(cuda)
    absd = lambda r, c, M: torch.from_numpy(GN.to_dense(r, c, M[0], M[1], np.abs(M[2]))).to(cuda)
    C_ = (rpc, cic, dC)
    Ad, Bd, Cd = dense(m, k, A), dense(k, n, B), dense(m, n, C_)
    ia, ja = stored(A[0], A[1])
    ib, jb = stored(B[0], B[1])
    da_dense, da_bound = (Cd @ Bd.T).cpu().numpy()[ia, ja], 2 * gamma(n) * (absd(m, n, C_) @ absd(k, n, B).T).cpu().numpy()[ia, ja]
    db_dense, db_bound = (Ad.T @ Cd).cpu().numpy()[ib, jb], 2 * gamma(m) * (absd(m, k, A).T @ absd(m, n, C_)).cpu().numpy()[ib, jb]
    assert (np.abs(ga - da_dense) <= da_bound).all(), (name, np.abs(ga - da_dense).max())
    assert (np.abs(gb - db_dense) <= db_bound).all(), (name, np.abs(gb - db_dense).max())
    op.destroy(), plan.destroy()


def test_a_duplicated_entry_receives_the_gradient_of_its_position(env, ash85):
    S, torch, cuda, AG = env
    m, k, n, A, B = cases(ash85)["dup_a"]
    dA, dB = up(torch, cuda, *A), up(torch, cuda, *B)
    op = AG.SpgemmOperator(m, k, n, dA[0], dA[1], dB[0], dB[1])
    va = dA[2].clone().requires_grad_(True)
    op.multiply(va, dB[2]).sum().backward()
    g = va.grad.cpu().numpy()
    pairs = 0
    for i in range(m):
        row = A[1][A[0][i]:A[0][i + 1]]
        if len(row) >= 2 and row[-1] == row[0]:                               # add_dups: the last entry repeats the first
            assert GN.bits(g)[A[0][i]] == GN.bits(g)[A[0][i + 1] - 1]
            pairs += 1
    assert pairs > 5
    op.destroy()


@pytest.mark.parametrize("dup", [False, True])
def test_gradcheck(env, dup):
    S, torch, cuda, AG = env
    rng = np.random.default_rng(3610)
    m, k, n = 7, 6, 8
    A, B = GN.random_csr(rng, m, k, 2, sort=not dup), GN.random_csr(rng, k, n, 2, sort=not dup)
    if dup:
        A, B = MN.add_dups(rng, A, every=2), MN.add_dups(rng, B, every=2)
    dA, dB = up(torch, cuda, *A), up(torch, cuda, *B)
    op = AG.SpgemmOperator(m, k, n, dA[0], dA[1], dB[0], dB[1])
    assert op.nnz_c > 10
    va, vb = dA[2].clone().requires_grad_(True), dB[2].clone().requires_grad_(True)
    assert torch.autograd.gradcheck(op.multiply, (va, vb))                    # torch's defaults; the function is bilinear
    op.destroy()


def test_only_the_requested_half_is_formed_and_the_plans_are_reused(env, ash85):
    S, torch, cuda, AG = env
    m, k, n, A, B = cases(ash85)["dup_b"]
    dA, dB = up(torch, cuda, *A), up(torch, cuda, *B)
    rng = np.random.default_rng(3620)
    op = AG.SpgemmOperator(m, k, n, dA[0], dA[1], dB[0], dB[1])
    assert op.grad_a_plan is None and op.grad_b_plan is None
    va = dA[2].clone().requires_grad_(True)
    op.multiply(va, dB[2]).sum().backward()                                   # val_b asks for nothing
    assert op.grad_a_plan is not None and op.grad_b_plan is None and op.transpose_a is None and op.transpose_c is None
    op2 = AG.SpgemmOperator(m, k, n, dA[0], dA[1], dB[0], dB[1])
    vb = dB[2].clone().requires_grad_(True)
    op2.multiply(dA[2], vb).sum().backward()                                  # val_a asks for nothing
    assert op2.grad_a_plan is None and op2.grad_b_plan is not None and op2.transpose_a is not None and op2.transpose_c is not None
    op2.destroy()
    # two more backward passes with new values: the same plans, fresh bits
    rpc, cic = (t.cpu().numpy() for t in op.csr())
    kept = None
    for _ in range(2):
        a, b, dC = rng.random(len(A[1])) - 0.5, rng.random(len(B[1])) - 0.5, rng.random(op.nnz_c) - 0.5
        ta, tb = (t.requires_grad_(True) for t in up(torch, cuda, a, b))
        op.multiply(ta, tb).backward(torch.from_numpy(dC).to(cuda))
        handles = tuple(p.handle.value for p in (op.grad_a_plan, op.grad_b_plan, op.transpose_a, op.transpose_c))
        assert kept is None or handles == kept
        kept = handles
        At, Ct = GN.transpose_csr(m, k, A[0], A[1], a), GN.transpose_csr(m, n, rpc, cic, dC)
        assert GN.same_bits(ta.grad.cpu().numpy(), S.mspgemm_ref(m, k, n, A[0], A[1], rpc, cic, dC, B[0], B[1], b))
        assert GN.same_bits(tb.grad.cpu().numpy(), S.mspgemm_ref(k, n, m, B[0], B[1], At[0], At[1], At[2], Ct[0], Ct[1], Ct[2]))
    op.destroy()


def test_the_product_feeds_csr_add_and_matvec_in_one_graph(env, ash85):
    S, torch, cuda, AG = env
    m, k, n, A, B = cases(ash85)["sorted"]
    dA, dB = up(torch, cuda, *A), up(torch, cuda, *B)
    op = AG.SpgemmOperator(m, k, n, dA[0], dA[1], dB[0], dB[1])
    rpc, cic = op.csr()
    geam = S.GeamPlan(m, n, rpc, cic, rpc, cic)                               # 1.0 * C + 0.5 * C, on C's pattern
    srp, sci = geam.csr()
    cop = AG.CsrOperator(m, n, srp, sci)
    va = dA[2].clone().requires_grad_(True)
    x = torch.from_numpy(np.random.default_rng(3630).random(n) + 0.5).to(cuda)
    vc = op.multiply(va, dB[2])
    y = cop.matvec(AG.csr_add(geam, vc, vc, 1.0, 0.5), x)
    y.sum().backward()
    torch.cuda.synchronize()
    # d/dA[i, k] of sum(1.5 (A B) x) = 1.5 (B x)[k]: n products and three more roundings (the sum's two scalings and its add)
    bx = GN.to_dense(k, n, *B) @ x.cpu().numpy()
    babs = np.abs(GN.to_dense(k, n, *B)) @ x.cpu().numpy()
    got, cols = va.grad.cpu().numpy(), np.asarray(A[1], np.int64)
    assert (np.abs(got - 1.5 * bx[cols]) <= 2 * gamma(n + 3) * 1.5 * babs[cols]).all()
    assert np.abs(got).max() > 0
    op.destroy(), geam.destroy(), cop.destroy()
