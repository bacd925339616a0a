"""Masked SpGEMM (MaskedSpgemmPlan: sblas_hip_mspgemm_plan_*) on one GPU: the gradient dA = A's pattern o (dC A^T) of
C = A * A, and SpgemmOperator's forward + backward.

Per input: create on the host clock (the call synchronises), numeric per call (median over `--rounds` rounds of calls
between two device events after a warm-up, every round reported), and the bytes the plan holds, for routes that
alternate inside every round so that all see the same machine:
  sorted     the plan as create makes it for ascending operands;
  general    the same plan with general=True, the quadratic path (half the rounds, a call or two each: the slow path);
  spgemm     what a user could do before (the yardstick): SpgemmPlan.multiply of the full product dC * A^T alone, A^T from
             a TransposePlan.  A lower bound on the old route, which still needs a gather onto A's pattern.  Its product
             count is computed first; above --max-products the full product is not formed and the record says
             "not measured" with the count;
  forward    SpgemmOperator.multiply without gradients;
  fwd_bwd    the same with both value arrays requiring gradients, and backward(dC): two masked SpGEMMs, two transposes'
             values refreshed.
sorted and general must give the same bits; the record says so.

Every input is measured in a child process of its own under its own time limit, one at a time, and nothing is started
after a child that failed or ran out of time.  One JSON object per input on stdout; --out writes the list.

  python tools/mspgemm_bench.py [--inputs banded5,nd24k,powerlaw] [--rounds 5] [--out profiles/r29_mspgemm.json]

Inputs, tools/spgemm_bench.py's: banded5 = 10^6 banded rows of 5 (band +-500); nd24k = nd24k_like(0.05), 3600 rows;
powerlaw = the power-law matrix (10^6 rows of 3 on average, rows of up to 5000), rows made ascending."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "s-blas_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def measure(name, args):
    import torch
    import sblas_amd as S
    import sblas_amd.autograd as AG
    from sblas_amd import synth
    from spgemm_bench import ascending, timed_pair
    if not torch.cuda.is_available():
        raise SystemExit("mspgemm_bench needs a GPU")
    dev = torch.device("cuda:0")
    if name == "banded5":
        n = args.rows
        rp, ci, v = synth.banded(n, 5, 500)
        label = "banded5, %d rows" % n
        rpa, cia, va = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (rp.astype(np.int32), ci.astype(np.int32), v))
    elif name == "nd24k":
        n, (rp, ci, v) = synth.nd24k_like(args.nd24k_scale)
        label = "nd24k_like(%g), %d rows" % (args.nd24k_scale, n)
        rpa, cia, va = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (rp.astype(np.int32), ci.astype(np.int32), v))
    else:
        assert name == "powerlaw", name
        n = args.rows
        rp, ci, v = synth.powerlaw(n, avg=3.0, max_len=5000)
        label = "powerlaw(%d)" % n
        rpa, cia, va = ascending(S, torch, dev, n, n, rp, ci, v)
    rec = dict(input=label + ": dA of A * A", n=n, nnz_a=int(cia.numel()), limits=S.mspgemm_limits(), device=torch.cuda.get_device_name(0))

    def clocked(make):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p = make()
        torch.cuda.synchronize()
        return p, (time.perf_counter() - t0) * 1e3

    c, rec["create_spgemm_forward_ms"] = clocked(lambda: S.SpgemmPlan(n, n, n, rpa, cia, rpa, cia))
    rpc, cic = c.csr()
    nnz_c = c.nnz_c
    rec["nnz_c"], rec["forward_products"] = nnz_c, c.info()["products"]
    dC = torch.from_numpy(np.random.default_rng(29).random(nnz_c) * 2 - 1).to(dev)
    plans = {}
    plans["sorted"], rec["create_sorted_ms"] = clocked(lambda: S.MaskedSpgemmPlan(n, n, n, rpa, cia, rpc, cic, rpa, cia))
    plans["general"], rec["create_general_ms"] = clocked(lambda: S.MaskedSpgemmPlan(n, n, n, rpa, cia, rpc, cic, rpa, cia, general=True))
    for route in plans:
        rec["info_%s" % route] = plans[route].info()
    assert rec["info_sorted"]["path"] == "sorted" and rec["info_general"]["path"] == "general"
    outs = {r: torch.empty(int(cia.numel()), dtype=torch.float64, device=dev) for r in plans}
    fns = {"sorted": lambda: plans["sorted"].multiply(dC, va, out=outs["sorted"])}

    # the yardstick: the full product dC * A^T, when it can be formed
    tp = S.TransposePlan(n, n, rpa, cia, va)
    colptr, rowidx, val_t = tp.csc()
    colcount = (colptr[1:] - colptr[:-1]).long()
    products = int(colcount[cic.long()].sum().item())                      # per entry (i, j) of dC, the entries of A^T's row j
    rec["spgemm_full_products"] = products
    full = None
    if products <= args.max_products:
        try:
            full, rec["create_spgemm_full_ms"] = clocked(lambda: S.SpgemmPlan(n, n, n, rpc, cic, colptr, rowidx))
        except S.SblasError as e:
            rec["spgemm_full"] = "not measured: the plan of the full product is refused (%s)" % str(e).splitlines()[0][:120]
    else:
        rec["spgemm_full"] = "not measured: the full product has %d products, above --max-products %d" % (products, args.max_products)
    if full is not None:
        rec["spgemm_full_nnz"] = full.nnz_c
        full_out = torch.empty(full.nnz_c, dtype=torch.float64, device=dev)
        fns["spgemm"] = lambda: full.multiply(dC, val_t, out=full_out)
    for route, (ms, each) in timed_pair(torch, fns, args.rounds).items():
        rec["numeric_%s_ms" % route], rec["numeric_%s_rounds" % route] = ms, each
    if full is not None:
        rec["spgemm_over_sorted"] = rec["numeric_spgemm_ms"] / rec["numeric_sorted_ms"]
        full.destroy()
        del full_out
    print(json.dumps(rec), flush=True)                                     # what is known so far, should the slow path run out of time

    # the general path, beside the sorted one again
    both = {"sorted_again": fns["sorted"], "general": lambda: plans["general"].multiply(dC, va, out=outs["general"])}
    for route, (ms, each) in timed_pair(torch, both, max(2, args.rounds // 2), budget_ms=1.0).items():
        rec["numeric_%s_ms" % route], rec["numeric_%s_rounds" % route] = ms, each
    torch.cuda.synchronize()
    rec["same_bits"] = bool(torch.equal(outs["sorted"].view(torch.int64), outs["general"].view(torch.int64)))
    rec["general_over_sorted"] = rec["numeric_general_ms"] / rec["numeric_sorted_again_ms"]
    for p in list(plans.values()) + [tp, c]:
        p.destroy()
    print(json.dumps(rec), flush=True)

    # the operator: forward alone against forward + backward
    op, rec["create_operator_ms"] = clocked(lambda: AG.SpgemmOperator(n, n, n, rpa, cia, rpa, cia))
    ga, gb = va.clone().requires_grad_(True), va.clone().requires_grad_(True)

    def fwd_bwd():
        ga.grad = gb.grad = None
        op.multiply(ga, gb).backward(dC)

    _, rec["first_backward_ms"] = clocked(fwd_bwd)                         # makes the two masked plans and the two transposes
    for route, (ms, each) in timed_pair(torch, {"forward": lambda: op.multiply(va, va), "fwd_bwd": fwd_bwd}, args.rounds).items():
        rec["operator_%s_ms" % route], rec["operator_%s_rounds" % route] = ms, each
    rec["fwd_bwd_over_forward"] = rec["operator_fwd_bwd_ms"] / rec["operator_forward_ms"]
    rec["info_grad_a"], rec["info_grad_b"] = op.grad_a_plan.info(), op.grad_b_plan.info()
    op.destroy()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="banded5,nd24k,powerlaw")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--nd24k-scale", type=float, default=0.05)
    ap.add_argument("--max-products", type=int, default=20000000000, help="the largest full product dC * A^T the yardstick forms")
    ap.add_argument("--limit", type=int, default=300, help="seconds an input may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help="(internal) measure this input in this process")
    args = ap.parse_args()
    if args.one:
        return measure(args.one, args)

    results, failed = [], None
    for name in args.inputs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", name, "--rounds", str(args.rounds), "--rows", str(args.rows),
               "--nd24k-scale", str(args.nd24k_scale), "--max-products", str(args.max_products)]
        try:
            run = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.limit)
        except subprocess.TimeoutExpired as e:
            lines = [l for l in (e.stdout or b"").decode().splitlines() if l.startswith("{")]
            failed = json.loads(lines[-1]) if lines else dict(input=name)
            failed["failed"] = "no full record within %d s; what is here was measured, the rest is not measured" % args.limit
        else:
            lines = [l for l in run.stdout.decode().splitlines() if l.startswith("{")]
            if run.returncode != 0 or not lines:
                failed = json.loads(lines[-1]) if lines else dict(input=name)
                failed["failed"] = "exit status %d; what is here was measured, the rest is not measured" % run.returncode
            else:
                results.append(json.loads(lines[-1]))
                print(lines[-1], flush=True)
        if failed:                                                          # nothing is started after a failure
            results.append(failed)
            print(json.dumps(failed), flush=True)
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
