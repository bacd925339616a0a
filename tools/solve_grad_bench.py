"""The values gradient of the solves on one GPU: the narrow SDDMM (sblas_hip_sddmm_narrow_f64_i32) against the SDDMM it
promises the bits of (sddmm_tensor), and what a backward costs next to its forward.

Per matrix, in one process, the routes alternating inside every round so that all see the same machine, medians over
`--rounds` rounds between two device events after a warm-up (tools/spgemm_bench.py's timed_pair), every round reported:
  k = 1, 2, 4, 8   narrow (part "all") and tensor on the same contiguous row-major operands; the record says that the
                   bits agree; the rate of the narrow kernel on its algorithmic bytes, 4 (colidx) + 8 (out) per entry
                   plus the two operands once, 8 k (rows + cols);
  lower triangle   at the same k: narrow with part "lower" against sddmm_tensor followed by masked_fill_ of the strict
                   upper entries, the route a triangular solve's gradient takes beyond the narrow kernel's widths;
  spmv             the planned SpMV on the same matrix, the byte yardstick (12 B per entry + 8 B per row read, 8 written);
  triangular       TriangularOperator on the lower triangle: forward alone, forward + backward (both gradients);
  pcg              SolveOperator(method="pcg", precond="jacobi") on the grid only (the matrix that is symmetric
                   positive definite): forward alone, forward + backward.
backward_over_forward is (forward + backward - forward) / forward on those medians.

One JSON object per matrix on stdout; --out writes the list.  Every matrix is measured in a child process of its own
under its own time limit, one at a time, and nothing is started after a child that failed or ran out of time.

  python tools/solve_grad_bench.py [--inputs nd24k,grid,banded5,powerlaw] [--rounds 5] [--out profiles/r30_solve_grad.json]

Matrices: tools/ilu0_bench.py's (nd24k_like made full, the five-point 1000^2 grid, the nine-diagonal band, the power law
made full)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "s-blas_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KS = (1, 2, 4, 8)


def measure(name, args):
    import torch
    import ilu0_bench as IB
    import sblas_amd as S
    from sblas_amd import autograd as AG
    from spgemm_bench import timed_pair
    dev = torch.device("cuda:0")
    up = lambda *arrays: tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)
    label, n, rp, ci, val = IB.build(name, args)
    if name == "grid":                                       # symmetric positive definite for PCG: the Laplacian's values
        row = np.repeat(np.arange(n), np.diff(rp))
        val = np.where(row == ci, 4.0, -1.0)
    drp, dci, dval = up(rp, ci, val)
    nnz = int(len(ci))
    rec = dict(matrix=label, n=n, nnz=nnz, limits=S.sddmm_narrow_limits(), device=torch.cuda.get_device_name(0), rounds=args.rounds)
    A = (n, n, drp, dci)
    rng = np.random.default_rng(5)
    fns, outs, tri = {}, {}, {}
    upper = dci > torch.repeat_interleave(torch.arange(n, dtype=torch.int32, device=dev), (drp[1:] - drp[:-1]).long())
    for k in KS:
        X, Y = up(rng.standard_normal((n, k)), rng.standard_normal((n, k)))
        outs[k] = (torch.empty(nnz, dtype=torch.float64, device=dev), torch.empty(nnz, dtype=torch.float64, device=dev))
        fns["narrow_k%d" % k] = lambda X=X, Y=Y, o=outs[k][0]: S.sddmm_narrow(A, X, Y, o)
        fns["tensor_k%d" % k] = lambda X=X, Y=Y, o=outs[k][1]: S.sddmm_tensor(A, X, Y, o)
        tri[k] = (torch.empty(nnz, dtype=torch.float64, device=dev), torch.empty(nnz, dtype=torch.float64, device=dev))
        fns["narrow_lower_k%d" % k] = lambda X=X, Y=Y, o=tri[k][0]: S.sddmm_narrow(A, X, Y, o, part="lower")
        fns["tensor_mask_k%d" % k] = lambda X=X, Y=Y, o=tri[k][1]: (S.sddmm_tensor(A, X, Y, o), o.masked_fill_(upper, 0.0))
    plan = S.SpmvPlan(n, n, drp, dci)
    x, y = torch.ones(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    fns["spmv"] = lambda: plan(dval, x, 1.0, 0.0, y)
    t = timed_pair(torch, fns, args.rounds)
    rec["ms"] = {k: v[0] for k, v in t.items()}
    rec["rounds_ms"] = {k: v[1] for k, v in t.items()}
    rec["same_bits"] = {"k%d" % k: bool(torch.equal(outs[k][0].view(torch.int64), outs[k][1].view(torch.int64))) for k in KS}
    rec["same_bits_lower"] = {"k%d" % k: bool(torch.equal(tri[k][0].view(torch.int64), tri[k][1].view(torch.int64))) for k in KS}
    rec["narrow_lower_over_tensor_mask"] = {"k%d" % k: t["narrow_lower_k%d" % k][0] / t["tensor_mask_k%d" % k][0] for k in KS}
    rec["narrow_over_tensor"] = {"k%d" % k: t["narrow_k%d" % k][0] / t["tensor_k%d" % k][0] for k in KS}
    rec["narrow_over_spmv"] = {"k%d" % k: t["narrow_k%d" % k][0] / t["spmv"][0] for k in KS}
    rec["narrow_tb_per_s"] = {"k%d" % k: (12.0 * nnz + 16.0 * k * n) / (t["narrow_k%d" % k][0] * 1e-3) / 1e12 for k in KS}
    rec["spmv_tb_per_s"] = (12.0 * nnz + 4.0 * n + 16.0 * n) / (t["spmv"][0] * 1e-3) / 1e12

    # ---- backward over forward ----
    b = torch.ones(n, dtype=torch.float64, device=dev)
    ops = {"triangular": AG.TriangularOperator(n, drp, dci, lower=True)}
    if name == "grid":
        ops["pcg_jacobi"] = AG.SolveOperator(n, drp, dci, method="pcg", precond="jacobi", rtol=1e-6, max_iter=20000, check_every=64)
    steps = {}
    for key, op in ops.items():
        v, bb = dval.clone().requires_grad_(), b.clone().requires_grad_()

        def forward(op=op):
            with torch.no_grad():
                op.solve(dval, b)

        def both(op=op, v=v, bb=bb):
            v.grad = bb.grad = None
            op.solve(v, bb).sum().backward()
        steps[key + "_forward"], steps[key + "_forward_backward"] = forward, both
    t = timed_pair(torch, steps, args.rounds)
    rec["solve_ms"] = {k: v[0] for k, v in t.items()}
    rec["solve_rounds_ms"] = {k: v[1] for k, v in t.items()}
    rec["backward_over_forward"] = {key: (t[key + "_forward_backward"][0] - t[key + "_forward"][0]) / t[key + "_forward"][0] for key in ops}
    if "pcg_jacobi" in ops:
        rec["pcg_iterations"] = {ph: int(st["iterations"]) for ph, st in ops["pcg_jacobi"].last.items()}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="nd24k,grid,banded5,powerlaw")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--grid-side", type=int, default=1000)
    ap.add_argument("--nd24k-scale", type=float, default=1.0)
    ap.add_argument("--limit", type=int, default=240, help="seconds a matrix may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help="(internal) measure this matrix in this process")
    args = ap.parse_args()
    if args.one:
        print(json.dumps(measure(args.one, args)))
        return 0
    records = []
    for name in args.inputs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", name, "--rounds", str(args.rounds), "--rows", str(args.rows),
               "--grid-side", str(args.grid_side), "--nd24k-scale", str(args.nd24k_scale)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print("%s: no result within %d s; nothing further is started" % (name, args.limit), file=sys.stderr)
            break
        if done.returncode != 0:
            print("%s: exit status %d; nothing further is started\n%s" % (name, done.returncode, done.stderr[-2000:]), file=sys.stderr)
            break
        records.append(json.loads(done.stdout.strip().splitlines()[-1]))
        print(json.dumps(records[-1]), flush=True)
    if args.out and records:
        with open(args.out, "w") as f:
            json.dump(records, f, indent=1)
    return 0 if len(records) == len(args.inputs.split(",")) else 1


if __name__ == "__main__":
    sys.exit(main())
