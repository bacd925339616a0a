"""FSAI on the device (FsaiPlan: sblas_hip_fsai_plan_*) against existing code in the same process, on one GPU (DESIGN.md
3.39).  The routes alternate inside every round, `--rounds` rounds, device events.

  (a) setup (the gather-and-Cholesky launch and the transpose's value update) against Ilu0Plan.factor on the same matrix,
      for G on A's lower pattern and, where it is built, on the lower pattern of A^2.
  (b) apply against the two planned SpMV calls it is made of, timed alone (SpmvPlan on csr() and TransposePlan(csr()).spmv:
      it should equal them), against Ilu0Plan.apply and against AmgPlan.apply (smoothed aggregation, the defaults).
  (c) PCG to 1e-8, iterations and host-clock milliseconds at check_every 32, one warm solve each: no preconditioner,
      Jacobi, ILU(0) in the natural and in the multicolour order, smoothed-aggregation AMG, FSAI on A, FSAI on A^2.

The matrices: the diagonally dominant five-point grid (`grid`), the unscaled five-point Laplacian (`laplace`) and the
symmetrised nd24k-like matrix (`nd24k`).  The last one's rows are longer than 64: it runs with --max-row (the crude
structural thinning: the diagonal and the entries of largest column below it), which the record names, and without A^2.

Every matrix is measured in a child process of its own under its own time limit, one at a time, and nothing is started
after a child that failed or ran out of time.  One JSON object per matrix on stdout; --out writes the list.

  python tools/fsai_bench.py [--inputs grid,laplace,nd24k] [--rounds 3] [--max-row 32] [--out profiles/r31_fsai.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "s-blas_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def lower_of_square(torch, S, n, drp, dci):
    """the lower triangle of the pattern of A^2 on the device: SpgemmPlan's structure through a lower-triangle filter"""
    sq = S.SpgemmPlan(n, n, n, drp, dci, drp, dci)
    rp2, ci2 = sq.csr()
    rows = torch.repeat_interleave(torch.arange(n, device=ci2.device), (rp2[1:] - rp2[:-1]).long())
    keep = ci2.long() <= rows
    counts = torch.zeros(n, dtype=torch.long, device=ci2.device).index_add_(0, rows[keep], torch.ones_like(rows[keep]))
    rpl = torch.cat([counts.new_zeros(1), counts.cumsum(0)]).int()
    cil = ci2[keep].contiguous()
    sq.destroy()
    return rpl, cil


def measure(name, args):
    import torch
    import sblas_amd as S
    import amg_bench as AB
    import sptrsv_bench as TB
    dev = torch.device("cuda:0")
    label, n, rp, ci, val = AB.matrix(name, args)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    drp, dci, dval = up(rp), up(ci), up(val)
    nnz = int(len(ci))
    thin = args.max_row if name == "nd24k" else None
    rec = dict(matrix=label, n=n, nnz=nnz, device=torch.cuda.get_device_name(0), rounds=args.rounds, limits=S.fsai_limits(), max_row=thin,
               thinning=None if thin is None else "structural and crude: the diagonal and the %d entries of largest column below it" % (thin - 1))
    fsai = {"fsai_A": S.FsaiPlan(n, drp, dci, max_row=thin)}
    if name != "nd24k":
        fsai["fsai_A2"] = S.FsaiPlan(n, drp, dci, pattern=lower_of_square(torch, S, n, drp, dci))
    for k, p in fsai.items():
        p.setup(dval)
        rec[k] = dict(info=p.info(), failed_row=p.check())
    spmv = S.SpmvPlan(n, n, drp, dci)
    ilu = S.Ilu0Plan(n, drp, dci)
    ilu.solvers()
    lu = ilu.factor(dval)
    sa = S.AmgPlan(n, drp, dci, prolongator="smoothed")
    sa.setup(dval)
    rec["amg"] = dict(levels=sa.levels(), launches=sa.info()["launches"], bytes=sa.info()["bytes"])
    b = up(np.random.default_rng(5).random(n) * 2 - 1)
    y, z, tmp = torch.empty_like(b), torch.empty_like(b), torch.empty_like(b)

    # (a) and (b): FSAI's two products timed alone are plans of their own on G's arrays
    grp, gci, gval = fsai["fsai_A"].csr()
    g_spmv, g_t = S.SpmvPlan(n, n, grp, gci), S.TransposePlan(n, n, grp, gci, gval)

    def two_products():
        g_spmv(gval, b, 1.0, 0.0, y)
        g_t.spmv(y, 1.0, 0.0, z)
    fns = {"spmv_A": lambda: spmv(dval, b, 1.0, 0.0, y), "two_products_alone": two_products,
           "ilu0_factor": lambda: ilu.factor(dval, out=lu), "ilu0_apply": lambda: ilu.apply(lu, b, out=z, tmp=tmp), "amg_apply": lambda: sa.apply(b, out=z)}
    for k, p in fsai.items():
        fns["%s_setup" % k] = lambda p=p: p.setup(dval)
        fns["%s_apply" % k] = lambda p=p: p.apply(b, out=z)
    for k, (ms, each) in TB.timed(torch, fns, args.rounds).items():
        rec["%s_ms" % k], rec["%s_rounds" % k] = ms, each
    rec["apply_over_two_products"] = rec["fsai_A_apply_ms"] / rec["two_products_alone_ms"]
    rec["ilu0_apply_over_fsai_apply"] = rec["ilu0_apply_ms"] / rec["fsai_A_apply_ms"]
    rec["fsai_setup_over_ilu0_factor"] = rec["fsai_A_setup_ms"] / rec["ilu0_factor_ms"]

    # (c)
    rhs = up(np.random.default_rng(30).standard_normal(n))
    cp = S.ColorPlan(n, drp, dci, seed=0)
    pp = S.PermutePlan(n, drp, dci, cp.order()[1].clone())
    cp.destroy()
    drpb, dcib, _ = pp.csr()
    dvalb, rhsb = pp.values(dval), pp.to_permuted(rhs)
    ilub = S.Ilu0Plan(n, drpb, dcib)
    lub = ilub.factor(dvalb)
    spmvb = S.SpmvPlan(n, n, drpb, dcib)
    dinv = ilu.pivots(dval).reciprocal_()
    natural, coloured = (drp, dci, dval, rhs, spmv), (drpb, dcib, dvalb, rhsb, spmvb)
    routes = {"none": (natural, None, {}), "jacobi": (natural, "jacobi", dict(dinv=dinv)), "ilu0_natural": (natural, ilu, dict(lu=lu)),
              "ilu0_multicolour": (coloured, ilub, dict(lu=lub)), "amg_smoothed": (natural, sa, {})}
    for k, p in fsai.items():
        routes[k] = (natural, p, {})
    pcg = {}
    for k, ((a_rp, a_ci, a_val, a_b, a_spmv), pre, extra) in routes.items():
        plan = S.KrylovPlan(n, a_rp, a_ci, spmv_plan=a_spmv, precond=pre)
        plan.solve(a_val, a_b, rtol=1e-8, max_iter=2, check_every=1, **extra)   # warm: code objects
        t, _ = AB.solve_timed(torch, lambda: plan.solve(a_val, a_b, rtol=1e-8, max_iter=args.max_iter, check_every=32, **extra))
        pcg[k] = dict(t, launches=plan.info()["launches"], ms_per_iteration=t["ms"] / max(t["iterations"], 1))
        plan.destroy()
    rec["pcg_1e-8"] = pcg
    for p in list(fsai.values()) + [spmv, spmvb, ilu, ilub, sa, pp, g_spmv, g_t]:
        p.destroy()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="grid,laplace,nd24k")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--grid-side", type=int, default=1000)
    ap.add_argument("--nd24k-scale", type=float, default=1.0)
    ap.add_argument("--max-row", type=int, default=32, help="the thinning of the matrix whose rows are longer than 64")
    ap.add_argument("--max-iter", type=int, default=4000)
    ap.add_argument("--limit", type=int, default=300, help="seconds a matrix may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help="(internal) measure this matrix in this process")
    args = ap.parse_args()
    if args.one:
        return measure(args.one, args)

    results, failed = [], None
    for name in args.inputs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", name, "--rounds", str(args.rounds), "--rows", str(args.rows),
               "--grid-side", str(args.grid_side), "--nd24k-scale", str(args.nd24k_scale), "--max-row", str(args.max_row),
               "--max-iter", str(args.max_iter)]
        try:
            run = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.limit)
        except subprocess.TimeoutExpired:
            failed = dict(matrix=name, failed="no result within %d s" % args.limit)
        else:
            lines = [l for l in run.stdout.decode().splitlines() if l.startswith("{")]
            if run.returncode != 0 or not lines:
                failed = dict(matrix=name, failed="exit status %d" % run.returncode)
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
