"""Aggregation AMG on the device (AmgPlan: sblas_hip_amg_plan_*) against the other preconditioners, on one GPU.

Per matrix: the hierarchy (level sizes, operator complexity, launches of a cycle), the host-clock time of create and of
the first setup, device-event times of setup, of one apply, of Ilu0Plan.apply and of the planned SpMV on the same matrix
(the median over `--rounds` rounds and every round, the routes alternating round by round), and PCG to 1e-8 with no
preconditioner, Jacobi, ILU(0), ILU(0) in the multicolour order and AMG in one process: iterations, status and the
host-clock time of each solve.

Every matrix is measured in a child process of its own under its own time limit, one at a time, and nothing is started
after a child that failed or ran out of time.  One JSON object per matrix on stdout; --out writes the list.

  python tools/amg_bench.py [--inputs nd24k,grid,bidiagonal,banded5,powerlaw,laplace] [--rounds 5] [--out profiles/r19_amg.json]
                            [--prolongator plain,smoothed] [--min-reduction 0.2] [--aggregation host,device] [--append]

--prolongator: the plans measured in the same process, one after the other ("plain", "smoothed" or both); the first one's
figures keep the record's old keys, every one's are under "prolongators".  --min-reduction: the coarsening guard of every
plan (default: the library's, 0 for plain and 0.2 for smoothed).

--aggregation host,device: a measurement of create alone instead of the one above.  Per matrix and
prolongator, create is timed on the host clock with the modes alternating, `--rounds` rounds, after one untimed create of
each mode on a small grid (the code objects load there); the two plans are compared array for array once.  Level 0's
aggregation alone is timed too: amg_aggregate_device with its round count, and the host rule on host arrays.  What remains
of a device-mode create is timed as parts at level 0: the structure's way to the host with its check, and the COO plan
of the level's triplets.  The yardstick is the host mode in the same run.  --append adds to the list in --out.

Matrices: those of tools/ilu0_bench.py made symmetric -- the same sorted symmetric patterns, every off-diagonal pair
given the value of its lower entry, the diagonal 1 + the row's absolute off-diagonal sum: symmetric positive definite --
and `laplace`: the unscaled five-point Laplacian (4 on the diagonal, -1 beside it) of side --grid-side, the tests' matrix."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "s-blas_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def symmetric(n, rp, ci, val):
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp.astype(np.int64)))
    col = ci.astype(np.int64)
    lo, hi = np.maximum(row, col), np.minimum(row, col)                      # the entry of the lower triangle names the pair
    key = row * n + col
    pos = np.searchsorted(key, lo * n + hi)                                  # rows ascend: the keys are sorted
    val = val[pos].copy()
    dg = row == col
    val[dg] = 1.0 + np.bincount(row, weights=np.where(dg, 0.0, np.abs(val)), minlength=n)
    return val


def laplace(side):
    """the five-point Laplacian of side x side points, rows ascending: (n, rowptr, colidx, val)"""
    idx = np.arange(side * side, dtype=np.int64)
    x, y = idx % side, idx // side
    cols = np.stack([idx - side, idx - 1, idx, idx + 1, idx + side], axis=1)
    keep = np.stack([y > 0, x > 0, np.ones_like(x, bool), x + 1 < side, y + 1 < side], axis=1)
    vals = np.broadcast_to(np.array([-1.0, -1.0, 4.0, -1.0, -1.0]), cols.shape)
    rp = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
    return side * side, rp, cols[keep].astype(np.int32), vals[keep].copy()


def solve_timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x, st = fn()
    torch.cuda.synchronize()
    return dict(iterations=st["iterations"], status=st["status"], rnorm=st["rnorm"], bnorm=st["bnorm"], ms=(time.perf_counter() - t0) * 1e3), x


def matrix(name, args):
    import ilu0_bench as IB
    if name == "laplace":
        n, rp, ci, val = laplace(args.grid_side)
        return "five-point Laplacian %d^2, unscaled" % args.grid_side, n, rp, ci, val
    label, n, rp, ci, val = IB.build(name, args)
    return label + ", symmetric", n, rp, ci, symmetric(n, rp, ci, val)


def host_ms(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def measure_create(name, args):
    """create in the aggregation modes of --aggregation, alternating; level 0's aggregation and the parts that remain"""
    import torch
    import sblas_amd as S
    dev = torch.device("cuda:0")
    label, n, rp, ci, val = matrix(name, args)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    drp, dci, dval = up(rp), up(ci), up(val)
    modes = args.aggregation.split(",")
    rec = dict(matrix=label, n=n, nnz=int(len(ci)), device=torch.cuda.get_device_name(0), rounds=args.rounds, aggregation=modes,
               min_reduction=args.min_reduction)
    wn, wrp, wci, _ = laplace(40)
    for kind in args.prolongator.split(","):                                # untimed: the code objects load
        for mode in modes:
            S.AmgPlan(wn, up(wrp), up(wci), prolongator=kind, aggregation=mode).destroy()
    S.amg_aggregate_device(wn, up(wrp), up(wci))
    per = {}
    for kind in args.prolongator.split(","):
        times = {mode: [] for mode in modes}
        shown = {}
        for r in range(args.rounds):
            for mode in (modes if r % 2 == 0 else modes[::-1]):
                ms, plan = host_ms(torch, lambda: S.AmgPlan(n, drp, dci, prolongator=kind, min_reduction=args.min_reduction, aggregation=mode))
                times[mode].append(ms)
                if r == 0:
                    shown[mode] = dict(levels=plan.levels(), info=plan.info(),
                                       ints=[[plan.level(l)[k].cpu() if plan.level(l)[k] is not None else None for k in ("rowptr", "colidx", "agg", "aggptr", "members")]
                                             for l in range(plan.info()["levels"])])
                plan.destroy()
        equal = all(len(shown[m]["ints"]) == len(shown[modes[0]]["ints"]) and
                    all((a is None and b is None) or torch.equal(a, b) for La, Lb in zip(shown[m]["ints"], shown[modes[0]]["ints"]) for a, b in zip(La, Lb))
                    for m in modes)
        per[kind] = dict(levels=shown[modes[0]]["levels"], operator_complexity=shown[modes[0]]["info"]["operator_complexity"], plans_equal=equal,
                         create_ms={m: float(np.median(times[m])) for m in modes}, create_rounds=times)
    rec["prolongators"] = per
    # level 0's aggregation alone
    dev_ms, host_rule_ms, rounds, n_agg = [], [], None, None
    for r in range(args.rounds):
        ms, (agg, aggptr, members, rounds) = host_ms(torch, lambda: S.amg_aggregate_device(n, drp, dci))
        dev_ms.append(ms)
        n_agg = int(aggptr.numel()) - 1
        t0 = time.perf_counter()
        h_agg = S.amg_aggregate(n, rp, ci)[0]
        host_rule_ms.append((time.perf_counter() - t0) * 1e3)
    rec["level0"] = dict(n_agg=n_agg, device_rounds=rounds, equal=bool(np.array_equal(agg.cpu().numpy(), h_agg)),
                         device_wrapper_ms=float(np.median(dev_ms)), device_wrapper_rounds=dev_ms,
                         host_rule_ms=float(np.median(host_rule_ms)), host_rule_rounds=host_rule_ms,
                         note="device_wrapper_ms includes the wrapper's own structure check on the host (rowptr and colidx fetched, sblas_ilu0_check)")
    # what remains of a device-mode create, at level 0: the structure's way to the host with its check, and the COO plan
    fetch_ms, coo_ms = [], []
    row = torch.repeat_interleave(torch.arange(n, device=dev, dtype=torch.int64), (drp[1:] - drp[:-1]).to(torch.int64))
    trow, tcol = agg[row].contiguous(), agg[dci.to(torch.int64)].contiguous()
    for r in range(args.rounds):
        def fetch():
            h_rp, h_ci = drp.cpu().numpy(), dci.cpu().numpy()
            bad = ctypes.c_int64(-1)
            return S.lib().sblas_ilu0_check(n, h_rp.ctypes.data, h_ci.ctypes.data, None, ctypes.byref(bad))
        fetch_ms.append(host_ms(torch, fetch)[0])
        ms, plan = host_ms(torch, lambda: S.CooPlan(n_agg, n_agg, trow, tcol, dup="sum"))
        coo_ms.append(ms)
        plan.destroy()
    rec["level0_parts"] = dict(fetch_and_check_ms=float(np.median(fetch_ms)), fetch_and_check_rounds=fetch_ms,
                               coo_plan_ms=float(np.median(coo_ms)), coo_plan_rounds=coo_ms)
    print(json.dumps(rec), flush=True)


def measure(name, args):
    if args.aggregation:
        return measure_create(name, args)
    import torch
    import sblas_amd as S
    import sptrsv_bench as TB
    dev = torch.device("cuda:0")
    label, n, rp, ci, val = matrix(name, args)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    drp, dci, dval = up(rp), up(ci), up(val)
    rec = dict(matrix=label, n=n, nnz=int(len(ci)), limits=S.amg_limits(), device=torch.cuda.get_device_name(0))
    kinds = args.prolongator.split(",")
    plans, per = {}, {}
    for kind in kinds:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plans[kind] = S.AmgPlan(n, drp, dci, prolongator=kind, min_reduction=args.min_reduction)
        torch.cuda.synchronize()
        per[kind] = dict(create_ms=(time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        plans[kind].setup(dval)
        torch.cuda.synchronize()
        per[kind]["first_setup_ms"] = (time.perf_counter() - t0) * 1e3
        per[kind]["info"], per[kind]["levels"], per[kind]["check"] = plans[kind].info(), plans[kind].levels(), plans[kind].check()
    amg = plans[kinds[0]]
    rec.update(per[kinds[0]])
    ilu = S.Ilu0Plan(n, drp, dci)
    lu = ilu.factor(dval)
    spmv = S.SpmvPlan(n, n, drp, dci)
    b = up(np.random.default_rng(5).random(n) * 2 - 1)
    z, y, tmp = torch.empty_like(b), torch.empty_like(b), torch.empty_like(b)
    ilu.solvers()
    fns = {"amg_setup": lambda: amg.setup(dval), "amg_apply": lambda: amg.apply(b, out=z)}
    for kind in kinds[1:]:
        fns["amg_%s_setup" % kind] = lambda kind=kind: plans[kind].setup(dval)
        fns["amg_%s_apply" % kind] = lambda kind=kind: plans[kind].apply(b, out=z)
    fns.update({"ilu0_apply": lambda: ilu.apply(lu, b, out=y, tmp=tmp), "spmv": lambda: spmv(dval, b, 1.0, 0.0, y)})
    for k, (ms, each) in TB.timed(torch, fns, args.rounds).items():
        rec["%s_ms" % k], rec["%s_rounds" % k] = ms, each
    rec["apply_over_ilu0_apply"] = rec["amg_apply_ms"] / rec["ilu0_apply_ms"]
    rec["apply_over_spmv"] = rec["amg_apply_ms"] / rec["spmv_ms"]
    for kind in kinds:
        tag = "amg" if kind == kinds[0] else "amg_%s" % kind
        per[kind].update(setup_ms=rec["%s_setup_ms" % tag], apply_ms=rec["%s_apply_ms" % tag], apply_rounds=rec["%s_apply_rounds" % tag],
                         apply_over_spmv=rec["%s_apply_ms" % tag] / rec["spmv_ms"])
    rec["ilu0_solve_launches"] = [p.info()["launches"] for p in ilu.solvers()]

    kw = dict(rtol=1e-8, max_iter=args.max_iter, check_every=32)
    pcg = {}
    plan = S.KrylovPlan(n, drp, dci, spmv_plan=spmv)
    pcg["none"], _ = solve_timed(torch, lambda: plan.solve(dval, b, **kw))
    plan.destroy()
    plan = S.KrylovPlan(n, drp, dci, spmv_plan=spmv, precond="jacobi")
    dinv = ilu.pivots(dval).reciprocal_()
    pcg["jacobi"], _ = solve_timed(torch, lambda: plan.solve(dval, b, dinv=dinv, **kw))
    plan.destroy()
    plan = S.KrylovPlan(n, drp, dci, spmv_plan=spmv, precond=ilu)
    pcg["ilu0"], _ = solve_timed(torch, lambda: plan.solve(dval, b, lu=lu, **kw))
    plan.destroy()
    for kind in kinds:
        plan = S.KrylovPlan(n, drp, dci, spmv_plan=spmv, precond=plans[kind])
        per[kind]["pcg"], _ = solve_timed(torch, lambda: plan.solve(dval, b, **kw))
        pcg["amg" if kind == kinds[0] else "amg_%s" % kind] = per[kind]["pcg"]
        plan.destroy()
    # ILU(0) in the multicolour order: the caller's composition (KrylovPlan's docstring)
    color = S.ColorPlan(n, drp, dci)
    perm = color.permute(drp, dci)
    crp, cci, _ = perm.csr()
    cilu = S.Ilu0Plan(n, crp, cci)
    cval = perm.values(dval)
    clu = cilu.factor(cval)
    cb = perm.to_permuted(b)
    plan = S.KrylovPlan(n, crp, cci, precond=cilu)
    pcg["ilu0_multicolour"], _ = solve_timed(torch, lambda: plan.solve(cval, cb, lu=clu, **kw))
    pcg["ilu0_multicolour"]["colours"] = color.info().get("colors")
    plan.destroy()
    rec["pcg"], rec["prolongators"] = pcg, per
    for p in (cilu, perm, color, ilu, spmv) + tuple(plans.values()):
        p.destroy()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="nd24k,grid,bidiagonal,banded5,powerlaw")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--grid-side", type=int, default=1000)
    ap.add_argument("--nd24k-scale", type=float, default=1.0)
    ap.add_argument("--max-iter", type=int, default=2000)
    ap.add_argument("--prolongator", default="plain", help="plain, smoothed or both, comma-separated")
    ap.add_argument("--min-reduction", type=float, default=None, help="the coarsening guard (default: the library's)")
    ap.add_argument("--aggregation", default=None, help="host,device: time create alone in these modes, alternating (DESIGN.md 3.26)")
    ap.add_argument("--append", action="store_true", help="add to the list already in --out")
    ap.add_argument("--limit", type=int, default=240, help="seconds a matrix may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help="(internal) measure this matrix in this process")
    args = ap.parse_args()
    if args.one:
        return measure(args.one, args)

    results, failed = [], None
    for name in args.inputs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", name, "--rounds", str(args.rounds), "--rows", str(args.rows),
               "--grid-side", str(args.grid_side), "--nd24k-scale", str(args.nd24k_scale), "--max-iter", str(args.max_iter), "--prolongator", args.prolongator]
        if args.min_reduction is not None:
            cmd += ["--min-reduction", str(args.min_reduction)]
        if args.aggregation:
            cmd += ["--aggregation", args.aggregation]
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
        if args.append and os.path.exists(args.out):
            with open(args.out) as f:
                results = json.load(f) + results
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
