"""Restarted GMRES in the library (GmresPlan: sblas_hip_gmres_*) against the library's BiCGStab (KrylovPlan) on the same
plans, in the same process, on one GPU.

Per matrix, with ILU(0), Jacobi and no preconditioner, for GMRES(10), GMRES(30), GMRES(64) and BiCGStab:
  - the solve at check_every = 1, 8 and 32: iterations (Arnoldi steps for GMRES: one SpMV and one M^-1 each; BiCGStab's
    iterations have two of each), restarts, time to converge by the host clock (start() to the status() that reports
    the end, so the surplus launches of a batch are paid for), and time per iteration;
  - the time per iteration alone: device events around iterate(k) with a tolerance that is never met.
The launches of a step / close / restart and the levels of the two solves are recorded next to them.

--dots times the multi-dot alone (sblas_hip_gmres_dots_f64) at k = 8, 32 and 65 columns of n = 10^6 against the bytes it
reads, 8 n (k + 1): device events around `steps` calls, the median of the rounds.

Every matrix (and the multi-dot) is measured in a child process of its own under its own time limit, one at a time, and
nothing is started after a child that failed or ran out of time.  One JSON object per child on stdout; --out writes the list.

  python tools/gmres_bench.py [--inputs dots,nd24k,grid,bidiagonal,banded5,powerlaw] [--out profiles/r18_gmres.json]

Matrices: those of tools/ilu0_bench.py as they are -- nonsymmetric values on a symmetric pattern, diagonally dominant."""
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

CHECK_EVERY = (1, 8, 32)
RESTARTS = (10, 30, 64)
DOT_COLUMNS = (8, 32, 65)


def timed_solves(torch, plan, dval, db, args, kw):
    """one solver on one system -> dict: the solve at every check_every, then the iteration alone"""
    rec = {}
    plan.solve(dval, db, rtol=args.rtol, max_iter=args.max_iter, **kw)                     # warm: the code objects are loaded
    for every in CHECK_EVERY:
        best = None
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x, st = plan.solve(dval, db, rtol=args.rtol, max_iter=args.max_iter, check_every=every, **kw)
            sec = time.perf_counter() - t0
            best = sec if best is None else min(best, sec)
        rec["check_every_%d" % every] = dict(status=st["status"], iterations=st["iterations"], restarts=st.get("restarts"),
                                             rnorm_over_bnorm=st["rnorm"] / st["bnorm"] if st["bnorm"] else None,
                                             ms_to_converge=best * 1e3, us_per_iteration=best * 1e6 / max(st["iterations"], 1))
    k = max(min(args.max_iter, 64), 1)                                                      # a whole cycle of the longest restart
    x = torch.zeros_like(db)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    each = []
    for _ in range(args.rounds):
        plan.start(dval, db, x.zero_(), rtol=0.0, atol=0.0, max_iter=10 ** 9, **kw)
        e0.record()
        plan.iterate(k)
        e1.record()
        st = plan.status()
        each.append(e0.elapsed_time(e1) * 1e3 / k)
    rec["us_per_iteration_enqueued"] = dict(median=float(np.median(each)), rounds=each, k=k, status_after=st["status"])
    return rec


def measure(name, args):
    import torch
    import sblas_amd as S
    import ilu0_bench as IB
    dev = torch.device("cuda:0")
    label, n, rp, ci, val = IB.build(name, args)
    b = np.random.default_rng(30).standard_normal(n)
    drp, dci, dval, db = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (rp, ci, val, b))
    rec = dict(matrix=label, n=n, nnz=int(len(ci)), rtol=args.rtol, max_iter=args.max_iter, limits=S.gmres_limits(),
               device=torch.cuda.get_device_name(0))
    ilu = S.Ilu0Plan(n, drp, dci)
    lu = ilu.factor(dval)
    dinv = ilu.pivots(dval).reciprocal_()
    lower, upper = ilu.solvers()
    rec["levels"] = dict(lower=lower.info()["levels"], upper=upper.info()["levels"],
                         lower_launches=lower.info()["launches"], upper_launches=upper.info()["launches"])
    spmv = S.SpmvPlan(n, n, drp, dci)
    for pname in ("ilu0", "jacobi", "none"):
        kw = dict(lu=lu) if pname == "ilu0" else dict(dinv=dinv) if pname == "jacobi" else {}
        precond = ilu if pname == "ilu0" else "jacobi" if pname == "jacobi" else None
        out = {}
        plan = S.KrylovPlan(n, drp, dci, method="bicgstab", spmv_plan=spmv, precond=precond)
        out["bicgstab"] = dict(launches_per_iteration=plan.info()["launches"], bytes=plan.info()["bytes"],
                               **timed_solves(torch, plan, dval, db, args, kw))
        plan.destroy()
        for m in RESTARTS:
            plan = S.GmresPlan(n, drp, dci, restart=m, spmv_plan=spmv, precond=precond)
            info = plan.info()
            out["gmres_%d" % m] = dict(launches=dict(step=info["step_launches"], close=info["close_launches"], restart=info["restart_launches"]),
                                       bytes=info["bytes"], **timed_solves(torch, plan, dval, db, args, kw))
            plan.destroy()
            base = out["bicgstab"]["check_every_8"]["ms_to_converge"]
            out["gmres_%d" % m]["over_bicgstab_to_converge_at_8"] = out["gmres_%d" % m]["check_every_8"]["ms_to_converge"] / base
        rec[pname] = out
    spmv.destroy(), ilu.destroy()
    print(json.dumps(rec), flush=True)


def measure_dots(args):
    import torch
    import sblas_amd as S
    dev = torch.device("cuda:0")
    n, steps = args.rows, 20
    g = torch.Generator(device=dev).manual_seed(5)
    V = torch.randn((max(DOT_COLUMNS), n), dtype=torch.float64, device=dev, generator=g)
    w = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
    rec = dict(kernel="multi-dot", n=n, steps=steps, device=torch.cuda.get_device_name(0), columns={})
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for k in DOT_COLUMNS:
        out = torch.empty(k, dtype=torch.float64, device=dev)
        ws = torch.empty(k * -(-n // S.krylov_limits()["cell"]), dtype=torch.float64, device=dev)
        S.gmres_dots(V[:k], w, out=out, workspace=ws)                                      # warm
        single = torch.empty(1, dtype=torch.float64, device=dev)
        S.krylov_dot(V[0], w, out=single, workspace=ws)
        each, each_single = [], []
        for _ in range(args.rounds):
            e0.record()
            for _ in range(steps):
                S.gmres_dots(V[:k], w, out=out, workspace=ws)
            e1.record()
            torch.cuda.synchronize()
            each.append(e0.elapsed_time(e1) * 1e3 / steps)
            e0.record()
            for _ in range(steps):
                for i in range(k):
                    S.krylov_dot(V[i], w, out=single, workspace=ws)
            e1.record()
            torch.cuda.synchronize()
            each_single.append(e0.elapsed_time(e1) * 1e3 / steps)
        us, nbytes = float(np.median(each)), 8 * n * (k + 1)
        rec["columns"][str(k)] = dict(us=us, rounds=each, bytes_read=nbytes, gb_per_s=nbytes / us / 1e3,
                                      us_as_single_dots=float(np.median(each_single)))
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="dots,nd24k,grid,bidiagonal,banded5,powerlaw")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--grid-side", type=int, default=1000)
    ap.add_argument("--nd24k-scale", type=float, default=1.0)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--max-iter", type=int, default=500)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help="(internal) measure this input in this process")
    args = ap.parse_args()
    if args.one:
        return measure_dots(args) if args.one == "dots" else measure(args.one, args)

    results, failed = [], None
    for name in args.inputs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", name, "--rounds", str(args.rounds), "--rows", str(args.rows),
               "--grid-side", str(args.grid_side), "--nd24k-scale", str(args.nd24k_scale), "--rtol", str(args.rtol),
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
