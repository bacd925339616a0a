"""PCG in the library (KrylovPlan: sblas_hip_krylov_*) against the torch loop of the tests, in the same process, on one GPU.

Per matrix, in the natural and in the multicolour order, with ILU(0), Jacobi and no preconditioner:
  - the library's solve at check_every = 1, 8 and 32: iterations, time to converge by the host clock (start() to the
    status() that reports the end, so the extra iterations of a batch are paid for), and time per iteration;
  - the library's time per iteration alone: device events around iterate(k) with a tolerance that is never met;
  - the torch loop (tests/test_gpu_ilu0.py's device_pcg, with Jacobi added): ten-odd torch launches an iteration and a
    host round trip for the norm; iterations, time to converge, time per iteration.
The library's launches per iteration and the levels of the two solves are recorded next to them.

Every matrix is measured in a child process of its own under its own time limit, one at a time, and nothing is started
after a child that failed or ran out of time.  One JSON object per matrix on stdout; --out writes the list.

  python tools/krylov_bench.py [--inputs nd24k,grid,bidiagonal,banded5,powerlaw] [--out profiles/r16_krylov.json]

Matrices: those of tools/ilu0_bench.py with the values made symmetric (entry (i, j) and (j, i) share the value drawn for
the lower one; the diagonal is 1 + the row's absolute off-diagonal sum), so that every one is symmetric positive definite."""
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


def symmetric_values(n, rp, ci, val):
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp.astype(np.int64)))
    col = ci.astype(np.int64)
    key = row * n + col                                                     # ascending: rows sorted, columns ascending
    twin = np.searchsorted(key, np.maximum(row, col) * n + np.minimum(row, col))
    out = val[twin]
    dg = row == col
    out[dg] = 1.0 + np.bincount(row, weights=np.where(dg, 0.0, np.abs(out)), minlength=n)
    return out


def torch_pcg(S, torch, n, drp, dci, dval, db, ilu, lu, dinv, rtol, limit):
    """the tests' loop: -> (iterations, seconds, converged)"""
    spmv = S.SpmvPlan(n, n, drp, dci)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x, r = torch.zeros_like(db), db.clone()
    q, z, tmp = torch.empty_like(db), torch.empty_like(db), torch.empty_like(db)
    if ilu is not None:
        precond = lambda r: ilu.apply(lu, r, out=z, tmp=tmp)
    elif dinv is not None:
        precond = lambda r: torch.mul(dinv, r, out=z)
    else:
        precond = lambda r: r
    zz = precond(r)
    p, rz, stop = zz.clone(), torch.dot(r, zz), rtol * float(torch.linalg.norm(db))
    count, done = limit, False
    for it in range(1, limit + 1):
        spmv(dval, p, 1.0, 0.0, q)
        alpha = rz / torch.dot(p, q)
        x += alpha * p
        r -= alpha * q
        if float(torch.linalg.norm(r)) <= stop:
            count, done = it, True
            break
        zz = precond(r)
        rz, old = torch.dot(r, zz), rz
        p = zz + (rz / old) * p
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    spmv.destroy()
    return count, sec, done


def one_order(S, torch, n, drp, dci, dval, db, args):
    """every preconditioner on one system -> dict"""
    out = {}
    ilu = S.Ilu0Plan(n, drp, dci)
    lu = ilu.factor(dval)
    dinv = ilu.pivots(dval).reciprocal_()
    lower, upper = ilu.solvers()
    out["levels"] = dict(lower=lower.info()["levels"], upper=upper.info()["levels"],
                         lower_launches=lower.info()["launches"], upper_launches=upper.info()["launches"])
    spmv = S.SpmvPlan(n, n, drp, dci)
    for name in ("ilu0", "jacobi", "none"):
        kw = dict(lu=lu) if name == "ilu0" else dict(dinv=dinv) if name == "jacobi" else {}
        plan = S.KrylovPlan(n, drp, dci, spmv_plan=spmv, precond=ilu if name == "ilu0" else "jacobi" if name == "jacobi" else None)
        rec = dict(launches_per_iteration=plan.info()["launches"], bytes=plan.info()["bytes"])
        plan.solve(dval, db, rtol=args.rtol, max_iter=args.max_iter, **kw)                 # warm: the code objects are loaded
        for every in CHECK_EVERY:
            best = None
            for _ in range(args.rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                x, st = plan.solve(dval, db, rtol=args.rtol, max_iter=args.max_iter, check_every=every, **kw)
                sec = time.perf_counter() - t0
                best = sec if best is None else min(best, sec)
            rec["check_every_%d" % every] = dict(status=st["status"], iterations=st["iterations"], ms_to_converge=best * 1e3,
                                                 us_per_iteration=best * 1e6 / max(st["iterations"], 1))
        # the iteration alone: never converging, timed by device events around one batch
        k = max(min(args.max_iter, 50), 1)
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
        its, sec, done = torch_pcg(S, torch, n, drp, dci, dval, db, ilu if name == "ilu0" else None, lu,
                                   dinv if name == "jacobi" else None, args.rtol, args.max_iter)          # warm
        best = None
        for _ in range(args.rounds):
            its, sec, done = torch_pcg(S, torch, n, drp, dci, dval, db, ilu if name == "ilu0" else None, lu,
                                       dinv if name == "jacobi" else None, args.rtol, args.max_iter)
            best = sec if best is None else min(best, sec)
        rec["torch_loop"] = dict(converged=done, iterations=its, ms_to_converge=best * 1e3, us_per_iteration=best * 1e6 / max(its, 1))
        rec["library_over_torch_to_converge"] = {str(e): rec["check_every_%d" % e]["ms_to_converge"] / rec["torch_loop"]["ms_to_converge"]
                                                 for e in CHECK_EVERY}
        plan.destroy()
        out[name] = rec
    spmv.destroy(), ilu.destroy()
    return out


def measure(name, args):
    import torch
    import sblas_amd as S
    import ilu0_bench as IB
    dev = torch.device("cuda:0")
    label, n, rp, ci, val = IB.build(name, args)
    val = symmetric_values(n, rp, ci, val)
    b = np.random.default_rng(30).standard_normal(n)
    drp, dci, dval, db = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (rp, ci, val, b))
    rec = dict(matrix=label + ", values made symmetric", n=n, nnz=int(len(ci)), rtol=args.rtol, max_iter=args.max_iter,
               limits=S.krylov_limits(), device=torch.cuda.get_device_name(0))
    rec["natural"] = one_order(S, torch, n, drp, dci, dval, db, args)
    color = S.ColorPlan(n, drp, dci)
    rec["colors"] = color.info()["colors"]
    perm = color.permute(drp, dci)
    color.destroy()
    drpb, dcib, _ = perm.csr()
    rec["multicolour"] = one_order(S, torch, n, drpb, dcib, perm.values(dval), perm.to_permuted(db), args)
    perm.destroy()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="nd24k,grid,bidiagonal,banded5,powerlaw")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--grid-side", type=int, default=1000)
    ap.add_argument("--nd24k-scale", type=float, default=1.0)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--max-iter", type=int, default=500)
    ap.add_argument("--limit", type=int, default=240, help="seconds a matrix may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help="(internal) measure this matrix in this process")
    args = ap.parse_args()
    if args.one:
        return measure(args.one, args)

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
