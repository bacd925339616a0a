"""Multicolour reordering (ColorPlan, PermutePlan) on one GPU, and what it does to ILU(0) and its solves.

Per matrix: colours, rounds (device and synchronous) and the time of ColorPlan and PermutePlan create (host clock around
calls that synchronise; the median of --rounds and every round), then Ilu0Plan.factor and Ilu0Plan.apply in the natural
and in the multicolour order (device events around warm calls, the two orders alternating round by round) with the
levels of each.  On the grid also preconditioned CG on the five-point Laplacian of the same pattern to 1e-10 in both
orders: iterations and wall time of a torch loop that reads one norm per iteration (the same loop for both orders; its
host overhead is in both times).

Every matrix is measured in a child process of its own under its own time limit, one at a time, and nothing is started
after a child that failed or ran out of time.  One JSON object per matrix on stdout; --out writes the list.

  python tools/color_bench.py [--inputs nd24k,grid,bidiagonal,banded5,powerlaw] [--rounds 5] [--out profiles/r14_color.json]

Matrices: those of tools/ilu0_bench.py (already structurally symmetric, sorted, with a dominant diagonal)."""
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


def host_timed(torch, make, rounds):
    """median and every round of the host time of make(), which synchronises; what it returns is destroyed"""
    each = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan = make()
        each.append((time.perf_counter() - t0) * 1e3)
        plan.destroy()
    return float(np.median(each)), [round(x, 3) for x in each]


def pcg(torch, S, n, drp, dci, dval, db, ilu, lu, tol, limit):
    """-> (iterations, ms): preconditioned CG with M^-1 = Ilu0Plan.apply"""
    spmv = S.SpmvPlan(n, n, drp, dci)
    ilu.solvers()
    x, r = torch.zeros_like(db), db.clone()
    q, z, tmp = torch.empty_like(db), torch.empty_like(db), torch.empty_like(db)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    zz = ilu.apply(lu, r, out=z, tmp=tmp)
    p, rz, stop = zz.clone(), torch.dot(r, zz), tol * float(torch.linalg.norm(db))
    count = limit + 1
    for it in range(1, limit + 1):
        spmv(dval, p, 1.0, 0.0, q)
        alpha = rz / torch.dot(p, q)
        x += alpha * p
        r -= alpha * q
        if float(torch.linalg.norm(r)) <= stop:
            count = it
            break
        zz = ilu.apply(lu, r, out=z, tmp=tmp)
        rz, old = torch.dot(r, zz), rz
        p = zz + (rz / old) * p
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    spmv.destroy()
    return count, ms


def measure(name, args):
    import torch
    import sblas_amd as S
    import ilu0_bench as IB
    import sptrsv_bench as TB
    dev = torch.device("cuda:0")
    label, n, rp, ci, val = IB.build(name, args)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    drp, dci, dval = up(rp), up(ci), up(val)
    rec = dict(matrix=label, n=n, nnz=int(len(ci)), limits=S.color_limits(), seed=args.seed, device=torch.cuda.get_device_name(0))

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cp = S.ColorPlan(n, drp, dci, seed=args.seed)
    rec["color_first_create_ms"] = (time.perf_counter() - t0) * 1e3
    rec["color_info"] = cp.info()
    rec["color_create_ms"], rec["color_create_rounds"] = host_timed(torch, lambda: S.ColorPlan(n, drp, dci, seed=args.seed), args.rounds)
    t0 = time.perf_counter()
    rec["sync_rounds"] = S.color_ref(n, rp, ci, args.seed)[2]
    rec["host_rule_ms"] = (time.perf_counter() - t0) * 1e3
    perm = cp.order()[1].clone()
    pp = S.PermutePlan(n, drp, dci, perm)
    rec["permute_info"] = pp.info()
    rec["permute_create_ms"], rec["permute_create_rounds"] = host_timed(torch, lambda: S.PermutePlan(n, drp, dci, perm), args.rounds)
    drpb, dcib, _ = pp.csr()
    dvalb = pp.values(dval)
    rec["permute_values_ms"] = TB.timed(torch, dict(v=lambda: pp.values(dval, out=dvalb)), args.rounds)["v"][0]
    cp.destroy()

    orders = dict(natural=(drp, dci, dval), multicolour=(drpb, dcib, dvalb))
    ilu = {k: S.Ilu0Plan(n, a[0], a[1]) for k, a in orders.items()}
    lu = {k: torch.empty_like(dval) for k in orders}
    b = up(np.random.default_rng(5).random(n) * 2 - 1)
    z, tmp = torch.empty_like(b), torch.empty_like(b)
    once = {}
    for k in orders:
        ilu[k].solvers()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ilu[k].factor(orders[k][2], out=lu[k])
        ilu[k].apply(lu[k], b, out=z, tmp=tmp)
        torch.cuda.synchronize()
        once[k] = (time.perf_counter() - t0) * 1e3
        rec["levels_%s" % k] = ilu[k].info()["levels"]
        rec["launches_%s" % k] = dict(factor=ilu[k].info()["launches"], lower=ilu[k].solvers()[0].info()["launches"],
                                      upper=ilu[k].solvers()[1].info()["launches"])
        rec["finite_%s" % k] = bool(torch.isfinite(lu[k]).all())
    rec["first_factor_and_apply_ms"] = once
    if max(once.values()) <= args.slow_ms:                                  # otherwise too long to repeat: the first calls stand
        fns = {}
        for k in orders:
            fns["factor_%s" % k] = lambda k=k: ilu[k].factor(orders[k][2], out=lu[k])
            fns["apply_%s" % k] = lambda k=k: ilu[k].apply(lu[k], b, out=z, tmp=tmp)
        for k, (ms, each) in TB.timed(torch, fns, args.rounds).items():
            rec["%s_ms" % k], rec["%s_rounds" % k] = ms, each
        rec["factor_multicolour_over_natural"] = rec["factor_multicolour_ms"] / rec["factor_natural_ms"]
        rec["apply_multicolour_over_natural"] = rec["apply_multicolour_ms"] / rec["apply_natural_ms"]

    if name == "grid" and not args.no_pcg:                                  # the Laplacian of the same pattern: SPD
        lap = np.where(np.repeat(np.arange(n), np.diff(rp.astype(np.int64))) == ci, 4.0, -1.0)
        dlap = up(lap)
        dlapb = pp.values(dlap)
        rhs = up(np.random.default_rng(30).standard_normal(n))
        out = {}
        for k, (a, v, r) in dict(natural=(orders["natural"], dlap, rhs), multicolour=(orders["multicolour"], dlapb, pp.to_permuted(rhs))).items():
            f = ilu[k].factor(v)
            its, ms = pcg(torch, S, n, a[0], a[1], v, r, ilu[k], f, 1e-10, args.pcg_limit)
            out[k] = dict(iterations=its, ms=ms, ms_per_iteration=ms / max(min(its, args.pcg_limit), 1), converged=its <= args.pcg_limit)
        rec["pcg_laplacian_1e-10"] = out
        rec["pcg_multicolour_over_natural_ms"] = out["multicolour"]["ms"] / out["natural"]["ms"]
    for p in ilu.values():
        p.destroy()
    pp.destroy()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="nd24k,grid,bidiagonal,banded5,powerlaw")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--grid-side", type=int, default=1000)
    ap.add_argument("--nd24k-scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-pcg", action="store_true")
    ap.add_argument("--pcg-limit", type=int, default=5000)
    ap.add_argument("--slow-ms", type=float, default=2000.0, help="a first factor + apply above this is not repeated")
    ap.add_argument("--limit", type=int, default=240, help="seconds a matrix may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help="(internal) measure this matrix in this process")
    args = ap.parse_args()
    if args.one:
        return measure(args.one, args)

    results, failed = [], None
    for name in args.inputs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", name, "--rounds", str(args.rounds), "--rows", str(args.rows),
               "--grid-side", str(args.grid_side), "--nd24k-scale", str(args.nd24k_scale), "--slow-ms", str(args.slow_ms),
               "--seed", str(args.seed), "--pcg-limit", str(args.pcg_limit)]
        cmd += ["--no-pcg"] if args.no_pcg else []
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
        if args.out:                                                        # what stands so far survives a later failure
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(results, f, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
