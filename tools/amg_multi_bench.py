"""The AMG cycle on a block of columns (AmgPlan.apply_multi, amg_sweep_multi) and its seat under KrylovMultiPlan against the
same work one column after another, in ONE process on one GPU.  The yardstick is always existing code in the same run
(amg_sweep, AmgPlan.apply, KrylovPlan with the same AmgPlan), never the code under test; no threshold is fixed in advance.

  --part sweep   the multi sweep on level 0 at s in --widths against s launches of amg_sweep on contiguous vectors, on the
                 unscaled five-point Laplacian of side --grid-side and on the nd24k-like matrix: microseconds by device
                 events and bytes per second on the algorithmic bytes (A's entries once: 12 bytes an entry and wd; b, x
                 and y once each: 3 n s doubles -- the single side moves A s times)
  --part cycle   apply_multi against s apply calls, plain and smoothed plans
  --part solve   PCG to --rtol on the unscaled Laplacian with the smoothed plan: one KrylovMultiPlan solve with the plan
                 as precond against s KrylovPlan solves with the same plan one after another, at check_every 1 and 8, by
                 the host clock from start() to the status() that reports the end; and KrylovMultiPlan with Jacobi, once,
                 up to --jacobi-iter iterations (not expected to converge)
The repetitions of the two sides are interleaved (multi, sequential, multi, ...); medians, minima and maxima are reported.
Each part merges its record into --out, so the parts can run as separate steps.

  python tools/amg_multi_bench.py --part sweep --out profiles/r24_amg_multi.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("s-blas_amd/python", "tools"):
    sys.path.insert(0, os.path.join(ROOT, *p.split("/")))


def stats(xs):
    xs = [float(x) for x in xs]
    return dict(median=float(np.median(xs)), min=min(xs), max=max(xs), rounds=len(xs))


def event_us(torch, fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner


def interleaved(torch, sides, rounds, inner):
    for fn in sides.values():
        fn()                                                                # warm: the code objects are loaded
    torch.cuda.synchronize()
    us = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            us[k].append(event_us(torch, fn, inner))
    return us


def device_matrix(torch, dev, name, args):
    import amg_bench as AB
    label, n, rp, ci, val = AB.matrix(name, args)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(label=label, n=n, nnz=int(len(ci)), rp=rp, ci=ci, val=val, drp=up(rp), dci=up(ci), dval=up(val))


def part_sweep(S, torch, dev, args, widths):
    out = {}
    for name in [x for x in args.inputs.split(",") if x]:
        A = device_matrix(torch, dev, name, args)
        n, nnz = A["n"], A["nnz"]
        plan = S.AmgPlan(n, A["drp"], A["dci"])
        plan.setup(A["dval"])
        rec = dict(matrix=A["label"], n=n, nnz=nnz, units=plan.level(0)["units"], widths={})
        for s in widths:
            g = torch.Generator(device=dev).manual_seed(s)
            B, X = (torch.randn((n, s), dtype=torch.float64, device=dev, generator=g) for _ in range(2))
            Y = torch.empty((n, s), dtype=torch.float64, device=dev)
            b, x = ([t[:, j].contiguous() for j in range(s)] for t in (B, X))
            y = torch.empty(n, dtype=torch.float64, device=dev)
            sides = {"multi": lambda: S.amg_sweep_multi(plan, 0, B, X, Y),
                     "single": lambda: [S.amg_sweep(plan, 0, b[j], x[j], y) for j in range(s)]}
            us = interleaved(torch, sides, args.rounds, args.inner)
            bytes_multi, bytes_single = nnz * 12 + n * 8 + 3 * n * s * 8, s * (nnz * 12 + n * 8 + 3 * n * 8)
            rec["widths"][str(s)] = dict(multi_us=stats(us["multi"]), single_us=stats(us["single"]),
                                         multi_gb_per_s=bytes_multi / np.median(us["multi"]) * 1e-3,
                                         single_gb_per_s=bytes_single / np.median(us["single"]) * 1e-3,
                                         single_over_multi=float(np.median(us["single"]) / np.median(us["multi"])),
                                         grid=S.amg_multi_grid(rec["units"], s))
            print(json.dumps({"sweep": name, "s": s, **rec["widths"][str(s)]}), flush=True)
        out[name] = rec
        plan.destroy()
    return out


def part_cycle(S, torch, dev, args, widths):
    out = {}
    for name in [x for x in args.cycle_inputs.split(",") if x]:
        A = device_matrix(torch, dev, name, args)
        n = A["n"]
        for kind in ("plain", "smoothed"):
            plan = S.AmgPlan(n, A["drp"], A["dci"], prolongator=kind)
            plan.setup(A["dval"])
            plan.reserve(max(widths))
            rec = dict(matrix=A["label"], n=n, levels=plan.levels(), launches=plan.info()["launches"], widths={})
            for s in widths:
                g = torch.Generator(device=dev).manual_seed(s)
                R = torch.randn((n, s), dtype=torch.float64, device=dev, generator=g)
                Z = torch.empty((n, s), dtype=torch.float64, device=dev)
                r = [R[:, j].contiguous() for j in range(s)]
                z = torch.empty(n, dtype=torch.float64, device=dev)
                sides = {"multi": lambda: plan.apply_multi(R, out=Z), "single": lambda: [plan.apply(r[j], out=z) for j in range(s)]}
                us = interleaved(torch, sides, args.rounds, args.inner)
                rec["widths"][str(s)] = dict(multi_us=stats(us["multi"]), single_us=stats(us["single"]),
                                             single_over_multi=float(np.median(us["single"]) / np.median(us["multi"])))
                print(json.dumps({"cycle": name, "plan": kind, "s": s, **rec["widths"][str(s)]}), flush=True)
            rec["reserved_bytes"] = plan.multi_info()["bytes"]
            out["%s %s" % (name, kind)] = rec
            plan.destroy()
    return out


def part_solve(S, torch, dev, args, widths):
    A = device_matrix(torch, dev, "laplace", args)
    n, drp, dci, dval = A["n"], A["drp"], A["dci"], A["dval"]
    amg = S.AmgPlan(n, drp, dci, prolongator="smoothed")
    amg.setup(dval)
    spmv = S.SpmvPlan(n, n, drp, dci)
    single = S.KrylovPlan(n, drp, dci, spmv_plan=spmv, precond=amg)
    diag = A["val"][A["ci"] == np.repeat(np.arange(n), np.diff(A["rp"].astype(np.int64)))]
    dinv = torch.from_numpy(1.0 / diag).to(dev)
    out = dict(matrix=A["label"], n=n, nnz=A["nnz"], rtol=args.rtol, amg=dict(levels=amg.levels(), launches=amg.info()["launches"]), widths={})
    for s in widths:
        B = np.random.default_rng(100 + s).standard_normal((n, s))
        dB = torch.from_numpy(B).to(dev)
        db = [dB[:, j].contiguous() for j in range(s)]
        multi = S.KrylovMultiPlan(n, drp, dci, s, precond=amg)
        rec = dict(launches_per_iteration=dict(multi_own=multi.info()["launches"], single=single.info()["launches"]))
        for check_every in (1, 8):
            kw = dict(rtol=args.rtol, max_iter=args.max_iter, check_every=check_every)

            def run_multi():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                X, st = multi.solve(dval, dB, **kw)
                return time.perf_counter() - t0, X, st

            def run_single():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = [single.solve(dval, db[j], **kw) for j in range(s)]
                return time.perf_counter() - t0, res

            run_multi(), run_single()                                        # warm
            tm, ts = [], []
            for _ in range(args.rounds):                                     # interleaved
                sec, X, st = run_multi()
                tm.append(sec * 1e3)
                sec, res = run_single()
                ts.append(sec * 1e3)
            its_m, its_s = st["iterations"].tolist(), [o[1]["iterations"] for o in res]
            rec["check_every_%d" % check_every] = dict(
                multi_ms=stats(tm), sequential_ms=stats(ts), sequential_over_multi=float(np.median(ts) / np.median(tm)),
                multi_status=sorted(set(st["status"])), sequential_status=sorted(set(o[1]["status"] for o in res)),
                multi_iterations=dict(min=min(its_m), max=max(its_m)), sequential_iterations=dict(min=min(its_s), max=max(its_s)))
        multi.destroy()
        # Jacobi, once: what a caller had before the block cycle
        jac = S.KrylovMultiPlan(n, drp, dci, s, precond="jacobi")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, st = jac.solve(dval, dB, dinv=dinv, rtol=args.rtol, max_iter=args.jacobi_iter, check_every=50)
        rec["jacobi"] = dict(ms=(time.perf_counter() - t0) * 1e3, max_iter=args.jacobi_iter, status=sorted(set(st["status"])),
                             iterations=dict(min=int(st["iterations"].min()), max=int(st["iterations"].max())),
                             worst_rnorm_over_bnorm=float((st["rnorm"] / st["bnorm"]).max()))
        jac.destroy()
        out["widths"][str(s)] = rec
        print(json.dumps({"solve": s, **rec}), flush=True)
    single.destroy(), spmv.destroy(), amg.destroy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("sweep", "cycle", "solve"), required=True)
    ap.add_argument("--widths", default="1,2,4,8,16,32")
    ap.add_argument("--inputs", default="laplace,nd24k")
    ap.add_argument("--cycle-inputs", default="laplace")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--grid-side", type=int, default=1000)
    ap.add_argument("--nd24k-scale", type=float, default=1.0)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--max-iter", type=int, default=500)
    ap.add_argument("--jacobi-iter", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import sblas_amd as S
    dev = torch.device("cuda:0")
    widths = [int(w) for w in args.widths.split(",")]
    part = dict(sweep=part_sweep, cycle=part_cycle, solve=part_solve)[args.part](S, torch, dev, args, widths)
    if args.out:
        result = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                result = json.load(f)
        result.update(device=torch.cuda.get_device_name(0), rounds=args.rounds, limits=S.amg_multi_limits())
        result[args.part] = part
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
