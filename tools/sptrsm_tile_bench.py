"""The tiled triangular solve (SptrsvPlan.solve_multi), Ilu0Plan.apply_multi and ILU(0)'s seat under KrylovMultiPlan against
the same work done by existing code, in ONE process on one GPU.  The yardsticks are always existing code in the same run,
never the code under test, and no threshold is fixed in advance:
  - s single solve() calls one after another on contiguous columns, and
  - the existing 2-D solve() (lanes along the right-hand sides) on the same block.

  --part solve   solve_multi at s in --widths against the two yardsticks on the lower triangles of the five-point grid
                 of side --grid-side, the nd24k-like matrix and the power law, by device events
  --part apply   Ilu0Plan.apply_multi against s apply() calls (and the 2-D apply()) on the full grid
  --part pcg     PCG to --rtol with the pair ilu.solvers() seated in a KrylovMultiPlan against s KrylovPlan + ILU(0) solves
                 one after another, on the grid (values made symmetric) in the natural and in the multicolour order, by
                 the host clock from start() to the status() that reports the end
  --part all     the three, in this order (the default)
The million-level inputs (bidiagonal, banded5) are left out: one solve of them does not finish in a visit.  The
repetitions of the sides are interleaved (tiled, singles, 2-D, tiled, ...); medians, minima and maxima are reported.  Each
part merges its record into --out, so the parts can also run as separate steps, each under a time limit of its own.

  python tools/sptrsm_tile_bench.py --out profiles/r25_sptrsm_tile.json"""
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


def event_ms(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def interleaved(torch, sides, rounds):
    for fn in sides.values():
        fn()                                                                # warm: the code objects are loaded
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            ms[k].append(event_ms(torch, fn))
    return ms


def lower_matrix(name, args):
    import sptrsv_bench as TB
    from sblas_amd import synth
    rng = np.random.default_rng(211)
    if name == "grid":
        n = args.grid_side ** 2
        return ("five-point grid %d^2, lower" % args.grid_side, n) + TB.grid_lower(args.grid_side, rng)
    if name == "nd24k":
        n, (rp, ci, v) = synth.nd24k_like(args.nd24k_scale)
        return ("nd24k_like(%g) lower, %d rows" % (args.nd24k_scale, n), n) + TB.lower_of(n, rp, ci, v)
    assert name == "powerlaw", name
    n = args.rows
    return ("powerlaw(%d) strict lower + diagonal" % n, n) + TB.lower_of(n, *synth.powerlaw(n, avg=3.0, max_len=5000))


def record(ms, s):
    rec = {k + "_ms": stats(v) for k, v in ms.items()}
    tiled = np.median(ms["tiled"])
    rec["singles_over_tiled"] = float(np.median(ms["singles"]) / tiled)
    rec["old_2d_over_tiled"] = float(np.median(ms["old_2d"]) / tiled)
    rec["tiled_over_one_single"] = float(tiled / (np.median(ms["singles"]) / s))
    return rec


def part_solve(S, torch, dev, args, widths):
    out = {}
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for name in [x for x in args.inputs.split(",") if x]:
        label, n, rp, ci, val = lower_matrix(name, args)
        drp, dci, dval = up(rp), up(ci), up(val)
        plan = S.SptrsvPlan(n, drp, dci)
        info = plan.info()
        rec = dict(matrix=label, n=n, nnz=int(len(ci)), levels=info["levels"], launches=info["launches"], wide_launches=info["wide_launches"],
                   chain_launches=info["chain_launches"], widths={})
        for s in widths:
            g = torch.Generator(device=dev).manual_seed(s)
            B = torch.randn((n, s), dtype=torch.float64, device=dev, generator=g)
            X, X2 = (torch.empty((n, s), dtype=torch.float64, device=dev) for _ in range(2))
            b = [B[:, j].contiguous() for j in range(s)]
            x = torch.empty(n, dtype=torch.float64, device=dev)
            sides = {"tiled": lambda: plan.solve_multi(dval, B, X=X),
                     "singles": lambda: [plan.solve(dval, b[j], x=x) for j in range(s)],
                     "old_2d": lambda: plan.solve(dval, B, x=X2)}
            rec["widths"][str(s)] = record(interleaved(torch, sides, args.rounds), s)
            print(json.dumps({"solve": name, "s": s, **rec["widths"][str(s)]}), flush=True)
        out[name] = rec
        plan.destroy()
        del drp, dci, dval
        torch.cuda.empty_cache()
    return out


def full_grid(S, torch, dev, args):
    """the full five-point grid with symmetric values (krylov_bench.py's `grid`) on the device"""
    import ilu0_bench as IB
    import krylov_bench as KB
    label, n, rp, ci, val = IB.build("grid", args)
    val = KB.symmetric_values(n, rp, ci, val)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(label=label + ", values made symmetric", n=n, nnz=int(len(ci)), drp=up(rp), dci=up(ci), dval=up(val))


def part_apply(S, torch, dev, args, widths):
    A = full_grid(S, torch, dev, args)
    n = A["n"]
    ilu = S.Ilu0Plan(n, A["drp"], A["dci"])
    lu = ilu.factor(A["dval"])
    lower, upper = ilu.solvers()
    rec = dict(matrix=A["label"], n=n, nnz=A["nnz"], lower_launches=lower.info()["launches"], upper_launches=upper.info()["launches"], widths={})
    for s in widths:
        g = torch.Generator(device=dev).manual_seed(s)
        R = torch.randn((n, s), dtype=torch.float64, device=dev, generator=g)
        Z, Z2, T2 = (torch.empty((n, s), dtype=torch.float64, device=dev) for _ in range(3))
        r = [R[:, j].contiguous() for j in range(s)]
        z, t = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2))
        sides = {"tiled": lambda: ilu.apply_multi(lu, R, out=Z),
                 "singles": lambda: [ilu.apply(lu, r[j], out=z, tmp=t) for j in range(s)],
                 "old_2d": lambda: ilu.apply(lu, R, out=Z2, tmp=T2)}
        rec["widths"][str(s)] = record(interleaved(torch, sides, args.rounds), s)
        print(json.dumps({"apply": s, **rec["widths"][str(s)]}), flush=True)
    ilu.destroy()
    return rec


def pcg_order(S, torch, dev, args, n, drp, dci, dval, widths):
    ilu = S.Ilu0Plan(n, drp, dci)
    lu = ilu.factor(dval)
    pair = ilu.solvers()
    spmv = S.SpmvPlan(n, n, drp, dci)
    single = S.KrylovPlan(n, drp, dci, spmv_plan=spmv, precond=pair)
    out = dict(lower_launches=pair[0].info()["launches"], upper_launches=pair[1].info()["launches"], widths={})
    kw = dict(lu=lu, rtol=args.rtol, max_iter=args.max_iter, check_every=args.check_every)
    for s in widths:
        dB = torch.from_numpy(np.random.default_rng(100 + s).standard_normal((n, s))).to(dev)
        db = [dB[:, j].contiguous() for j in range(s)]
        multi = S.KrylovMultiPlan(n, drp, dci, s, precond=pair)

        def run_multi():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            X, st = multi.solve(dval, dB, **kw)
            return time.perf_counter() - t0, st

        def run_single():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = [single.solve(dval, db[j], **kw)[1] for j in range(s)]
            return time.perf_counter() - t0, res

        run_multi(), single.solve(dval, db[0], **kw)                        # warm
        tm, ts = [], []
        for _ in range(args.pcg_rounds):                                    # interleaved
            sec, st = run_multi()
            tm.append(sec * 1e3)
            sec, res = run_single()
            ts.append(sec * 1e3)
        its_m, its_s = st["iterations"].tolist(), [o["iterations"] for o in res]
        out["widths"][str(s)] = dict(multi_ms=stats(tm), sequential_ms=stats(ts), sequential_over_multi=float(np.median(ts) / np.median(tm)),
                                     launches_per_iteration=dict(multi_own=multi.info()["launches"], single=single.info()["launches"]),
                                     multi_status=sorted(set(st["status"])), sequential_status=sorted(set(o["status"] for o in res)),
                                     multi_iterations=dict(min=min(its_m), max=max(its_m)),
                                     sequential_iterations=dict(min=min(its_s), max=max(its_s)))
        print(json.dumps({"pcg": s, **out["widths"][str(s)]}), flush=True)
        multi.destroy()
    single.destroy(), spmv.destroy(), ilu.destroy()
    return out


def part_pcg(S, torch, dev, args, widths):
    A = full_grid(S, torch, dev, args)
    n, drp, dci, dval = A["n"], A["drp"], A["dci"], A["dval"]
    rec = dict(matrix=A["label"], n=n, nnz=A["nnz"], rtol=args.rtol, check_every=args.check_every)
    natural = [int(w) for w in args.natural_widths.split(",")] if args.natural_widths else widths
    rec["natural"] = pcg_order(S, torch, dev, args, n, drp, dci, dval, natural)
    color = S.ColorPlan(n, drp, dci)
    rec["colors"] = color.info()["colors"]
    perm = color.permute(drp, dci)
    color.destroy()
    drpb, dcib, _ = perm.csr()
    rec["multicolour"] = pcg_order(S, torch, dev, args, n, drpb, dcib, perm.values(dval), widths)
    perm.destroy()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("all", "solve", "apply", "pcg"), default="all")
    ap.add_argument("--widths", default="1,2,4,8,16,32,64")
    ap.add_argument("--natural-widths", default="", help="widths of the PCG part in the natural order (default: --widths)")
    ap.add_argument("--inputs", default="grid,nd24k,powerlaw")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pcg-rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--grid-side", type=int, default=1000)
    ap.add_argument("--nd24k-scale", type=float, default=1.0)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--max-iter", type=int, default=2000)
    ap.add_argument("--check-every", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import sblas_amd as S
    if not torch.cuda.is_available():
        raise SystemExit("sptrsm_tile_bench needs a GPU")
    dev = torch.device("cuda:0")
    widths = [int(w) for w in args.widths.split(",")]
    parts = dict(solve=part_solve, apply=part_apply, pcg=part_pcg)
    for name in (parts if args.part == "all" else [args.part]):
        part = parts[name](S, torch, dev, args, widths)
        if args.out:                                                        # merged part by part: a part that ran is kept
            result = {}
            if os.path.exists(args.out):
                with open(args.out) as f:
                    result = json.load(f)
            result.update(device=torch.cuda.get_device_name(0), rounds=args.rounds, limits=S.sptrsm_tile_limits())
            if name == "solve":                                             # by matrix: --inputs may name one a step
                result.setdefault(name, {}).update(part)
            else:
                result[name] = part
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
