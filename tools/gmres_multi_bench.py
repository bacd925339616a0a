"""GMRES(m) for several right-hand sides at once (GmresMultiPlan: sblas_hip_gmres_multi_*) against the same solves one
after another (GmresPlan), in ONE process on one GPU.  The yardstick is the sequential single-right-hand-side run of the
same process; no threshold is fixed in advance, and losses are reported as they come.

For s in --widths (1, 2, 4, 8, 16, 32):
  - "dots": the tiled multi-dot (gmres_multi_dots on k basis blocks of n = --rows rows, k = 8 / 32 / 65) against s calls of
    gmres_dots on contiguous columns: microseconds by device events and bytes per second (a pass reads (k + 1) n s doubles);
  - "grid", "nd24k": GMRES(10) and GMRES(30) to --rtol, without a preconditioner and with Jacobi, on the nonsymmetric
    --grid-side^2 grid and the nd24k-like matrix of tools/ilu0_bench.py as they are: one GmresMultiPlan solve of s columns
    against s GmresPlan solves (with an SpmvPlan) one after another, by the host clock from start() to the status() that
    reports the end.
The repetitions of the two sides are interleaved (multi, sequential, multi, ...); medians, minima and maxima of --rounds
(7) are reported.  --out is read first when it exists, so the parts may be measured in separate runs.

  python tools/gmres_multi_bench.py [--parts dots,grid,nd24k] [--out profiles/r27_gmres_multi.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("s-blas_amd/python", "tools", "tests"):
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


def dots(S, torch, dev, n, s, k, rounds, inner=5):
    """one multi-dot pass over k blocks of s columns against s single multi-dots over k contiguous columns"""
    g = torch.Generator(device=dev).manual_seed(1000 * k + s)
    V = torch.randn((k, n, s), dtype=torch.float64, device=dev, generator=g)
    W = torch.randn((n, s), dtype=torch.float64, device=dev, generator=g)
    cols = [V[:, :, c].contiguous() for c in range(s)]                       # (k, n) each, as gmres_dots takes them
    wcol = [W[:, c].contiguous() for c in range(s)]
    cells = -(-n // S.krylov_limits()["cell"])
    out_m, ws_m = torch.empty((k, s), dtype=torch.float64, device=dev), torch.empty(k * s * cells, dtype=torch.float64, device=dev)
    out_1, ws_1 = torch.empty(k, dtype=torch.float64, device=dev), torch.empty(k * cells, dtype=torch.float64, device=dev)
    sides = {"multi": lambda: S.gmres_multi_dots(V, W, out=out_m, workspace=ws_m),
             "single": lambda: [S.gmres_dots(cols[c], wcol[c], out=out_1, workspace=ws_1) for c in range(s)]}
    for fn in sides.values():
        fn()                                                                # warm: the code objects are loaded
    torch.cuda.synchronize()
    us = {name: [] for name in sides}
    for _ in range(rounds):                                                  # interleaved
        for name, fn in sides.items():
            us[name].append(event_us(torch, fn, inner))
    bytes_ = (k + 1) * n * s * 8
    return dict(multi_us=stats(us["multi"]), single_us=stats(us["single"]), multi_gb_per_s=bytes_ / np.median(us["multi"]) * 1e-3,
                single_gb_per_s=bytes_ / np.median(us["single"]) * 1e-3, single_over_multi=float(np.median(us["single"]) / np.median(us["multi"])))


def solves(S, torch, dev, A, s, restart, precond, args):
    n, rp, ci, val, drp, dci, dval, ddinv = A
    B = np.random.default_rng(100 + s).standard_normal((n, s))
    dB = torch.from_numpy(B).to(dev)
    db = [dB[:, c].contiguous() for c in range(s)]
    multi = S.GmresMultiPlan(n, drp, dci, s, restart=restart, precond=precond)
    spmv = S.SpmvPlan(n, n, drp, dci)
    single = S.GmresPlan(n, drp, dci, restart=restart, spmv_plan=spmv, precond=precond)
    kw = dict(rtol=args.rtol, max_iter=args.max_iter, check_every=args.check_every, dinv=ddinv if precond == "jacobi" else None)

    def run_multi():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        X, st = multi.solve(dval, dB, **kw)
        return time.perf_counter() - t0, X, st

    def run_single():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = [single.solve(dval, db[c], **kw) for c in range(s)]
        return time.perf_counter() - t0, out

    run_multi(), run_single()                                                # warm
    tm, ts = [], []
    for _ in range(args.rounds):                                             # interleaved
        sec, X, st = run_multi()
        tm.append(sec * 1e3)
        sec, out = run_single()
        ts.append(sec * 1e3)
    its_m, its_s = st["iterations"].tolist(), [o[1]["iterations"] for o in out]
    info = multi.info()
    rec = dict(s=s, restart=restart, precond=precond, multi_ms=stats(tm), sequential_ms=stats(ts),
               sequential_over_multi=float(np.median(ts) / np.median(tm)),
               multi_status=sorted(set(st["status"])), sequential_status=sorted(set(o[1]["status"] for o in out)),
               multi_steps=dict(min=min(its_m), max=max(its_m)), sequential_steps=dict(min=min(its_s), max=max(its_s)),
               multi_ms_per_lockstep_step=float(np.median(tm) / max(max(its_m), 1)),
               sequential_ms_per_step=float(np.median(ts) / max(sum(its_s), 1)),
               launches_per_step=dict(multi_own=info["step_launches"], single=single.info()["step_launches"]), plan_bytes=info["bytes"])
    multi.destroy(), single.destroy(), spmv.destroy()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="dots,grid,nd24k")
    ap.add_argument("--widths", default="1,2,4,8,16,32")
    ap.add_argument("--blocks", default="8,32,65")
    ap.add_argument("--restarts", default="10,30")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--grid-side", type=int, default=1000)
    ap.add_argument("--nd24k-scale", type=float, default=1.0)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--max-iter", type=int, default=500)
    ap.add_argument("--check-every", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import sblas_amd as S
    import ilu0_bench as IB
    import solver_compose as SC
    dev = torch.device("cuda:0")
    widths = [int(w) for w in args.widths.split(",")]
    result = dict(solves={}, dots={})
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            result = json.load(f)
    result.update(device=torch.cuda.get_device_name(0), rtol=args.rtol, max_iter=args.max_iter, check_every=args.check_every,
                  rounds=args.rounds, limits=S.gmres_multi_limits())

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)

    for part in [x for x in args.parts.split(",") if x]:
        if part == "dots":
            result["dots"]["rows"] = args.rows
            for k in [int(v) for v in args.blocks.split(",")]:
                for s in widths:
                    rec = dots(S, torch, dev, args.rows, s, k, args.rounds)
                    result["dots"]["k%d_s%d" % (k, s)] = dict(k=k, s=s, **rec)
                    print(json.dumps({"dots": dict(k=k, s=s), **rec}), flush=True)
                    torch.cuda.empty_cache()
                save()
            continue
        label, n, rp, ci, val = IB.build(part, args)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        A = (n, rp, ci, val, up(rp), up(ci), up(val), up(1.0 / val[SC.stored_diagonal(rp, ci)]))
        rec = result["solves"].setdefault(part, dict(matrix=label, n=n, nnz=int(len(ci)), cases={}))
        for restart in [int(v) for v in args.restarts.split(",")]:
            for precond in (None, "jacobi"):
                for s in widths:
                    one = solves(S, torch, dev, A, s, restart, precond, args)
                    rec["cases"]["m%d_%s_s%d" % (restart, precond or "none", s)] = one
                    print(json.dumps({"matrix": part, **one}), flush=True)
                save()
    save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
