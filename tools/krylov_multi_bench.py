"""Several right-hand sides at once (KrylovMultiPlan: sblas_hip_krylov_multi_*) against the same solves one after another
(KrylovPlan), in ONE process on one GPU.  The yardstick is the sequential single-right-hand-side run of the same process;
no threshold is fixed in advance.

For s in --widths (1, 2, 4, 8, 16, 32):
  - the multi-dot (one dot of every column, krylov_multi_dots) against s calls of krylov_dot on contiguous vectors, and
    the x / r update (krylov_multi_update "pcg_xr") against s calls of krylov_update, on n = --rows rows: microseconds by
    device events and bytes per second (a dot reads 2 n s doubles; the update reads 4 n s and writes 2 n s);
  - a PCG solve to --rtol on the five-point grid --grid-side^2 and on the nd24k-like matrix of tools/ilu0_bench.py, values
    made symmetric as in tools/krylov_bench.py: one KrylovMultiPlan solve of s columns against s KrylovPlan solves (with an
    SpmvPlan) one after another, by the host clock from start() to the status() that reports the end.
The repetitions of the two sides are interleaved (multi, sequential, multi, ...); medians, minima and maxima are reported.
At s = 8 the true residuals |b_j - A x_j| (float64, on the host) of both sides are compared column by column, and the
"it solves" cases of tests/test_gpu_krylov_multi.py are measured the same way.

  python tools/krylov_multi_bench.py [--out profiles/r23_krylov_multi.json]"""
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


def kernels(S, torch, dev, n, s, rounds, inner=20):
    """the multi-dot and the x / r update against s single calls"""
    g = torch.Generator(device=dev).manual_seed(s)
    blk = lambda: torch.randn((n, s), dtype=torch.float64, device=dev, generator=g)
    X, R, P, Q = blk(), blk(), blk(), blk()
    cols = [[t[:, j].contiguous() for j in range(s)] for t in (X, R, P, Q)]
    cells = -(-n // S.krylov_limits()["cell"])
    out_m, ws_m = torch.empty((1, s), dtype=torch.float64, device=dev), torch.empty(s * cells, dtype=torch.float64, device=dev)
    out_1, ws_1 = torch.empty(1, dtype=torch.float64, device=dev), torch.empty(cells, dtype=torch.float64, device=dev)
    scal_m = torch.zeros((s, 16), dtype=torch.float64, device=dev)
    scal_m[:, 4] = 1e-3                                                     # alpha; status 0: running
    scal_1 = scal_m[0].clone()
    part_m, part_1 = torch.empty(2 * s * cells, dtype=torch.float64, device=dev), torch.empty(2 * cells, dtype=torch.float64, device=dev)
    sides = {
        "dot_multi": lambda: S.krylov_multi_dots([(P, Q)], out=out_m, workspace=ws_m),
        "dot_single": lambda: [S.krylov_dot(cols[2][j], cols[3][j], out=out_1, workspace=ws_1) for j in range(s)],
        "update_multi": lambda: S.krylov_multi_update("pcg_xr", scal_m, [X, R, P, Q], partial=part_m),
        "update_single": lambda: [S.krylov_update("pcg_xr", scal_1, [c[j] for c in cols], partial=part_1) for j in range(s)],
    }
    for fn in sides.values():
        fn()                                                                # warm: the code objects are loaded
    torch.cuda.synchronize()
    us = {k: [] for k in sides}
    for _ in range(rounds):                                                  # interleaved
        for k, fn in sides.items():
            us[k].append(event_us(torch, fn, inner))
    rec = {}
    for k, moved in (("dot", 2), ("update", 6)):
        bytes_ = moved * n * s * 8
        rec[k] = dict(multi_us=stats(us[k + "_multi"]), single_us=stats(us[k + "_single"]),
                      multi_gb_per_s=bytes_ / np.median(us[k + "_multi"]) * 1e-3, single_gb_per_s=bytes_ / np.median(us[k + "_single"]) * 1e-3,
                      single_over_multi=float(np.median(us[k + "_single"]) / np.median(us[k + "_multi"])))
    return rec


def solves(S, torch, dev, A, s, args, residuals):
    n, rp, ci, val, drp, dci, dval = A
    B = np.random.default_rng(100 + s).standard_normal((n, s))
    dB = torch.from_numpy(B).to(dev)
    db = [dB[:, j].contiguous() for j in range(s)]
    multi = S.KrylovMultiPlan(n, drp, dci, s)
    spmv = S.SpmvPlan(n, n, drp, dci)
    single = S.KrylovPlan(n, drp, dci, spmv_plan=spmv)
    kw = dict(rtol=args.rtol, max_iter=args.max_iter, check_every=args.check_every)

    def run_multi():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        X, st = multi.solve(dval, dB, **kw)
        return time.perf_counter() - t0, X, st

    def run_single():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = [single.solve(dval, db[j], **kw) for j in range(s)]
        return time.perf_counter() - t0, out

    run_multi(), run_single()                                                # warm
    tm, ts = [], []
    for _ in range(args.rounds):                                             # interleaved
        sec, X, st = run_multi()
        tm.append(sec * 1e3)
        sec, out = run_single()
        ts.append(sec * 1e3)
    its_m, its_s = st["iterations"].tolist(), [o[1]["iterations"] for o in out]
    rec = dict(s=s, multi_ms=stats(tm), sequential_ms=stats(ts), sequential_over_multi=float(np.median(ts) / np.median(tm)),
               multi_status=sorted(set(st["status"])), sequential_status=sorted(set(o[1]["status"] for o in out)),
               multi_iterations=dict(min=min(its_m), max=max(its_m)), sequential_iterations=dict(min=min(its_s), max=max(its_s)),
               multi_ms_per_lockstep_iteration=float(np.median(tm) / max(max(its_m), 1)),
               sequential_ms_per_iteration=float(np.median(ts) / max(sum(its_s), 1)),
               launches_per_iteration=dict(multi_own=multi.info()["launches"], single=single.info()["launches"]))
    if residuals:
        row = np.repeat(np.arange(n), np.diff(rp.astype(np.int64)))
        true = lambda b, x: float(np.linalg.norm(b - np.bincount(row, val * x[ci], minlength=n)))
        xm = X.cpu().numpy()
        rec["true_residual_multi_over_single"] = [true(B[:, j], xm[:, j]) / true(B[:, j], out[j][0].cpu().numpy()) for j in range(s)]
    multi.destroy(), single.destroy(), spmv.destroy()
    return rec


def it_solves(S, torch, dev):
    """the cases of tests/test_gpu_krylov_multi.py::test_it_solves_as_well_as_the_single_solver, measured"""
    import krylov_numerics as KN
    import multi_compose as MC
    import solver_compose as SC
    out = {}
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    for method, make in (("pcg", KN.spd_perturbed), ("bicgstab", KN.convection_diffusion)):
        n, rp, ci, val = A = make(48)
        B, X0, names = MC.columns(n, lambda v: KN.matvec(*A, v))
        drp, dci, dval = up(rp), up(ci), up(val)
        for jacobi in (False, True):
            precond = "jacobi" if jacobi else None
            dinv = up(1.0 / val[SC.stored_diagonal(rp, ci)]) if jacobi else None
            plan = S.KrylovMultiPlan(n, drp, dci, B.shape[1], method=method, precond=precond)
            X, st = plan.solve(dval, up(B), X=up(X0), dinv=dinv, rtol=1e-10)
            single = S.KrylovPlan(n, drp, dci, method=method, precond=precond)
            true = lambda b, v: float(np.linalg.norm(b - KN.matvec(n, rp, ci, val, v)))
            rec = {}
            for j, name in enumerate(names):
                xs, sst = single.solve(dval, up(B[:, j]), x=up(X0[:, j]), dinv=dinv, rtol=1e-10)
                if sst["status"] != "converged":
                    continue
                mine, theirs = true(B[:, j], X.cpu().numpy()[:, j]), true(B[:, j], xs.cpu().numpy())
                rec[name] = dict(iterations_multi=int(st["iterations"][j]), iterations_single=sst["iterations"],
                                 ratio=mine / theirs if theirs > 0.0 else (1.0 if mine == 0.0 else float("inf")))
            out["%s%s" % (method, " with Jacobi" if jacobi else "")] = rec
            plan.destroy(), single.destroy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="1,2,4,8,16,32")
    ap.add_argument("--inputs", default="grid,nd24k")
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
    import krylov_bench as KB
    dev = torch.device("cuda:0")
    widths = [int(w) for w in args.widths.split(",")]
    result = dict(device=torch.cuda.get_device_name(0), rtol=args.rtol, check_every=args.check_every, rounds=args.rounds,
                  limits=S.krylov_multi_limits(), kernels=dict(rows=args.rows), solves={})
    for s in widths:
        result["kernels"][str(s)] = kernels(S, torch, dev, args.rows, s, args.rounds)
        print(json.dumps({"kernels": s, **result["kernels"][str(s)]}), flush=True)
    for name in [x for x in args.inputs.split(",") if x]:
        label, n, rp, ci, val = IB.build(name, args)
        val = KB.symmetric_values(n, rp, ci, val)
        A = (n, rp, ci, val) + tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (rp, ci, val))
        rec = dict(matrix=label + ", values made symmetric", n=n, nnz=int(len(ci)), widths={})
        for s in widths:
            rec["widths"][str(s)] = solves(S, torch, dev, A, s, args, residuals=s == 8)
            print(json.dumps({"matrix": name, **rec["widths"][str(s)]}), flush=True)
        result["solves"][name] = rec
    result["it_solves"] = it_solves(S, torch, dev)
    print(json.dumps({"it_solves": result["it_solves"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
