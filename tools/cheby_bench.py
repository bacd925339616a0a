"""Chebyshev smoothing on the device (ChebyshevPlan: sblas_hip_cheby_plan_*) against existing code in the same process,
on one GPU.  The routes alternate inside every round, `--rounds` rounds, device events.

  (a) the step kernel against the AMG sweep on the same level-0 matrix: one STEP launch is (smooth of degree 9 - smooth of
      degree 1) / 8; the yardstick is amg_sweep on an AmgPlan of the same matrix, and the SpMV plan beside it.  The byte
      ratio (12 nnz + 16 units + 48 n) / (12 nnz + 16 units + 32 n) is reported next to the measured one, with the
      spread of the sweep's own rounds.
  (b) setup with the estimate against setup with a given lambda_max (dinv, the row bound and the table only), and
      AmgPlan.setup with the Chebyshev smoother (an estimate a level) against the same plan's with the Jacobi smoother
      (`laplace` only: the smoothed-aggregation plan of (c)).
  (c) PCG to 1e-8 (`laplace` only): no preconditioner, Jacobi, the polynomial of degree 2 / 4 / 8, smoothed-aggregation
      AMG with Jacobi V(1,1) and V(2,2) and with the Chebyshev smoother of degree 2 and 3 (nu = 1): iterations and
      host-clock milliseconds at check_every 32, the median of the rounds -- and for the AMG rows at check_every 1 as well,
      since the iterations enqueued behind the one that converged still run their cycles -- and one apply of each AMG
      setting on device events.

Every matrix is measured in a child process of its own under its own time limit, one at a time, and nothing is started
after a child that failed or ran out of time.  One JSON object per matrix on stdout; --out writes the list.

  python tools/cheby_bench.py [--inputs laplace,nd24k] [--rounds 3] [--out profiles/r22_cheby.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "s-blas_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


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
    rec = dict(matrix=label, n=n, nnz=nnz, device=torch.cuda.get_device_name(0), rounds=args.rounds, limits=S.cheby_limits())
    plans = {d: S.ChebyshevPlan(n, drp, dci, degree=d) for d in (1, 2, 4, 8, 9)}
    for p in plans.values():
        p.setup(dval)
    rec["estimate"] = plans[4].check()
    units = plans[4].info()["units"]
    amg = S.AmgPlan(n, drp, dci, max_levels=1)                               # level 0 alone: the sweep's yardstick
    amg.setup(dval)
    spmv = S.SpmvPlan(n, n, drp, dci)
    b = up(np.random.default_rng(5).random(n) * 2 - 1)
    x, y, z = up(np.random.default_rng(6).random(n)), torch.empty_like(b), torch.empty_like(b)

    # (a) and (b)
    fns = {"amg_sweep": lambda: S.amg_sweep(amg, 0, b, x, y), "smooth1": lambda: plans[1].smooth(b, x, out=z),
           "smooth9": lambda: plans[9].smooth(b, x, out=z), "spmv": lambda: spmv(dval, x, 1.0, 0.0, y),
           "amg_sweep_again": lambda: S.amg_sweep(amg, 0, b, x, y),
           "apply4": lambda: plans[4].apply(b, out=z),
           "setup_estimate": lambda: plans[4].setup(dval), "setup_given": lambda: plans[4].setup(dval, lambda_max=2.0),
           "amg_setup_jacobi": lambda: amg.setup(dval)}
    for k, (ms, each) in TB.timed(torch, fns, args.rounds).items():
        rec["%s_ms" % k], rec["%s_rounds" % k] = ms, each
    plans[4].setup(dval)
    step = [(a - c) / 8.0 for a, c in zip(rec["smooth9_rounds"], rec["smooth1_rounds"])]
    sweeps = rec["amg_sweep_rounds"] + rec["amg_sweep_again_rounds"]
    rec["step_ms"], rec["step_rounds"] = float(np.median(step)), [round(v, 5) for v in step]
    rec["sweep_ms"] = float(np.median(sweeps))
    rec["sweep_spread"] = (max(sweeps) - min(sweeps)) / rec["sweep_ms"]
    rec["step_over_sweep"] = rec["step_ms"] / rec["sweep_ms"]
    rec["byte_ratio"] = (12.0 * nnz + 16.0 * units + 48.0 * n) / (12.0 * nnz + 16.0 * units + 32.0 * n)
    rec["step_gbs"] = (12.0 * nnz + 16.0 * units + 48.0 * n) / rec["step_ms"] / 1e6
    rec["sweep_gbs"] = (12.0 * nnz + 16.0 * units + 32.0 * n) / rec["sweep_ms"] / 1e6
    rec["setup_launches"] = plans[4].info()["setup_launches"]

    # (c)
    if name == "laplace":
        kw = dict(rtol=1e-8, max_iter=args.max_iter, check_every=32)
        ilu = S.Ilu0Plan(n, drp, dci)
        dinv = ilu.pivots(dval).reciprocal_()
        sa = S.AmgPlan(n, drp, dci, prolongator="smoothed")
        routes = {"none": (None, {}), "jacobi": ("jacobi", dict(dinv=dinv))}
        for d in (2, 4, 8):
            routes["chebyshev%d" % d] = (plans[d], {})
        amg_kw = {"amg_sa_jacobi_v11": dict(nu=1), "amg_sa_jacobi_v22": dict(nu=2), "amg_sa_chebyshev2": dict(smoother="chebyshev", degree=2),
                  "amg_sa_chebyshev3": dict(smoother="chebyshev", degree=3)}
        for k in amg_kw:
            routes[k] = (sa, {})
        sa.setup(dval, smoother="chebyshev")                                 # the first one allocates: outside every timing
        rec["amg_levels"] = sa.levels()
        solvers = {k: S.KrylovPlan(n, drp, dci, spmv_plan=spmv, precond=pre) for k, (pre, _) in routes.items()}
        pcg = {k: dict(ms_rounds=[]) for k in routes}
        for r in range(args.rounds):
            for k in (list(routes) if r % 2 == 0 else list(routes)[::-1]):
                if k in amg_kw:
                    sa.setup(dval, **amg_kw[k])
                t, _ = AB.solve_timed(torch, lambda: solvers[k].solve(dval, b, **dict(kw, **routes[k][1])))
                pcg[k]["ms_rounds"].append(round(t.pop("ms"), 3))
                pcg[k].update(t)
                if k in amg_kw:                                              # a frozen batch still runs its cycles: stop at every iteration too
                    t, _ = AB.solve_timed(torch, lambda: solvers[k].solve(dval, b, **dict(kw, check_every=1)))
                    pcg[k].setdefault("ms_check_every_1_rounds", []).append(round(t["ms"], 3))
        for k in pcg:
            pcg[k]["ms"] = float(np.median(pcg[k]["ms_rounds"]))
            if k in amg_kw:
                pcg[k]["ms_check_every_1"] = float(np.median(pcg[k]["ms_check_every_1_rounds"]))
        rec["pcg"] = pcg
        # one apply of every AMG setting, and the two setups, alternating
        sa.setup(dval, smoother="chebyshev", degree=2)
        rec["amg_eig"] = [{k: v for k, v in E.items() if k != "table"} for E in sa.eig()]
        amg_fns = {}
        for k, kw2 in amg_kw.items():
            def one(kw2=kw2):
                sa.setup(dval, **kw2)
                sa.apply(b, out=z)
            amg_fns["setup_and_apply_" + k] = one
        amg_fns["amg_sa_setup_jacobi"] = lambda: sa.setup(dval)
        amg_fns["amg_sa_setup_chebyshev2"] = lambda: sa.setup(dval, smoother="chebyshev", degree=2)
        for k, (ms, each) in TB.timed(torch, amg_fns, args.rounds).items():
            rec["%s_ms" % k], rec["%s_rounds" % k] = ms, each
        for k in amg_kw:                                                     # apply alone: the pair less the setup of its smoother
            setup = rec["amg_sa_setup_chebyshev2_ms" if "chebyshev" in k else "amg_sa_setup_jacobi_ms"]
            rec["apply_%s_ms" % k], rec["launches_%s" % k] = rec["setup_and_apply_%s_ms" % k] - setup, None
        for k, kw2 in amg_kw.items():
            sa.setup(dval, **kw2)
            rec["launches_%s" % k] = sa.info()["launches"]
        for p in list(solvers.values()) + [sa, ilu]:
            p.destroy()
    for p in list(plans.values()) + [amg, spmv]:
        p.destroy()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="laplace,nd24k")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--grid-side", type=int, default=1000)
    ap.add_argument("--nd24k-scale", type=float, default=1.0)
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
               "--grid-side", str(args.grid_side), "--nd24k-scale", str(args.nd24k_scale), "--max-iter", str(args.max_iter)]
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
