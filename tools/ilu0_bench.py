"""ILU(0) on the device (Ilu0Plan: sblas_hip_ilu0_plan_*) on one GPU.

Per matrix: levels and launches, time per factorisation under `auto` and `per_level` (device events around `steps` warm
calls; the median over `--rounds` rounds and every round are reported, the two modes alternating round by round), the
lower unit SptrsvPlan solve on the same matrix in the same run (it has the same levels: the latency floor), the planned
SpMV (it reads the same bytes once: the byte floor), and the chain_rows sweep from which the default is to be chosen.

Every matrix is measured in a child process of its own under its own time limit, one at a time, and nothing is started
after a child that failed or ran out of time.  One JSON object per matrix on stdout; --out writes the list.

  python tools/ilu0_bench.py [--inputs nd24k,grid,bidiagonal,banded5,powerlaw] [--rounds 5] [--out profiles/r13_ilu0.json]

Matrices: the lower triangles of tools/sptrsv_bench.py made full (the pattern plus its transpose) and sorted, so that
`bidiagonal` is a tridiagonal matrix and `banded5` has nine diagonals; off-diagonals uniform in [-1, 1), the diagonal
1 + the row's absolute off-diagonal sum, so no factorisation breaks down."""
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

SWEEP = (16, 32, 64, 128, 256, 512, 1024, 2048, 4096)


def full_sorted(n, rp, ci, rng):
    """the pattern plus its transpose plus the diagonal, rows ascending, nothing doubled; dominant values"""
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp.astype(np.int64)))
    col = ci.astype(np.int64)
    off = row != col
    r = np.concatenate([row[off], col[off], np.arange(n)])
    c = np.concatenate([col[off], row[off], np.arange(n)])
    key = np.unique(r * n + c)
    r, c = key // n, key % n
    val = rng.random(len(key)) * 2 - 1
    dg = r == c
    val[dg] = 1.0 + np.bincount(r, weights=np.where(dg, 0.0, np.abs(val)), minlength=n)
    rp2 = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=rp2[1:])
    return rp2.astype(np.int32), c.astype(np.int32), val


def build(name, args):
    import sptrsv_bench as TB
    from sblas_amd import synth
    rng = np.random.default_rng(211)
    if name == "nd24k":
        n, (rp, ci, v) = synth.nd24k_like(args.nd24k_scale)
        label, low = "nd24k_like(%g), %d rows" % (args.nd24k_scale, n), TB.lower_of(n, rp, ci, v)
    elif name == "grid":
        n = args.grid_side ** 2
        label, low = "five-point grid %d^2" % args.grid_side, TB.grid_lower(args.grid_side, rng)
    elif name in ("bidiagonal", "banded5"):
        n = args.rows
        label, low = "%s made full, %d rows" % (name, n), TB.band_lower(n, 2 if name == "bidiagonal" else 5, rng)
    else:
        assert name == "powerlaw", name
        n = args.rows
        label, low = "powerlaw(%d) made full" % n, TB.lower_of(n, *synth.powerlaw(n, avg=3.0, max_len=5000))
    return (label, n) + full_sorted(n, low[0], low[1], rng)


def measure(name, args):
    import torch
    import sblas_amd as S
    import sptrsv_bench as TB
    dev = torch.device("cuda:0")
    label, n, rp, ci, val = build(name, args)
    drp, dci, dval = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (rp, ci, val))
    rec = dict(matrix=label, n=n, nnz=int(len(ci)), limits=S.ilu0_limits(), device=torch.cuda.get_device_name(0))
    plans = {}
    for mode in ("auto", "per_level"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plans[mode] = S.Ilu0Plan(n, drp, dci, mode=mode)
        rec["create_%s_ms" % mode] = (time.perf_counter() - t0) * 1e3
        rec["info_%s" % mode] = plans[mode].info()
    lu = {m: torch.empty_like(dval) for m in plans}
    once = {}
    for m in plans:                                                        # the first call of each, by the host clock
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plans[m].factor(dval, out=lu[m])
        torch.cuda.synchronize()
        once[m] = (time.perf_counter() - t0) * 1e3
    rec["first_call_ms"] = once
    rec["same_bits"] = bool(torch.equal(lu["auto"].view(torch.int64), lu["per_level"].view(torch.int64)))
    rec["finite"] = bool(torch.isfinite(lu["auto"]).all())
    slow = max(once.values()) > args.slow_ms                               # too long to repeat: the first calls stand
    if not slow:
        fns = {m: (lambda m=m: plans[m].factor(dval, out=lu[m])) for m in plans}
        lower = S.SptrsvPlan(n, drp, dci, lower=True, unit_diag=True)
        b = torch.from_numpy(np.random.default_rng(5).random(n) * 2 - 1).to(dev)
        x, y = torch.empty_like(b), torch.empty_like(b)
        spmv = S.SpmvPlan(n, n, drp, dci)
        fns["sptrsv_lower"] = lambda: lower.solve(lu["auto"], b, x=x)
        fns["spmv"] = lambda: spmv(dval, b, 1.0, 0.0, y)
        for k, (ms, each) in TB.timed(torch, fns, args.rounds).items():
            rec["%s_ms" % k], rec["%s_rounds" % k] = ms, each
        rec["sptrsv_lower_info"] = lower.info()
        rec["auto_over_per_level"] = rec["auto_ms"] / rec["per_level_ms"]
        rec["auto_over_sptrsv_lower"] = rec["auto_ms"] / rec["sptrsv_lower_ms"]
        rec["auto_us_per_level"] = 1e3 * rec["auto_ms"] / max(rec["info_auto"]["levels"], 1)
        lower.destroy(), spmv.destroy()
    for p in plans.values():
        p.destroy()
    if not slow and not args.no_sweep and rec["info_auto"]["widest_level"] > SWEEP[0]:
        ps = {cr: S.Ilu0Plan(n, drp, dci, chain_rows=cr) for cr in SWEEP}
        ps["per_level"] = S.Ilu0Plan(n, drp, dci, mode="per_level")
        out = torch.empty_like(dval)
        res = TB.timed(torch, {cr: (lambda cr=cr: ps[cr].factor(dval, out=out)) for cr in ps}, args.rounds, budget_ms=600.0)
        sw = {}
        for cr, p in ps.items():
            i = p.info()
            sw[str(cr)] = dict(ms=res[cr][0], rounds=res[cr][1], launches=i["launches"], wide=i["wide_launches"], chain=i["chain_launches"])
            p.destroy()
        rec["chain_rows_sweep"] = sw
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="nd24k,grid,bidiagonal,banded5,powerlaw")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--grid-side", type=int, default=1000)
    ap.add_argument("--nd24k-scale", type=float, default=1.0)
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--slow-ms", type=float, default=2000.0, help="a first call above this is not repeated")
    ap.add_argument("--limit", type=int, default=240, help="seconds a matrix may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help="(internal) measure this matrix in this process")
    args = ap.parse_args()
    if args.one:
        return measure(args.one, args)

    results, failed = [], None
    for name in args.inputs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", name, "--rounds", str(args.rounds), "--rows", str(args.rows),
               "--grid-side", str(args.grid_side), "--nd24k-scale", str(args.nd24k_scale), "--slow-ms", str(args.slow_ms)]
        cmd += ["--no-sweep"] if args.no_sweep else []
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
