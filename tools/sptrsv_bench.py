"""Sparse triangular solves (SptrsvPlan: sblas_hip_sptrsv_plan_*) on one GPU, in one process.

Per matrix: levels and launches, time per solve under `auto` and `per_level` (device events around `steps` warm calls;
the median over `--rounds` rounds and every round are reported, the two modes alternating round by round), SpSM at 8 and
64 right-hand sides under `auto`, the planned SpMV on the same triangle in the same run (it reads the same bytes once:
the floor of any solve), and a host substitution (scipy.sparse.linalg.spsolve_triangular when scipy is there) for scale.
Then the chain_rows sweep on the matrices whose levels vary in width: the default is chosen from it.
One JSON object per matrix on stdout; --out writes the list.

  python tools/sptrsv_bench.py [--inputs nd24k,grid,bidiagonal,banded5,powerlaw] [--rounds 5] [--out profiles/r12_sptrsv.json]

Matrices (lower triangles; the diagonal is 1 + the row's absolute off-diagonal sum, so no solve overflows):
nd24k = nd24k_like(--nd24k-scale); grid = the five-point stencil on --grid-side squared; bidiagonal and banded5 = --rows
rows of 2 and of 5 consecutive columns; powerlaw = the strict lower part of powerlaw(--rows)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "s-blas_amd", "python"))

SWEEP = (16, 32, 64, 128, 256, 512, 1024, 2048, 4096)


def assemble_lower(n, r, c, w):
    """CSR of the strictly lower triplets (r, c, w), rows in the order given, plus a dominant diagonal stored last"""
    order = np.argsort(r, kind="stable")
    r, c, w = r[order], c[order], w[order]
    cnt = np.bincount(r, minlength=n)
    rp = np.zeros(n + 1, np.int64)
    np.cumsum(cnt + 1, out=rp[1:])
    start = np.concatenate([[0], np.cumsum(cnt)])[:-1]
    at = rp[:-1][r] + (np.arange(len(r)) - start[r])
    ci, val = np.empty(rp[-1], np.int32), np.empty(rp[-1], np.float64)
    ci[at], val[at] = c, w
    ci[rp[1:] - 1] = np.arange(n)
    val[rp[1:] - 1] = 1.0 + np.bincount(r, weights=np.abs(w), minlength=n)
    return rp.astype(np.int32), ci, val


def lower_of(n, rp, ci, v):
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp.astype(np.int64)))
    keep = ci < row
    return assemble_lower(n, row[keep], ci[keep].astype(np.int64), v[keep])


def band_lower(n, width, rng):
    """row i holds the columns i - width + 1 .. i"""
    r = np.concatenate([np.arange(k, n, dtype=np.int64) for k in range(1, width)]) if width > 1 else np.zeros(0, np.int64)
    c = np.concatenate([np.arange(0, n - k, dtype=np.int64) for k in range(1, width)]) if width > 1 else np.zeros(0, np.int64)
    return assemble_lower(n, r, c, rng.random(len(r)) * 2 - 1)


def grid_lower(side, rng):
    i = np.arange(side * side, dtype=np.int64)
    south, west = i[i >= side], i[i % side > 0]
    r, c = np.concatenate([south, west]), np.concatenate([south - side, west - 1])
    return assemble_lower(side * side, r, c, rng.random(len(r)) * 2 - 1)


def timed(torch, fns, rounds, budget_ms=1500.0, max_steps=20):
    """{name: (median ms, [rounds])}: the routes alternate inside every round; steps per round from a first timed call"""
    out, steps = {k: [] for k in fns}, {}
    for k, fn in fns.items():
        fn()                                                                # warm: code objects, caches
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        one = (time.perf_counter() - t0) * 1e3
        steps[k] = int(max(1, min(max_steps, budget_ms / rounds / max(one, 1e-3))))
    for _ in range(rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps[k]):
                fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) / steps[k])
    return {k: (float(np.median(v)), [round(x, 4) for x in v]) for k, v in out.items()}


def host_solve(n, rp, ci, val, b):
    try:
        import scipy.sparse as sp
        from scipy.sparse.linalg import spsolve_triangular
    except ImportError:
        return None, None
    A = sp.csr_matrix((val, ci, rp), shape=(n, n))
    A.sort_indices()
    t0 = time.perf_counter()
    x = spsolve_triangular(A, b, lower=True)
    return (time.perf_counter() - t0) * 1e3, x


def measure(S, torch, dev, name, n, rp, ci, val, rounds, sweep, max_per_level=200000):
    rng = np.random.default_rng(5)
    b = rng.random(n) * 2 - 1
    drp, dci, dval, db = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (rp, ci, val, b))
    rec = dict(matrix=name, n=n, nnz=int(len(ci)))
    plans = {}
    for mode in ("auto", "per_level"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plans[mode] = S.SptrsvPlan(n, drp, dci, mode=mode)
        rec["create_%s_ms" % mode] = (time.perf_counter() - t0) * 1e3
        rec["info_%s" % mode] = plans[mode].info()
    x = {m: torch.empty(n, dtype=torch.float64, device=dev) for m in plans}
    if rec["info_per_level"]["launches"] > max_per_level:                  # too many launches to repeat: one solve, host clock
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plans["per_level"].solve(dval, db, x=x["per_level"])
        torch.cuda.synchronize()
        rec["per_level_once_ms"] = (time.perf_counter() - t0) * 1e3
        once = x.pop("per_level")
        plans.pop("per_level").destroy()
    fns = {m: (lambda m=m: plans[m].solve(dval, db, x=x[m])) for m in plans}
    spmv, y = S.SpmvPlan(n, n, drp, dci), torch.zeros(n, dtype=torch.float64, device=dev)
    fns["spmv"] = lambda: spmv(dval, db, 1.0, 0.0, y)
    for k, (ms, each) in timed(torch, fns, rounds).items():
        rec["%s_ms" % k], rec["%s_rounds" % k] = ms, each
    for m in plans:
        rec["%s_over_spmv" % m] = rec["%s_ms" % m] / rec["spmv_ms"]
        rec["%s_us_per_level" % m] = 1e3 * rec["%s_ms" % m] / max(rec["info_auto"]["levels"], 1)
    if "per_level" in plans:
        rec["same_bits"] = bool(torch.equal(x["auto"].view(torch.int64), x["per_level"].view(torch.int64)))
        rec["auto_over_per_level"] = rec["auto_ms"] / rec["per_level_ms"]
    else:
        rec["same_bits"] = bool(torch.equal(x["auto"].view(torch.int64), once.view(torch.int64)))
        rec["auto_over_per_level"] = rec["auto_ms"] / rec["per_level_once_ms"]
    for nrhs in (8, 64):
        B = torch.from_numpy(rng.random((n, nrhs)) * 2 - 1).to(dev)
        X = torch.empty_like(B)
        ms, each = timed(torch, {"m": lambda: plans["auto"].solve(dval, B, x=X)}, max(2, rounds // 2), budget_ms=1000.0)["m"]
        rec["spsm%d_auto_ms" % nrhs], rec["spsm%d_auto_rounds" % nrhs] = ms, each
        del B, X
    hms, hx = host_solve(n, rp, ci, val, b)
    rec["host_scipy_ms"] = hms
    if hx is not None:
        rec["max_diff_vs_host"] = float(np.abs(x["auto"].cpu().numpy() - hx).max() / np.abs(hx).max())
    for p in plans.values():
        p.destroy()
    if sweep:
        sw = {}
        ps = {cr: S.SptrsvPlan(n, drp, dci, chain_rows=cr) for cr in SWEEP}
        ps["per_level"] = S.SptrsvPlan(n, drp, dci, mode="per_level")
        xs = torch.empty(n, dtype=torch.float64, device=dev)
        res = timed(torch, {cr: (lambda cr=cr: ps[cr].solve(dval, db, x=xs)) for cr in ps}, rounds, budget_ms=600.0)
        for cr, p in ps.items():
            i = p.info()
            sw[str(cr)] = dict(ms=res[cr][0], rounds=res[cr][1], launches=i["launches"], wide=i["wide_launches"], chain=i["chain_launches"])
            p.destroy()
        rec["chain_rows_sweep"] = sw
    spmv.destroy()
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="nd24k,grid,bidiagonal,banded5,powerlaw")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--grid-side", type=int, default=1000)
    ap.add_argument("--nd24k-scale", type=float, default=1.0)
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import sblas_amd as S
    from sblas_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("sptrsv_bench needs a GPU")
    dev = torch.device("cuda:0")
    results = [dict(limits=S.sptrsv_limits(), device=torch.cuda.get_device_name(0))]
    rng = np.random.default_rng(211)
    for name in args.inputs.split(","):
        sweep = not args.no_sweep
        if name == "nd24k":
            n, (rp, ci, v) = synth.nd24k_like(args.nd24k_scale)
            label, (rp, ci, v) = "nd24k_like(%g) lower, %d rows" % (args.nd24k_scale, n), lower_of(n, rp, ci, v)
        elif name == "grid":
            n = args.grid_side ** 2
            label, (rp, ci, v) = "five-point grid %d^2, lower" % args.grid_side, grid_lower(args.grid_side, rng)
        elif name in ("bidiagonal", "banded5"):
            n, width = args.rows, 2 if name == "bidiagonal" else 5
            label, (rp, ci, v), sweep = "%s, %d rows" % (name, n), band_lower(n, width, rng), False   # every level is one row
        else:
            assert name == "powerlaw", name
            n = args.rows
            label, (rp, ci, v) = "powerlaw(%d) strict lower + diagonal" % n, lower_of(n, *synth.powerlaw(n, avg=3.0, max_len=5000))
        results.append(measure(S, torch, dev, label, n, rp, ci, v, args.rounds, sweep))
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
