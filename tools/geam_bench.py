"""GEAM (GeamPlan: sblas_hip_geam_plan_*) on one GPU: C = alpha * A + beta * B with new values every call.

Per pair: create on the host clock (the call synchronises), numeric per call (median over `--rounds` rounds of calls
between two device events after a warm-up, every round reported), and the bytes the plan holds, for four routes that
alternate inside every round so that all see the same machine:
  sorted     the plan as create makes it for ascending operands (one launch over C's entries);
  scatter    the sorted path with the two-launch ordered-scatter numeric (scatter=True): A's terms through dest_a, then
             B's through dest_b with a match flag; 8 B less held per entry of C;
  general    the same plan with general=True (yardstick 2: scale, then the owned COO plan's assemble);
  coo        what a user could do before (yardstick 1): a CooPlan(dup="sum") over A's triplets followed by B's, and per
             call torch.cat((alpha * va, beta * vb)) and assemble.
All four must give the same bits; the record says so.  numeric's achieved rate is stated on the algorithmic bytes of
the sorted path, 24 B read + 8 B written per entry of C, to be held against the 8 TB/s roofline and the planned SpMV's
5.4 TB/s on the same chip.

Every pair is measured in a child process of its own under its own time limit, one at a time, the four routes inside
that one process, and nothing is started after a child that failed or ran out of time.  One JSON object per pair on
stdout; --out writes the list.

  python tools/geam_bench.py [--inputs nd24k,grid,banded5,powerlaw] [--rounds 5] [--out profiles/r28_geam.json]

Pairs, on tools/ilu0_bench.py's matrices: nd24k = nd24k_like made full + its transpose (TransposePlan.csc()); grid = the
five-point 1000^2 grid + the identity; banded5 = the nine-diagonal band + the same band shifted by two columns;
powerlaw = the power-law matrix made full + its transpose (rows of up to 5000 entries)."""
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

ALPHA, BETA = 1.0, 0.125
ROOFLINE_TBS, SPMV_TBS = 8.0, 5.4


def shifted(n, rp, ci, val, by):
    """the same entries `by` columns to the right; what leaves the matrix is dropped"""
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp.astype(np.int64)))
    keep = ci.astype(np.int64) + by < n
    rp2 = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(row[keep], minlength=n), out=rp2[1:])
    return rp2.astype(np.int32), (ci[keep] + by).astype(np.int32), val[keep]


def measure(name, args):
    import torch
    import ilu0_bench as IB
    import sblas_amd as S
    from spgemm_bench import timed_pair
    dev = torch.device("cuda:0")
    up = lambda *arrays: tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)
    label, n, rp, ci, val = IB.build(name, args)
    rpa, cia, va = up(rp, ci, val)
    keep = []                                                               # plans whose arrays B views
    if name in ("nd24k", "powerlaw"):
        t = S.TransposePlan(n, n, rpa, cia, va)
        rpb, cib, vb = t.csc()
        keep.append(t)
        label += " + its transpose"
    elif name == "grid":
        rpb = torch.arange(n + 1, dtype=torch.int32, device=dev)
        cib, vb = rpb[:n].contiguous(), torch.ones(n, dtype=torch.float64, device=dev)
        label += " + the identity"
    else:
        rpb, cib, vb = up(*shifted(n, rp, ci, val, 2))
        label += " + the same band two columns to the right"
    rec = dict(pair=label, n=n, nnz_a=int(cia.numel()), nnz_b=int(cib.numel()), alpha=ALPHA, beta=BETA, device=torch.cuda.get_device_name(0))

    def clocked(make):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p = make()
        torch.cuda.synchronize()
        return p, (time.perf_counter() - t0) * 1e3

    plans = {}
    plans["sorted"], rec["create_sorted_ms"] = clocked(lambda: S.GeamPlan(n, n, rpa, cia, rpb, cib))
    plans["scatter"], rec["create_scatter_ms"] = clocked(lambda: S.GeamPlan(n, n, rpa, cia, rpb, cib, scatter=True))
    plans["general"], rec["create_general_ms"] = clocked(lambda: S.GeamPlan(n, n, rpa, cia, rpb, cib, general=True))

    def make_coo():
        lens = lambda r: (r[1:] - r[:-1]).long()
        rows = torch.arange(n, dtype=torch.int32, device=dev)
        row = torch.cat((torch.repeat_interleave(rows, lens(rpa)), torch.repeat_interleave(rows, lens(rpb))))
        return S.CooPlan(n, n, row, torch.cat((cia, cib)), dup="sum")
    coo, rec["create_coo_ms"] = clocked(make_coo)                           # the triplet expansion is part of this route
    for route in ("sorted", "scatter", "general"):
        rec["info_%s" % route] = plans[route].info()
    rec["info_coo"] = coo.info()
    assert rec["info_sorted"]["path"] == "sorted" and rec["info_general"]["path"] == "general"
    nnz_c = plans["sorted"].nnz_c
    rec["nnz_c"], rec["matched"] = nnz_c, rec["info_sorted"]["matched"]
    rec["bytes_held"] = dict(sorted=rec["info_sorted"]["bytes"], scatter=rec["info_scatter"]["bytes"], general=rec["info_general"]["bytes"], coo=rec["info_coo"]["bytes"])
    outs = {r: torch.empty(nnz_c, dtype=torch.float64, device=dev) for r in ("sorted", "scatter", "general", "coo")}
    fns = {r: (lambda r=r: plans[r].add(va, vb, ALPHA, BETA, out=outs[r])) for r in plans}
    fns["coo"] = lambda: coo.assemble(torch.cat((ALPHA * va, BETA * vb)), out=outs["coo"])
    for route, (ms, each) in timed_pair(torch, fns, args.rounds).items():
        rec["numeric_%s_ms" % route], rec["numeric_%s_rounds" % route] = ms, each
    torch.cuda.synchronize()
    i64 = lambda t: t.view(torch.int64)
    rec["same_bits"] = all(bool(torch.equal(i64(outs["sorted"]), i64(outs[r]))) for r in ("scatter", "general", "coo"))
    rec["same_structure"] = all(bool(torch.equal(x, y)) for x, y in zip(plans["sorted"].csr(), coo.csr()[:2]))
    rec["algorithmic_bytes"] = 32 * nnz_c
    rec["sorted_tb_per_s"] = rec["algorithmic_bytes"] / (rec["numeric_sorted_ms"] * 1e-3) / 1e12
    rec["sorted_over_roofline"] = rec["sorted_tb_per_s"] / ROOFLINE_TBS
    rec["sorted_over_spmv_rate"] = rec["sorted_tb_per_s"] / SPMV_TBS
    rec["coo_over_sorted"] = rec["numeric_coo_ms"] / rec["numeric_sorted_ms"]
    rec["general_over_sorted"] = rec["numeric_general_ms"] / rec["numeric_sorted_ms"]
    rec["scatter_over_sorted"] = rec["numeric_scatter_ms"] / rec["numeric_sorted_ms"]
    for p in list(plans.values()) + [coo] + keep:
        p.destroy()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="nd24k,grid,banded5,powerlaw")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--grid-side", type=int, default=1000)
    ap.add_argument("--nd24k-scale", type=float, default=1.0)
    ap.add_argument("--limit", type=int, default=240, help="seconds a pair may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help="(internal) measure this pair in this process")
    args = ap.parse_args()
    if args.one:
        return measure(args.one, args)

    results, failed = [], None
    for name in args.inputs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", name, "--rounds", str(args.rounds), "--rows", str(args.rows),
               "--grid-side", str(args.grid_side), "--nd24k-scale", str(args.nd24k_scale)]
        try:
            run = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.limit)
        except subprocess.TimeoutExpired:
            failed = dict(pair=name, failed="no result within %d s" % args.limit)
        else:
            lines = [l for l in run.stdout.decode().splitlines() if l.startswith("{")]
            if run.returncode != 0 or not lines:
                failed = dict(pair=name, failed="exit status %d" % run.returncode)
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
