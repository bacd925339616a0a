"""Column-major against row-major dense operands (sblas_hip_spmm_csr_ordered) on one GPU, in one process.

For every (matrix, N, planned) case: the same A, B and C values in both layouts, warm-up and clock settling as bench.py
does, then `--rounds` rounds that alternate the (COL, COL) and the (ROW, ROW) call, each round `--steps` calls between
two device events; the median per-call time of each is reported with their ratio.  Every case also checks that the
row-major result is the transposed column-major one bit for bit.  One JSON object per case on stdout; --out writes the
list.  Kernel times (staging against stage 2) come from a separate rocprofv3 --kernel-trace --stats run of this script.

  python tools/order_bench.py [--rounds 7] [--steps 20] [--out profiles/r04_order.json]

Cases: nd24k_like at N = 8, 32, 64, 128, 256 and banded(1M, 5, 2000) at N = 64, each unplanned and planned.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "s-blas_amd", "python"), ROOT):
    sys.path.insert(0, p)


def timed(fn, steps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / steps  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--scale", type=float, default=1.0, help="row-count scale (rehearsals)")
    ap.add_argument("--widths", default="8,32,64,128,256")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    import sblas_amd as S
    from sblas_amd import synth
    from bench import settle
    if not torch.cuda.is_available():
        raise SystemExit("order_bench needs a GPU: there is no CPU path")
    dev = torch.device("cuda:0")
    rows, (rp, ci, v) = synth.nd24k_like(args.scale)
    cases = [("nd24k_like", rows, (rp, ci, v), int(n)) for n in args.widths.split(",")]
    br = max(1000, int(1_000_000 * args.scale))
    cases.append(("banded(1M, 5, 2000)", br, synth.banded(br, 5, 2000), 64))
    results = []
    mats = {}
    for name, m, (rp, ci, v), n in cases:
        if name not in mats:
            mats.clear()
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            mats[name] = (up(rp), up(ci), up(v))
        drp, dci, dv = mats[name]
        k = m
        rng = np.random.default_rng(n)
        Bl, Cl = rng.standard_normal((k, n)), rng.standard_normal((m, n))
        Bc = torch.from_numpy(np.ascontiguousarray(Bl.T).reshape(-1)).to(dev)
        Br = torch.from_numpy(np.ascontiguousarray(Bl).reshape(-1)).to(dev)
        Cc = torch.from_numpy(np.ascontiguousarray(Cl.T).reshape(-1)).to(dev)
        Cr = torch.from_numpy(np.ascontiguousarray(Cl).reshape(-1)).to(dev)
        ws = torch.empty(S.spmm_workspace_bytes(m, k, len(ci), n) // 8 + 1, dtype=torch.float64, device=dev)
        for planned in (False, True):
            plan = S.SpmmPlan(m, k, drp, dci, n) if planned else None

            def call(order):
                B, C, ldb, ldc = (Bc, Cc, k, m) if order == S.COL_MAJOR else (Br, Cr, n, n)
                if plan is None:
                    S.spmm_ordered(m, k, drp, dci, dv, B, ldb, order, n, 1.0, 0.0, C, ldc, order, ws)
                else:
                    plan.spmm_ordered(dv, B, ldb, order, n, 1.0, 0.0, C, ldc, order, ws)
            call(S.COL_MAJOR)
            call(S.ROW_MAJOR)
            torch.cuda.synchronize()
            same = Cr.view(m, n).cpu().numpy().tobytes() == Cc.view(n, m).t().contiguous().cpu().numpy().tobytes()
            settle(torch, lambda: (call(S.COL_MAJOR), call(S.ROW_MAJOR)))
            tc, tr = [], []
            for _ in range(args.rounds):
                tc.append(timed(lambda: call(S.COL_MAJOR), args.steps))
                tr.append(timed(lambda: call(S.ROW_MAJOR), args.steps))
            mc, mr = statistics.median(tc), statistics.median(tr)
            res = dict(matrix=name, rows=m, nnz=len(ci), n=n, planned=planned, col_major_us=round(mc, 2),
                       row_major_us=round(mr, 2), ratio=round(mr / mc, 4), col_spread_us=round(max(tc) - min(tc), 2),
                       row_spread_us=round(max(tr) - min(tr), 2), bit_identical=same)
            print(json.dumps(res), flush=True)
            results.append(res)
            if plan is not None:
                plan.destroy()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
