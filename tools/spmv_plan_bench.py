"""Planned against unplanned SpMV (sblas_hip_spmv_plan_*) on one GPU, in one process.

For every matrix: one plan, warm-up of both calls, then `--rounds` rounds that alternate the unplanned and the planned
call, each round `--steps` calls between two device events; the median per-call time of each is reported.  Both results
are checked against the CPU oracle (orc_spmv_csr).  One JSON object per matrix on stdout; --out writes the list.

  python tools/spmv_plan_bench.py [--only a,f,g] [--rounds 7] [--steps 20] [--out profiles/r04_spmv_plan.json]

(a) nd24k_like (bench matrix)  (b) banded(1M, 7, 2000)  (c) banded(600k, 48, 2000)  (d) queen_like(1M)
(e) powerlaw(1M, 3.2, max 5000)  (f) powerlaw(1M, 3.2, max 1M)  (g) 500k banded rows of 7, then 500k of 150 (+-2000)
(h) (g) interleaved every 300 rows.  (g) also times the unplanned call on its two halves separately.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "s-blas_amd", "python"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)


def matrices(scale):
    from sblas_amd import synth
    n = lambda k: max(1000, int(k * scale))
    return {
        "a": ("nd24k_like", lambda: synth.nd24k_like(scale)[1]),
        "b": ("banded(1M, 7, 2000)", lambda: synth.banded(n(1_000_000), 7, 2000)),
        "c": ("banded(600k, 48, 2000)", lambda: synth.banded(n(600_000), 48, 2000)),
        "d": ("queen_like(1M)", lambda: synth.queen_like(n(1_000_000))),
        "e": ("powerlaw(1M, 3.2, 5000)", lambda: synth.powerlaw(n(1_000_000), avg=3.2, max_len=5000)),
        "f": ("powerlaw(1M, 3.2, 1M)", lambda: synth.powerlaw(n(1_000_000), avg=3.2, max_len=1_000_000)),
        "g": ("500k rows of 7, then 500k of 150", lambda: synth.mixed_banded(n(1_000_000))),
        "h": ("rows of 7 and 150 interleaved every 300", lambda: synth.mixed_banded(n(1_000_000), interleave=300)),
    }


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
    ap.add_argument("--only", default="abcdefgh")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="row-count scale (rehearsals)")
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import sblas_amd as S
    import oracle_py as O
    if not torch.cuda.is_available():
        raise SystemExit("spmv_plan_bench needs a GPU")
    dev = torch.device("cuda:0")
    d = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
    results = []
    for key, (label, make) in matrices(a.scale).items():
        if key not in a.only.replace(",", ""):
            continue
        t0 = time.time()
        rp, ci, v = make()
        rows = len(rp) - 1
        cols = max(rows, int(ci.max()) + 1)
        R, Cx, V = d(rp), d(ci), d(v)
        rng = np.random.default_rng(5)
        xh = rng.random(cols)
        x = d(xh)
        y_un = torch.zeros(rows, dtype=torch.float64, device=dev)
        y_pl = torch.zeros(rows, dtype=torch.float64, device=dev)
        t1 = time.time()
        plan = S.SpmvPlan(rows, cols, R, Cx)
        torch.cuda.synchronize()
        plan_ms = (time.time() - t1) * 1000.0
        un = lambda: S.spmv(rows, cols, R, Cx, V, x, 1.0, 0.0, y_un)
        pl = lambda: plan(V, x, 1.0, 0.0, y_pl)
        for _ in range(a.warmup):
            un()
            pl()
        torch.cuda.synchronize()
        t_un, t_pl = [], []
        for _ in range(a.rounds):
            t_un.append(timed(un, a.steps))
            t_pl.append(timed(pl, a.steps))
        rec = dict(matrix=key, label=label, rows=rows, nnz=int(len(ci)), plan=plan.info(),
                   unplanned_us=float(np.median(t_un)), planned_us=float(np.median(t_pl)),
                   unplanned_spread_us=[float(min(t_un)), float(max(t_un))], planned_spread_us=[float(min(t_pl)), float(max(t_pl))],
                   plan_create_ms=plan_ms)
        rec["planned_over_unplanned"] = rec["planned_us"] / rec["unplanned_us"]
        if key == "g":
            # what a user gets by splitting the matrix by hand: the unplanned call on each half
            half = rows // 2
            rp1 = rp[:half + 1]
            rp2 = (rp[half:] - rp[half]).astype(np.int32)
            R1, R2 = d(rp1), d(rp2)
            C1, C2 = Cx[:int(rp[half])], Cx[int(rp[half]):]
            V1, V2 = V[:int(rp[half])], V[int(rp[half]):]
            h1 = lambda: S.spmv(half, cols, R1, C1, V1, x, 1.0, 0.0, y_un)
            h2 = lambda: S.spmv(rows - half, cols, R2, C2, V2, x, 1.0, 0.0, y_un, y_offset=half)
            for _ in range(a.warmup):
                h1()
                h2()
            t1s, t2s = [], []
            for _ in range(a.rounds):
                t1s.append(timed(h1, a.steps))
                t2s.append(timed(h2, a.steps))
            rec["halves_unplanned_us"] = [float(np.median(t1s)), float(np.median(t2s))]
            rec["planned_over_halves"] = rec["planned_us"] / sum(rec["halves_unplanned_us"])
        if not a.no_check:
            un()
            pl()
            torch.cuda.synchronize()
            ref = O.spmv(rows, rp, ci, v, xh, np.zeros(rows), 1.0, 0.0)
            scale = max(np.abs(ref).max(), 1e-300)
            rec["unplanned_rel_err"] = float(np.abs(y_un.cpu().numpy() - ref).max() / scale)
            rec["planned_rel_err"] = float(np.abs(y_pl.cpu().numpy() - ref).max() / scale)
            rec["planned_equals_unplanned"] = bool(torch.equal(y_un, y_pl))
        rec["wall_s"] = time.time() - t0
        print(json.dumps(rec), flush=True)
        results.append(rec)
        plan.destroy()
        del R, Cx, V, x, y_un, y_pl
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
