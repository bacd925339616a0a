"""Plain SpMM plan against split SpMM plan (sblas_hip_spmm_plan_create_split) on one GPU, in one process.

For every case (matrix, N, split parameters): both plans, warm-up of both, then `--rounds` rounds that alternate the
plain and the split planned call, each round `--steps` calls between two device events; the median per-call time of
each is reported.  Both results are checked against the CPU oracle (orc_spmm_csr) on the first case of every matrix
and N, and every row the split plan does not split is compared bit for bit with the plain plan.  One JSON object per
case on stdout; --out writes the list.

  python tools/spmm_split_bench.py [--cases powerlaw:1000000:40:1000000@128,...] [--sweep 8192:2048,16384:4096]
                                   [--rounds 7] [--steps 10] [--out profiles/r05_spmm_split.json]

A case is <matrix>@<N>; matrices: powerlaw:ROWS:AVG:MAXLEN (synth.powerlaw), bench (synth.nd24k_like, the bench
matrix).  --sweep lists split_min:piece pairs (0:0 = the library's defaults).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "s-blas_amd", "python"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

DEFAULT_CASES = ("powerlaw:1000000:40:1000000@128,powerlaw:1000000:40:1000000@256,powerlaw:300000:40:300000@64,"
                 "powerlaw:1000000:40:100000@128,powerlaw:1000000:40:12000@128,bench@64")


def make_matrix(spec):
    from sblas_amd import synth
    if spec == "bench":
        rows, (rp, ci, v) = synth.nd24k_like(1.0)
        return rows, rows, rp, ci, v
    kind, rows, avg, max_len = spec.split(":")
    assert kind == "powerlaw", spec
    rp, ci, v = synth.powerlaw(int(rows), avg=float(avg), max_len=int(max_len))
    return int(rows), int(rows), rp, ci, v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=DEFAULT_CASES)
    ap.add_argument("--sweep", default="0:0", help="split_min:piece pairs, comma-separated")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import sblas_amd as S
    import oracle_py as O
    if not torch.cuda.is_available():
        raise SystemExit("spmm_split_bench needs a GPU")
    dev = torch.device("cuda:0")
    sweep = [tuple(int(x) for x in p.split(":")) for p in args.sweep.split(",")]
    results, cache = [], {}
    for case in args.cases.split(","):
        spec, n = case.split("@")
        n = int(n)
        if spec not in cache:
            cache.clear()
            cache[spec] = make_matrix(spec)
        rows, cols, rp, ci, v = cache[spec]
        nnz = len(ci)
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        R, Cx, V = d(rp), d(ci), d(v)
        rng = np.random.default_rng(11)
        Bh = rng.random(cols * n) * 2 - 1
        B = d(Bh)
        ws = torch.empty(S.spmm_workspace_bytes(rows, cols, nnz, n) // 8 + 1, dtype=torch.float64, device=dev)
        plain = S.SpmmPlan(rows, cols, R, Cx, n)
        Cp = torch.zeros(rows * n, dtype=torch.float64, device=dev)
        plain.spmm(V, B, cols, n, 1.0, 0.0, Cp, rows, ws)
        torch.cuda.synchronize()
        ref = None
        lens = np.diff(rp.astype(np.int64))
        for k, (smin, piece) in enumerate(sweep):
            split = S.SpmmPlan(rows, cols, R, Cx, n, split=True, split_min=smin, piece=piece)
            info = split.split_info()
            Cs = torch.zeros(rows * n, dtype=torch.float64, device=dev)
            split.spmm(V, B, cols, n, 1.0, 0.0, Cs, rows, ws)
            torch.cuda.synchronize()
            gp, gs = Cp.cpu().numpy().reshape(n, rows), Cs.cpu().numpy().reshape(n, rows)
            pieces, srows = S.spmm_split_classify(rp, split_min=smin, piece=piece)
            is_split = np.zeros(rows, bool)
            is_split[srows[:, 0]] = info["split_rows"] > 0
            unsplit_identical = bool(np.array_equal(gp[:, ~is_split], gs[:, ~is_split]))
            err = None
            if k == 0:
                ref = O.spmm_omp(rows, cols, n, rp, ci, v, Bh, np.zeros(rows * n), 1.0, 0.0).reshape(n, rows)
            scale = max(float(np.abs(ref).max()), 1e-300)
            err = dict(plain=float(np.abs(gp - ref).max() / scale), split=float(np.abs(gs - ref).max() / scale))

            def timed(plan, Cm):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    plan.spmm(V, B, cols, n, 1.0, 0.0, Cm, rows, ws)
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / args.steps

            for _ in range(2):
                timed(plain, Cp), timed(split, Cs)
            tp, ts = [], []
            for _ in range(args.rounds):
                tp.append(timed(plain, Cp))
                ts.append(timed(split, Cs))
            r = dict(matrix=spec, n=n, rows=rows, nnz=nnz, max_row=int(lens.max()), split_min=smin or S.SPMM_SPLIT_MIN,
                     piece=piece or S.SPMM_SPLIT_PIECE, split_info=info, plan_info=split.info(),
                     plain_ms=float(np.median(tp)), split_ms=float(np.median(ts)), plain_ms_all=tp, split_ms_all=ts,
                     speedup=float(np.median(tp) / np.median(ts)), rel_err=err, unsplit_rows_identical=unsplit_identical)
            print(json.dumps(r), flush=True)
            results.append(r)
            split.destroy()
        plain.destroy()
        del R, Cx, V, B, ws, Cp
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
