"""Transposed products (sblas_hip_transpose_plan_*) against the products as stored, on one GPU, in one process.

Per matrix: the plan's creation time (host clock around create, which synchronises), the transpose alone
(sblas_hip_csr_transpose_f64_i32 between two device events), update_values, A^T x against A x (SpmvPlan on A) and
A^T B against A B (SpmmPlan on A; a TransposePlan of the same width) at each N.  Every timed figure is the median over
`--rounds` rounds of `--steps` calls between two device events, after a warm-up.  One JSON object per matrix on stdout;
--out writes the list.  Kernel times come from a separate run under rocprofv3 --kernel-trace --stats (--rounds 1).

  python tools/transpose_bench.py [--matrices nd24k,queen:1000000,powerlaw:1000000:40:1000000,powerlaw_t:...]
                                  [--ns 64,256] [--rounds 7] [--steps 10] [--out profiles/r06_transpose.json]
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

DEFAULT = "nd24k,queen:1000000,powerlaw:1000000:40:1000000,powerlaw_t:1000000:40:1000000"


def make_matrix(spec):
    """(rows, cols, rowptr, colidx, val); powerlaw_t is the host transpose of the powerlaw matrix (a 10^6-entry column)"""
    from sblas_amd import synth
    kind, *a = spec.split(":")
    if kind == "nd24k":
        rows, (rp, ci, v) = synth.nd24k_like(1.0)
        return rows, rows, rp, ci, v
    if kind == "queen":
        rp, ci, v = synth.queen_like_grid(int(a[0]))
        return len(rp) - 1, len(rp) - 1, rp, ci, v
    rows = int(a[0])
    rp, ci, v = synth.powerlaw(rows, avg=float(a[1]), max_len=int(a[2]))
    if kind == "powerlaw":
        return rows, rows, rp, ci, v
    assert kind == "powerlaw_t", spec
    perm = np.argsort(ci, kind="stable")
    row_of = np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp))
    cp = np.zeros(rows + 1, np.int64)
    np.cumsum(np.bincount(ci, minlength=rows), out=cp[1:])
    return rows, rows, cp.astype(np.int32), row_of[perm], v[perm]


def timed(torch, fn, rounds, steps):
    """median ms per call over rounds of `steps` calls between two device events"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / steps)
    return float(np.median(out)), [round(x, 4) for x in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default=DEFAULT)
    ap.add_argument("--ns", default="64,256")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import sblas_amd as S
    if not torch.cuda.is_available():
        raise SystemExit("transpose_bench needs a GPU")
    dev = torch.device("cuda:0")
    results = []
    for spec in args.matrices.split(","):
        rows, cols, rp, ci, v = make_matrix(spec)
        nnz = len(ci)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        rp_d, ci_d, v_d = up(rp), up(ci), up(v)
        rec = dict(matrix=spec, rows=rows, cols=cols, nnz=nnz, max_row=int(np.diff(rp).max()),
                   max_col=int(np.bincount(ci, minlength=cols).max()), passes=(max(cols - 1, 0).bit_length() + 7) // 8)
        r = lambda f: timed(torch, f, args.rounds, args.steps)
        # the transpose alone, into preallocated outputs
        colptr = torch.empty(cols + 1, dtype=torch.int32, device=dev)
        rowidx = torch.empty(nnz, dtype=torch.int32, device=dev)
        valT = torch.empty(nnz, dtype=torch.float64, device=dev)
        perm = torch.empty(nnz, dtype=torch.int32, device=dev)
        wsb = S.transpose_workspace_bytes(rows, cols, nnz)
        tws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
        L = S.lib()
        st = S._stream()

        def transpose():
            S.check(L.sblas_hip_csr_transpose_f64_i32(-1, st, rows, cols, nnz, rp_d.data_ptr(), ci_d.data_ptr(), v_d.data_ptr(),
                                                      colptr.data_ptr(), rowidx.data_ptr(), valT.data_ptr(), perm.data_ptr(),
                                                      tws.data_ptr(), wsb), "transpose")
        rec["transpose_ms"], rec["transpose_rounds"] = r(transpose)
        rec["transpose_workspace_bytes"] = wsb
        del tws, colptr, rowidx, valT, perm
        # plans: creation (synchronises) on the host clock
        for split in (False, True) if spec.startswith("powerlaw_t") else (False,):
            tag = "split_" if split else ""
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tp = S.TransposePlan(rows, cols, rp_d, ci_d, v_d, n=int(args.ns.split(",")[0]), split=split)
            rec[tag + "plan_create_ms"] = (time.perf_counter() - t0) * 1e3
            rec[tag + "plan_info"] = tp.info()
            tp.destroy()
        tp = S.TransposePlan(rows, cols, rp_d, ci_d, v_d)
        rec["update_values_ms"], _ = r(lambda: tp.update_values(v_d))
        x = torch.rand(rows, dtype=torch.float64, device=dev)
        y = torch.zeros(cols, dtype=torch.float64, device=dev)
        xa = torch.rand(cols, dtype=torch.float64, device=dev)
        ya = torch.zeros(rows, dtype=torch.float64, device=dev)
        ap_ = S.SpmvPlan(rows, cols, rp_d, ci_d)
        for _ in range(2):       # alternate the two, twice
            rec["spmv_t_ms"], rec["spmv_t_rounds"] = r(lambda: tp.spmv(x, 1.0, 0.0, y))
            rec["spmv_ms"], rec["spmv_rounds"] = r(lambda: ap_(v_d, xa, 1.0, 0.0, ya))
        rec["spmv_t_over_spmv"] = rec["spmv_t_ms"] / rec["spmv_ms"]
        tp.destroy()
        ap_.destroy()
        del x, y, xa, ya
        for N in (int(n) for n in args.ns.split(",")):
            splits = (False, True) if spec.startswith("powerlaw_t") else (False,)
            for split in splits:
                tag = "spmm%d%s" % (N, "_split" if split else "")
                tp = S.TransposePlan(rows, cols, rp_d, ci_d, v_d, n=N, split=split)
                ap_ = S.SpmmPlan(rows, cols, rp_d, ci_d, N, split=split)
                ws = torch.empty(max(S.spmm_workspace_bytes(cols, rows, nnz, N), S.spmm_workspace_bytes(rows, cols, nnz, N)) // 8 + 1,
                                 dtype=torch.float64, device=dev)
                B = torch.rand(rows * N, dtype=torch.float64, device=dev)
                Cm = torch.zeros(cols * N, dtype=torch.float64, device=dev)
                Ba = torch.rand(cols * N, dtype=torch.float64, device=dev)
                Ca = torch.zeros(rows * N, dtype=torch.float64, device=dev)
                for _ in range(2):
                    rec[tag + "_t_ms"], _r = r(lambda: tp.spmm_ordered(B, rows, S.COL_MAJOR, N, 1.0, 0.0, Cm, cols, S.COL_MAJOR, ws))
                    rec[tag + "_ms"], _r = r(lambda: ap_.spmm_ordered(v_d, Ba, cols, S.COL_MAJOR, N, 1.0, 0.0, Ca, rows, S.COL_MAJOR, ws))
                rec[tag + "_t_over_ab"] = rec[tag + "_t_ms"] / rec[tag + "_ms"]
                tp.destroy()
                ap_.destroy()
                del ws, B, Cm, Ba, Ca
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del rp_d, ci_d, v_d
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
