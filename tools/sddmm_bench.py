"""SDDMM on a CSR pattern (sblas_hip_sddmm_csr_f64_i32) on one GPU, in one process.

Per input and k, alternating inside one run (two passes over the list, the second pass's figures stay):
  - SDDMM with (ROW, ROW) operands, beta = 0; once more with a column-major Y (its staging copy included) and with beta = 1;
  - the yardstick: the library's own direct SpMM kernel on the same matrix at n = k, pinned with SBLAS_SPMM_VARIANT=dpp,
    row-major B and C.  It pulls the same gathered operand bytes (nnz * k * 8) through L2 -> CU, so it is the nearest
    measured thing to a floor for a direct SDDMM.  The default SpMM (LDS-tiled where it applies) is printed beside it to
    size what a tiled SDDMM could buy;
  - what a user had before: (X[row] * Y[col]).sum(1) in torch (skipped above --torch-max bytes of temporaries), and
    torch.sparse.sampled_addmm as a cross-check of the values where this torch build runs it ("unavailable" otherwise).
Every figure is the median over `--rounds` rounds of `--steps` calls between two device events, after a warm-up.
Algorithmic bytes: nnz * (4 + 8) + (rows + 1) * 4 + (rows + cols) * k * 8 (+ nnz * 8 when beta != 0); gathered bytes:
nnz * k * 8.  One JSON object per (input, k) on stdout; --out writes the list.  Kernel times come from a separate run
under rocprofv3 --kernel-trace --stats (the program after --, no counters in the same run).

  python tools/sddmm_bench.py [--inputs "nd24k@1,8,16,32,64,128,256;queen:300000@64,256;..."] [--rounds 5] [--steps 3]
                              [--torch-max 40e9] [--no-torch] [--out profiles/r08_sddmm.json]

Inputs: nd24k[:scale] = nd24k_like, queen:R = queen_like_grid(R), powerlaw:R:AVG:MAX, banded:R:NNZ_PER_ROW:HALF_BAND."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "s-blas_amd", "python"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

DEFAULT = "nd24k@1,8,16,32,64,128,256;queen:300000@64,256;powerlaw:1000000:3:1000000@64;banded:1000000:5:2000@64"
HBM_PEAK = 8.0e12


def make_pattern(spec):
    from sblas_amd import synth
    kind, *a = spec.split(":")
    if kind == "nd24k":
        rows, (rp, ci, _) = synth.nd24k_like(float(a[0]) if a else 1.0)
    elif kind == "queen":
        rp, ci, _ = synth.queen_like_grid(int(a[0]))
    elif kind == "powerlaw":
        rp, ci, _ = synth.powerlaw(int(a[0]), avg=float(a[1]), max_len=int(a[2]))
    else:
        assert kind == "banded", spec
        rp, ci, _ = synth.banded(int(a[0]), int(a[1]), int(a[2]))
    rows = len(rp) - 1
    return rows, rows, np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)


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
    ap.add_argument("--inputs", default=DEFAULT)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--torch-max", type=float, default=40e9)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import sblas_amd as S
    if not torch.cuda.is_available():
        raise SystemExit("sddmm_bench needs a GPU")
    dev = torch.device("cuda:0")
    results = []

    def variant(name):
        if name:
            os.environ["SBLAS_SPMM_VARIANT"] = name
        else:
            os.environ.pop("SBLAS_SPMM_VARIANT", None)
        S.reload_env()

    for item in args.inputs.split(";"):
        spec, ks = item.split("@")
        rows, cols, rp, ci = make_pattern(spec)
        nnz = len(ci)
        R, Cx = torch.from_numpy(rp).to(dev), torch.from_numpy(ci).to(dev)
        A = (rows, cols, R, Cx)
        row_idx = torch.repeat_interleave(torch.arange(rows, device=dev), (R[1:] - R[:-1]).long())
        col_idx = Cx.long()
        lens = np.diff(rp.astype(np.int64))
        g = torch.Generator(device=dev)
        g.manual_seed(211)
        val = torch.rand(nnz, dtype=torch.float64, device=dev, generator=g)
        for k in (int(x) for x in ks.split(",")):
            r = lambda f: timed(torch, f, args.rounds, args.steps)
            rec = dict(input=spec, rows=rows, cols=cols, nnz=nnz, k=k, longest_row=int(lens.max()), mean_row=float(lens.mean()))
            X = torch.rand(rows, k, dtype=torch.float64, device=dev, generator=g) - 0.5
            Y = torch.rand(cols, k, dtype=torch.float64, device=dev, generator=g) - 0.5
            Yc = Y.t().contiguous().t()                     # the same values, column-major
            out = torch.empty(nnz, dtype=torch.float64, device=dev)
            out1 = torch.zeros(nnz, dtype=torch.float64, device=dev)
            ws = torch.empty((S.sddmm_workspace_bytes(rows, cols, nnz, k, S.ROW_MAJOR, S.COL_MAJOR) + 7) // 8, dtype=torch.float64,
                             device=dev)
            Cm = torch.empty(rows, k, dtype=torch.float64, device=dev)
            sws = torch.empty((S.spmm_workspace_bytes(rows, cols, nnz, k) + 7) // 8, dtype=torch.float64, device=dev)
            Asp = (rows, cols, R, Cx, val)
            temporaries = 2.0 * nnz * k * 8
            use_torch = not args.no_torch and temporaries <= args.torch_max
            for _ in range(2):                              # alternate, twice; the second pass's figures stay
                rec["sddmm_ms"], rec["sddmm_rounds"] = r(lambda: S.sddmm_tensor(A, X, Y, out, 1.0, 0.0))
                variant("dpp")
                rec["spmm_direct_dpp_ms"], rec["spmm_direct_dpp_rounds"] = r(lambda: S.spmm_tensor(Asp, Y, Cm, 1.0, 0.0, workspace=sws))
                variant(None)
                rec["spmm_default_ms"], _ = r(lambda: S.spmm_tensor(Asp, Y, Cm, 1.0, 0.0, workspace=sws))
                rec["sddmm_col_major_y_ms"], _ = r(lambda: S.sddmm_tensor(A, X, Yc, out, 1.0, 0.0, workspace=ws))
                rec["sddmm_beta1_ms"], _ = r(lambda: S.sddmm_tensor(A, X, Y, out1, 1.0, 1.0))
                if use_torch:
                    rec["torch_gather_ms"], _ = timed(torch, lambda: (X[row_idx] * Y[col_idx]).sum(1), max(1, args.rounds // 2), 1)
            S.sddmm_tensor(A, X, Y, out, 1.0, 0.0)
            alg = nnz * 12 + (rows + 1) * 4 + (rows + cols) * k * 8
            gathered = nnz * k * 8
            ms = rec["sddmm_ms"]
            rec.update(algorithmic_bytes=alg, gathered_bytes=gathered, algorithmic_TBps=alg / ms / 1e9,
                       share_of_8TBps=alg / (ms * 1e-3) / HBM_PEAK, gathered_TBps=gathered / ms / 1e9,
                       ns_per_nonzero=ms * 1e6 / nnz, over_spmm_direct_dpp=ms / rec["spmm_direct_dpp_ms"],
                       over_spmm_default=ms / rec["spmm_default_ms"],
                       beta1_algorithmic_TBps=(alg + 8 * nnz) / rec["sddmm_beta1_ms"] / 1e9)
            if use_torch:
                ref = (X[row_idx] * Y[col_idx]).sum(1)
                rec["torch_gather_over_sddmm"] = rec["torch_gather_ms"] / ms
                rec["max_abs_diff_vs_torch_gather"] = float((out - ref).abs().max())
                del ref
            else:
                rec["torch_gather_ms"] = "skipped: %.1f GB of temporaries" % (temporaries / 1e9)
            if not args.no_torch:
                try:
                    csr = torch.sparse_csr_tensor(R.long(), col_idx, torch.zeros(nnz, dtype=torch.float64, device=dev), (rows, cols))
                    Yt = Y.t()
                    got = torch.sparse.sampled_addmm(csr, X, Yt, beta=0.0)
                    rec["sampled_addmm_ms"], _ = timed(torch, lambda: torch.sparse.sampled_addmm(csr, X, Yt, beta=0.0),
                                                       max(1, args.rounds // 2), 1)
                    rec["max_abs_diff_vs_sampled_addmm"] = float((out - got.values()).abs().max())
                    del csr, got
                except Exception as e:                      # not a dependency: record and go on
                    rec["sampled_addmm_ms"] = "unavailable: %s" % type(e).__name__
            print(json.dumps(rec), flush=True)
            results.append(rec)
            del X, Y, Yc, out, out1, ws, Cm, sws
            torch.cuda.empty_cache()
        del R, Cx, row_idx, col_idx, val
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
