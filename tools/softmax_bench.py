"""Row-wise softmax on a CSR pattern (sblas_hip_csr_softmax_f64_i32 and its backward) on one GPU, in one process.

Per input, alternating inside one run (two passes over the list, the second pass's figures stay):
  - the op: csr_softmax forward (out of place), and csr_softmax_backward;
  - the reference: the fastest torch route that runs on the input, forward and backward each:
      scatter   t = scale * x; m = scatter_reduce(amax); e = exp(t - m[row]); e / scatter_reduce(sum)[row]
      segment   the same with torch.segment_reduce over the row lengths
      sparse    torch.sparse.softmax(dim=1) on the COO tensor, and on the CSR tensor
    a route this torch build does not run is recorded as "unavailable: <error>"; one whose first call takes more than
    --slow-seconds is timed over a single call.  The scatter route is not called at all on an input whose longest row
    exceeds --scatter-max-row (default 100000) and is recorded as "left out: ...": scatter_reduce(amax) resolves a row
    with atomics on one address, and a single call on a row of 10^6 entries runs for minutes.  The backward of a route
    is torch.autograd.grad through its own forward graph, timed alone;
  - the yardstick: the library's planned SpMV on the same matrix (12 bytes a nonzero against the softmax's 16).
Every figure is the median over `--rounds` rounds of `--steps` calls between two device events, after a warm-up.
Algorithmic bytes: forward nnz * 16 + (rows + 1) * 4, backward nnz * 24 + (rows + 1) * 4.  One JSON object per input on
stdout; --out writes the list (rewritten after every input, so a run that is cut short leaves what it finished), with
power_law_over_banded added to a power-law record when a banded one is in the same run.  Kernel times come from a separate run under rocprofv3 --kernel-trace --stats (the
program after --, no counters in the same run; --no-torch keeps the trace to the library's kernels).

  python tools/softmax_bench.py [--inputs "nd24k;queen:300000;banded:1000000:5:2000;powerlaw:1000000:3:1000000"]
                                [--rounds 5] [--steps 3] [--scale 0.125] [--no-torch] [--routes scatter,segment,...]
                                [--scatter-max-row 100000] [--slow-seconds 1.0]
                                [--out profiles/r09_softmax.json]

Inputs as in tools/sddmm_bench.py: nd24k[:scale], queen:R, powerlaw:R:AVG:MAX, banded:R:NNZ_PER_ROW:HALF_BAND."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "s-blas_amd", "python"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

from sddmm_bench import make_pattern, timed  # noqa: E402

DEFAULT = "nd24k;queen:300000;banded:1000000:5:2000;powerlaw:1000000:3:1000000"
HBM_PEAK = 8.0e12


def torch_routes(torch, rows, cols, R, Cx, row_idx, lens, scale):
    """name -> function x -> softmax values (differentiable torch expressions)"""
    ninf = float("-inf")

    def scatter(x):
        t = x * scale
        m = torch.full((rows,), ninf, dtype=x.dtype, device=x.device).scatter_reduce(0, row_idx, t, "amax", include_self=True)
        e = torch.exp(t - m[row_idx])
        s = torch.zeros(rows, dtype=x.dtype, device=x.device).scatter_reduce(0, row_idx, e, "sum", include_self=True)
        return e / s[row_idx]

    def segment(x):
        t = x * scale
        m = torch.segment_reduce(t, "max", lengths=lens, unsafe=True)
        e = torch.exp(t - m[row_idx])
        return e / torch.segment_reduce(e, "sum", lengths=lens, unsafe=True)[row_idx]

    coo_idx = torch.stack([row_idx, Cx.long()])

    def sparse_coo(x):
        return torch.sparse.softmax(torch.sparse_coo_tensor(coo_idx, x * scale, (rows, cols), is_coalesced=True), dim=1).values()

    def sparse_csr(x):
        return torch.sparse.softmax(torch.sparse_csr_tensor(R.long(), Cx.long(), x * scale, (rows, cols)), dim=1).values()

    return dict(scatter=scatter, segment=segment, sparse_coo=sparse_coo, sparse_csr=sparse_csr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default=DEFAULT)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=0.125)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--routes", default="scatter,segment,sparse_coo,sparse_csr", help="the torch routes to try")
    ap.add_argument("--slow-seconds", type=float, default=1.0, help="a torch route whose first call takes longer is timed once")
    ap.add_argument("--scatter-max-row", type=int, default=100000,
                    help="the scatter route (atomics on one address per row) is left out where the longest row is longer")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import sblas_amd as S
    if not torch.cuda.is_available():
        raise SystemExit("softmax_bench needs a GPU")
    dev = torch.device("cuda:0")
    results = []
    for spec in args.inputs.split(";"):
        rows, cols, rp, ci = make_pattern(spec)
        nnz = len(ci)
        lens_h = np.diff(rp.astype(np.int64))
        R, Cx = torch.from_numpy(rp).to(dev), torch.from_numpy(ci).to(dev)
        lens = (R[1:] - R[:-1]).long()
        row_idx = torch.repeat_interleave(torch.arange(rows, device=dev), lens)
        g = torch.Generator(device=dev)
        g.manual_seed(211)
        x = (torch.rand(nnz, dtype=torch.float64, device=dev, generator=g) - 0.5) * 40.0
        dp = torch.rand(nnz, dtype=torch.float64, device=dev, generator=g) - 0.5
        xv = torch.rand(cols, dtype=torch.float64, device=dev, generator=g)
        out, dx, y = torch.empty_like(x), torch.empty_like(x), torch.empty(rows, dtype=torch.float64, device=dev)
        ws = torch.empty((S.csr_softmax_workspace_bytes(rows, nnz) + 7) // 8, dtype=torch.float64, device=dev)
        plan = S.SpmvPlan(rows, cols, R, Cx)
        r = lambda f: timed(torch, f, args.rounds, args.steps)
        rec = dict(input=spec, rows=rows, nnz=nnz, longest_row=int(lens_h.max()), mean_row=float(lens_h.mean()), scale=args.scale,
                   workspace_bytes=int(ws.numel() * 8))
        S.csr_softmax(R, x, out, args.scale, workspace=ws)
        S.csr_softmax_backward(R, out, dp, dx, args.scale, workspace=ws)
        torch.cuda.synchronize()
        print("%s: the op runs" % spec, file=sys.stderr, flush=True)
        routes = {} if args.no_torch else torch_routes(torch, rows, cols, R, Cx, row_idx, lens, args.scale)
        routes = {k: v for k, v in routes.items() if k in args.routes.split(",")}
        if "scatter" in routes and rec["longest_row"] > args.scatter_max_row:
            del routes["scatter"]                             # never called: one call runs for minutes on such a row
            rec["scatter_ms"] = rec["scatter_backward_ms"] = "left out: longest row %d > --scatter-max-row %d" % (
                rec["longest_row"], args.scatter_max_row)
            print("%s: route scatter left out" % spec, file=sys.stderr, flush=True)
        alive, slow = {}, set()
        for name, fn in routes.items():                       # which routes run at all, and how long one call takes
            try:
                t0 = time.perf_counter()
                xr = x.clone().requires_grad_()
                val = fn(xr)
                torch.autograd.grad(val, xr, dp, retain_graph=False)
                torch.cuda.synchronize()
                alive[name] = fn
                if time.perf_counter() - t0 > args.slow_seconds:  # e.g. atomics on a row of 10^6 entries: one round of one call
                    slow.add(name)
            except Exception as e:                            # not a dependency: record and go on
                rec[name + "_ms"] = rec[name + "_backward_ms"] = "unavailable: %s: %s" % (type(e).__name__, str(e)[:80])
            print("%s: route %s %s" % (spec, name, "slow" if name in slow else "runs" if name in alive else "unavailable"),
                  file=sys.stderr, flush=True)
        for _ in range(2):                                    # alternate, twice; the second pass's figures stay
            rec["softmax_ms"], rec["softmax_rounds"] = r(lambda: S.csr_softmax(R, x, out, args.scale, workspace=ws))
            rec["spmv_planned_ms"], rec["spmv_planned_rounds"] = r(lambda: plan(x, xv, 1.0, 0.0, y))
            rec["backward_ms"], rec["backward_rounds"] = r(lambda: S.csr_softmax_backward(R, out, dp, dx, args.scale, workspace=ws))
            for name, fn in alive.items():
                if name in slow and "rounds_of_" + name in rec:
                    continue                                  # a slow route is timed once
                rt = (lambda f: timed(torch, f, 1, 1)) if name in slow else r
                if name in slow:
                    rec["rounds_of_" + name] = 1
                with torch.no_grad():
                    rec[name + "_ms"], _ = rt(lambda: fn(x))
                xr = x.clone().requires_grad_()
                val = fn(xr)
                rec[name + "_backward_ms"], _ = rt(lambda: torch.autograd.grad(val, xr, dp, retain_graph=True))
                del val, xr
                print("%s: timed %s" % (spec, name), file=sys.stderr, flush=True)
        S.csr_softmax(R, x, out, args.scale, workspace=ws)
        S.csr_softmax_backward(R, out, dp, dx, args.scale, workspace=ws)
        fwd_bytes, bwd_bytes = nnz * 16 + (rows + 1) * 4, nnz * 24 + (rows + 1) * 4
        ms, bms = rec["softmax_ms"], rec["backward_ms"]
        rec.update(forward_bytes=fwd_bytes, backward_bytes=bwd_bytes, forward_TBps=fwd_bytes / ms / 1e9,
                   backward_TBps=bwd_bytes / bms / 1e9, forward_share_of_8TBps=fwd_bytes / (ms * 1e-3) / HBM_PEAK,
                   ns_per_nonzero=ms * 1e6 / nnz, over_spmv_planned=ms / rec["spmv_planned_ms"],
                   over_spmv_planned_against_16_over_12=ms / rec["spmv_planned_ms"] / (16.0 / 12.0))
        if alive:
            best_f = min(alive, key=lambda n: rec[n + "_ms"])
            best_b = min(alive, key=lambda n: rec[n + "_backward_ms"])
            rec.update(reference_forward=best_f, reference_forward_ms=rec[best_f + "_ms"],
                       reference_backward=best_b, reference_backward_ms=rec[best_b + "_backward_ms"],
                       reference_over_softmax=rec[best_f + "_ms"] / ms, reference_backward_over_backward=rec[best_b + "_backward_ms"] / bms)
            for name, fn in alive.items():                    # every route against the op, forward and backward
                xr = x.clone().requires_grad_()
                val = fn(xr)
                gref, = torch.autograd.grad(val, xr, dp)
                rec[name + "_max_abs_diff"] = float((out - val.detach()).abs().max())
                rec[name + "_backward_max_abs_diff"] = float((dx - gref).abs().max())
                del val, gref, xr
        results.append(rec)
        banded = [q for q in results if q["input"].startswith("banded")]
        for q in results:                                     # the long row against short rows, per nonzero
            if q["input"].startswith("powerlaw") and banded:
                bq = banded[-1]
                q["power_law_over_banded"] = dict(
                    banded=bq["input"], forward=q["softmax_ms"] / bq["softmax_ms"], backward=q["backward_ms"] / bq["backward_ms"],
                    forward_per_nonzero=q["softmax_ms"] / q["nnz"] / (bq["softmax_ms"] / bq["nnz"]),
                    backward_per_nonzero=q["backward_ms"] / q["nnz"] / (bq["backward_ms"] / bq["nnz"]))
        print(json.dumps(rec), flush=True)
        write_out(args.out, results)
        plan.destroy()
        del R, Cx, row_idx, lens, x, dp, out, dx, ws
        torch.cuda.empty_cache()


def write_out(path, results):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
