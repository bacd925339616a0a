"""Fused attention on a CSR pattern (CsrOperator.attention) against the composition it replaces,
op.matmul(op.softmax(op.sddmm(Q, K), scale), V), on one GPU, in one process and one run.

Per input and width d = dv, with Q, K, V requiring grad:
  - forward alone and forward + backward (torch.autograd.grad of all three inputs) of both routes, alternated round by
    round: every figure is the median over `--rounds` rounds of `--steps` calls between two device events, after a
    warm-up call of each; each round's figure is kept, and `spread` is (max - min) / median of a route's rounds.  A
    ratio fused / composition closer to 1 than the larger of the two spreads is a tie.  The composition's kernels are
    the parent's, so its figure in the same run is the yardstick;
  - the peak of torch.cuda.max_memory_allocated over one forward + backward of each route, above what was allocated
    before it (the operands, the operator's plans and workspaces after the warm-up);
  - max_abs_diff of O and of the three gradients between the routes.
One JSON object per (input, width) on stdout; --out writes the list, rewritten after every record.
Kernel times: `--trace DIR --out FILE` starts, for every input and width, a child
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/<tag> -- python tools/attention_bench.py
              --inputs <input> --widths <w> --rounds 1 --steps 1
(a run of its own per case, no counters alongside; this process never opens the GPU) and merges the kernel_stats.csv
summaries into FILE with an "Input" column (the tag), the library's kernels only.  `--collect-stats DIR --out FILE` only
merges summaries that are already there.

  python tools/attention_bench.py [--inputs "nd24k;queen:300000;banded:1000000:5:2000;powerlaw:1000000:3:1000000"]
                                  [--widths 64,16] [--rounds 5] [--steps 3] [--scale 0.125] [--out profiles/r10_attention.json]
  python tools/attention_bench.py --trace DIR --out profiles/r10_attention_kernel_stats.csv [--inputs ...] [--widths ...]

Inputs as in tools/sddmm_bench.py: nd24k[:scale], queen:R, powerlaw:R:AVG:MAX, banded:R:NNZ_PER_ROW:HALF_BAND."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "s-blas_amd", "python"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

from sddmm_bench import make_pattern  # noqa: E402

DEFAULT = "nd24k;queen:300000;banded:1000000:5:2000;powerlaw:1000000:3:1000000"


def alternated(torch, fns, rounds, steps):
    """{name: (median ms per call, the rounds)}: a warm-up call of each, then `rounds` rounds in which every function in
    turn runs `steps` calls between two device events"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) / steps)
    return {name: (float(np.median(v)), [round(x, 4) for x in v]) for name, v in out.items()}


def spread(rounds):
    return (max(rounds) - min(rounds)) / float(np.median(rounds))


def collect_stats(src, out):
    """DIR/<tag>/**/*kernel_stats.csv -> one csv, the rows of the library's own kernels under the tag of their run"""
    import csv
    import glob
    rows, header = [], None
    for tag in sorted(t for t in os.listdir(src) if os.path.isdir(os.path.join(src, t))):
        files = sorted(glob.glob(os.path.join(src, tag, "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)
        if not files:
            continue
        with open(files[-1], newline="") as f:
            r = csv.reader(f)
            header = next(r)
            rows += [[tag] + line for line in r if line and "sblas::" in line[0]]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w", newline="") as f:
        w = csv.writer(f, quoting=csv.QUOTE_ALL)
        w.writerow(["Input"] + (header or []))
        w.writerows(rows)


def trace(args):
    """one rocprofv3 kernel trace per (input, width), each a fresh child process, then the merged table"""
    import subprocess
    for spec in args.inputs.split(";"):
        for w in args.widths.split(","):
            tag = "%s_d%s" % (spec.replace(":", "_"), w)
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(args.trace, tag), "--",
                   sys.executable, os.path.abspath(__file__), "--inputs", spec, "--widths", w, "--rounds", "1", "--steps", "1",
                   "--scale", str(args.scale)]
            with open(os.path.join(args.trace, tag + ".log"), "w") as log:
                rc = subprocess.call(cmd, stdout=log, stderr=subprocess.STDOUT, timeout=args.trace_timeout)
            if rc != 0:                                       # nothing more is started on the GPU after a failure
                raise SystemExit("trace of %s failed with status %d: see %s.log" % (tag, rc, os.path.join(args.trace, tag)))
            print("traced %s" % tag, file=sys.stderr, flush=True)
    collect_stats(args.trace, args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default=DEFAULT)
    ap.add_argument("--widths", default="64,16")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=0.125)
    ap.add_argument("--out", default=None)
    ap.add_argument("--collect-stats", default=None, help="merge the rocprofv3 summaries under this folder into --out and exit")
    ap.add_argument("--trace", default=None, help="run every case under rocprofv3 --kernel-trace --stats into this folder, merge into --out")
    ap.add_argument("--trace-timeout", type=float, default=280.0, help="seconds a traced child may take")
    args = ap.parse_args()
    if args.collect_stats:
        return collect_stats(args.collect_stats, args.out)
    if args.trace:
        os.makedirs(args.trace, exist_ok=True)
        return trace(args)

    import torch
    from sblas_amd.autograd import CsrOperator
    if not torch.cuda.is_available():
        raise SystemExit("attention_bench needs a GPU")
    dev = torch.device("cuda:0")
    results = []
    for spec in args.inputs.split(";"):
        rows, cols, rp, ci = make_pattern(spec)
        nnz = len(ci)
        lens = np.diff(rp.astype(np.int64))
        R, Cx = torch.from_numpy(rp).to(dev), torch.from_numpy(ci).to(dev)
        for w in (int(x) for x in args.widths.split(",")):
            op = CsrOperator(rows, cols, R, Cx, n=w)
            g = torch.Generator(device=dev)
            g.manual_seed(211)
            rand = lambda r: (torch.rand(r, w, dtype=torch.float64, device=dev, generator=g) * 2 - 1)
            Q, K, V = (rand(r).requires_grad_() for r in (rows, cols, cols))
            dO = rand(rows)
            routes = dict(fused=lambda: op.attention(Q, K, V, args.scale),
                          composition=lambda: op.matmul(op.softmax(op.sddmm(Q, K), args.scale), V))
            both = lambda f: torch.autograd.grad(f(), (Q, K, V), dO)
            rec = dict(input=spec, rows=rows, nnz=nnz, longest_row=int(lens.max()), mean_row=float(lens.mean()), d=w, dv=w,
                       scale=args.scale, operand_bytes_each=rows * w * 8, score_bytes=nnz * 8)
            outs = {name: (f().detach(),) + both(f) for name, f in routes.items()}      # also the warm-up: plans, workspaces
            for i, what in enumerate(("O", "dQ", "dK", "dV")):
                rec["max_abs_diff_" + what] = float((outs["fused"][i] - outs["composition"][i]).abs().max())
            del outs
            for name, f in routes.items():
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                both(f)
                torch.cuda.synchronize()
                rec[name + "_peak_bytes"] = int(torch.cuda.max_memory_allocated() - base)
                kept = f()
                torch.cuda.synchronize()
                rec[name + "_kept_bytes"] = int(torch.cuda.memory_allocated() - base)   # what the graph holds until backward
                del kept
            fwd = alternated(torch, routes, args.rounds, args.steps)
            fb = alternated(torch, {name: (lambda f=f: both(f)) for name, f in routes.items()}, args.rounds, args.steps)
            for name in routes:
                rec[name + "_forward_ms"], rec[name + "_forward_rounds"] = fwd[name]
                rec[name + "_forward_backward_ms"], rec[name + "_forward_backward_rounds"] = fb[name]
            for what, t in (("forward", fwd), ("forward_backward", fb)):
                rec[what + "_fused_over_composition"] = t["fused"][0] / t["composition"][0]
                rec[what + "_spread"] = max(spread(t["fused"][1]), spread(t["composition"][1]))
                rec[what + "_tie"] = abs(rec[what + "_fused_over_composition"] - 1.0) < rec[what + "_spread"]
            rec["peak_composition_over_fused"] = rec["composition_peak_bytes"] / max(rec["fused_peak_bytes"], 1)
            results.append(rec)
            print(json.dumps(rec), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    json.dump(results, f, indent=1)
            op.destroy()
            del Q, K, V, dO, op
            torch.cuda.empty_cache()
        del R, Cx


if __name__ == "__main__":
    main()
