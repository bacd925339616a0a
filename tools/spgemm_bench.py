"""SpGEMM (SpgemmPlan: sblas_hip_spgemm_plan_*) on one GPU, in one process.

Per input: create (host clock around the call, which synchronises) and numeric (median over `--rounds` rounds of calls
between two device events, after a warm-up; the spread is reported) for the plan as the host rule makes it (AUTO) and
for the same product with general=True, alternated round by round so that both see the same machine.  Products per
second are the plan's own product count over the numeric time.  Beside them, for comparison only, torch.sparse.mm on
CSR tensors on the same GPU when this torch build has it (it sums in an order of its own: no bits are compared).
One JSON object per input on stdout; --out writes the list.

  python tools/spgemm_bench.py [--inputs banded5,queen,nd24k,powerlaw,galerkin] [--rounds 5] [--out profiles/r11_spgemm.json]

Inputs: banded5 = A * A, 10^6 banded rows of 5 (band +-500); queen = A * A of queen_like_grid(--queen-rows); nd24k = A * A
of nd24k_like(--nd24k-scale); powerlaw = A * A of the power-law matrix (10^6 rows of 3 on average), rows made ascending
by coo_to_csr(dup="sum"); galerkin = P^T (A P) as two products, A = banded5 and P piecewise constant over 4 rows."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "s-blas_amd", "python"))


def timed_pair(torch, fns, rounds, budget_ms=2000.0):
    """{name: (median ms, [rounds])}: the routes alternate inside every round; steps per round from a first timed call"""
    out = {k: [] for k in fns}
    steps = {}
    for k, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        one = (time.perf_counter() - t0) * 1e3
        steps[k] = int(max(1, min(20, budget_ms / rounds / max(one, 1e-3))))
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


def ascending(S, torch, dev, rows, cols, rp, ci, v):
    """the CSR with ascending, distinct rows (coo_to_csr sum), as device tensors"""
    lens = torch.from_numpy(np.diff(rp.astype(np.int64))).to(dev)
    row = torch.repeat_interleave(torch.arange(rows, dtype=torch.int32, device=dev), lens)
    col = torch.from_numpy(np.ascontiguousarray(ci, np.int32)).to(dev)
    val = torch.from_numpy(np.ascontiguousarray(v, np.float64)).to(dev)
    rowptr, colidx, out, _, _ = S.coo_to_csr(rows, cols, row, col, val, dup="sum")
    return rowptr, colidx.contiguous(), out.contiguous()


def measure(S, torch, dev, name, A, B, rounds, with_torch=True):
    """A = (m, k, rowptr, colidx, val), B likewise, device tensors -> (record, C as a tuple)"""
    m, k, rpa, cia, va = A
    _, n, rpb, cib, vb = B
    rec = dict(product=name, m=m, k=k, n=n, nnz_a=int(cia.numel()), nnz_b=int(cib.numel()))
    plans, outs = {}, {}
    for route, kw in (("auto", dict()), ("general", dict(general=True))):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plans[route] = S.SpgemmPlan(m, k, n, rpa, cia, rpb, cib, **kw)
        torch.cuda.synchronize()
        rec["create_%s_ms" % route] = (time.perf_counter() - t0) * 1e3
        rec["info_%s" % route] = plans[route].info()
        outs[route] = torch.empty(plans[route].nnz_c, dtype=torch.float64, device=dev)
    fns = {r: (lambda r=r: plans[r].multiply(va, vb, out=outs[r])) for r in plans}
    for route, (ms, each) in timed_pair(torch, fns, rounds).items():
        rec["numeric_%s_ms" % route], rec["numeric_%s_rounds" % route] = ms, each
        rec["numeric_%s_products_per_s" % route] = rec["info_auto"]["products"] / (ms * 1e-3) if ms > 0 else None
    rec["general_over_auto"] = rec["numeric_general_ms"] / rec["numeric_auto_ms"]
    rec["same_bits"] = bool(torch.equal(outs["auto"].view(torch.int64), outs["general"].view(torch.int64)))
    rpc, cic = plans["auto"].csr()
    C_ = (m, n, rpc.clone(), cic.clone(), outs["auto"].clone())
    if with_torch:
        try:
            ta = torch.sparse_csr_tensor(rpa.long(), cia.long(), va, size=(m, k))
            tb = torch.sparse_csr_tensor(rpb.long(), cib.long(), vb, size=(k, n))
            ms, each = timed_pair(torch, {"t": lambda: torch.sparse.mm(ta, tb)}, max(1, rounds // 2))["t"]
            rec["comparison_torch_sparse_mm_ms"], rec["comparison_torch_sparse_mm_rounds"] = ms, each
        except Exception as e:                                             # this build has no CSR x CSR product
            rec["comparison_torch_sparse_mm"] = "not supported: %s" % str(e).splitlines()[0][:160]
    for p in plans.values():
        p.destroy()
    print(json.dumps(rec), flush=True)
    return rec, C_


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="banded5,queen,nd24k,powerlaw,galerkin")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--queen-rows", type=int, default=100000)
    ap.add_argument("--nd24k-scale", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import sblas_amd as S
    from sblas_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("spgemm_bench needs a GPU")
    dev = torch.device("cuda:0")
    results = [dict(limits=S.spgemm_limits())]
    up = lambda rp, ci, v: tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (rp.astype(np.int32), ci.astype(np.int32), v))
    for name in args.inputs.split(","):
        if name in ("banded5", "galerkin"):
            rows = args.rows
            a = (rows, rows) + up(*synth.banded(rows, 5, 500))
            if name == "banded5":
                results.append(measure(S, torch, dev, "banded5: A * A", a, a, args.rounds)[0])
                continue
            coarse = (rows + 3) // 4                                       # P: row i holds one 1 in column i // 4
            p = (rows, coarse, torch.arange(rows + 1, dtype=torch.int32, device=dev),
                 (torch.arange(rows, dtype=torch.int32, device=dev) // 4).contiguous(), torch.ones(rows, dtype=torch.float64, device=dev))
            colptr, rowidx, valT, _ = S.csr_transpose(rows, coarse, p[2], p[3], p[4])
            pt = (coarse, rows, colptr, rowidx, valT)
            rec, ap_ = measure(S, torch, dev, "galerkin: A * P", a, p, args.rounds)
            results.append(rec)
            results.append(measure(S, torch, dev, "galerkin: P^T * (A P)", pt, ap_, args.rounds)[0])
        elif name == "queen":
            rp, ci, v = synth.queen_like_grid(args.queen_rows)
            rows = len(rp) - 1
            a = (rows, rows) + ascending(S, torch, dev, rows, rows, rp, ci, v)
            results.append(measure(S, torch, dev, "queen_like_grid(%d): A * A" % rows, a, a, args.rounds)[0])
        elif name == "nd24k":
            rows, (rp, ci, v) = synth.nd24k_like(args.nd24k_scale)
            a = (rows, rows) + up(rp, ci, v)
            results.append(measure(S, torch, dev, "nd24k_like(%g), %d rows: A * A" % (args.nd24k_scale, rows), a, a, args.rounds)[0])
        else:
            assert name == "powerlaw", name
            rows = args.rows
            rp, ci, v = synth.powerlaw(rows, avg=3.0, max_len=5000)
            a = (rows, rows) + ascending(S, torch, dev, rows, rows, rp, ci, v)
            results.append(measure(S, torch, dev, "powerlaw(%d): A * A" % rows, a, a, args.rounds)[0])
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
