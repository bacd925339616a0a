"""CSR from COO triplets (sblas_hip_coo_to_csr_f64_i32, sblas_hip_coo_plan_*) on one GPU, in one process.

Per input and duplicate mode: the one-shot conversion into preallocated outputs, the plan's creation (host clock around
create, which synchronises) and assemble.  Beside them, for scale: the existing transpose of the same matrix
(sblas_hip_csr_transpose_f64_i32 on the converted KEEP CSR, alternated with the conversion), TransposePlan.update_values
(the same gather as a KEEP assemble, alternated with it, as is a KEEP assemble of the same triplets given in CSR order),
torch's own coalesce() on the device and the host route a user
had before (D2H, numpy.lexsort + a left-to-right sum per run, H2D; host clock, one run, inputs up to --host-max
triplets).  Every device figure is the median over `--rounds` rounds of `--steps` calls between two device events, after
a warm-up.  Byte counts are the algorithm's own, rates are those bytes over the measured time.
One JSON object per input on stdout; --out writes the list.  Kernel times come from a separate run under
rocprofv3 --kernel-trace --stats (--rounds 1 --steps 1 --no-host).

  python tools/coo_bench.py [--inputs nd24k,queen:1000000:8,powerlaw:1000000:3:1000000] [--rounds 5] [--steps 3]
                            [--host-max 50000000] [--no-host] [--out profiles/r07_coo.json]

Inputs: nd24k = nd24k_like shuffled (no duplicates); queen:R:K = queen_like_grid(R) with every entry split into 1..K
triplets, shuffled; powerlaw:R:AVG:MAX = the power-law matrix shuffled.  The splitting and the shuffle run on the device
(torch.randperm, fixed seed)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "s-blas_amd", "python"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

DEFAULT = "nd24k,queen:1000000:8,powerlaw:1000000:3:1000000"
HBM_PEAK = 8.0e12


def make_triplets(torch, dev, spec):
    """(rows, cols, row, col, val) device tensors, shuffled"""
    from sblas_amd import synth
    kind, *a = spec.split(":")
    split = 1
    if kind == "nd24k":
        rows, (rp, ci, v) = synth.nd24k_like(float(a[0]) if a else 1.0)
    elif kind == "queen":
        rp, ci, v = synth.queen_like_grid(int(a[0]))
        rows, split = len(rp) - 1, int(a[1]) if len(a) > 1 else 1
    else:
        assert kind == "powerlaw", spec
        rows = int(a[0])
        rp, ci, v = synth.powerlaw(rows, avg=float(a[1]), max_len=int(a[2]))
    g = torch.Generator(device=dev)
    g.manual_seed(211)
    lens = torch.from_numpy(np.diff(rp.astype(np.int64))).to(dev)
    row = torch.repeat_interleave(torch.arange(rows, dtype=torch.int32, device=dev), lens)
    col = torch.from_numpy(np.ascontiguousarray(ci)).to(dev)
    val = torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    if split > 1:                          # every entry becomes 1 .. split triplets, each with a share of its value
        k = torch.randint(1, split + 1, (len(ci),), generator=g, device=dev)
        row, col = torch.repeat_interleave(row, k), torch.repeat_interleave(col, k)
        val = torch.repeat_interleave(val / k, k) * (0.5 + torch.rand(int(k.sum()), generator=g, dtype=torch.float64, device=dev))
    p = torch.randperm(row.numel(), generator=g, device=dev)
    return rows, rows, row[p].contiguous(), col[p].contiguous(), val[p].contiguous()


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


def bitlen(n):
    return int(n - 1).bit_length() if n > 1 else 0


def conversion_bytes(rows, cols, nnz, entries, dup):
    """bytes the conversion's passes move: the sort, the row-key gather and the structure / finish passes"""
    cp, rp = (bitlen(cols) + 7) // 8, (bitlen(rows) + 7) // 8
    sort = 20 * nnz * (cp + rp) - (4 * nnz if cp + rp else 0)     # the first pass has no payload to read
    keys = 12 * nnz if cp else 0
    if dup == "keep":
        finish = 36 * nnz                                         # sidx, col, val in; colidx, val, perm, runptr out
    else:
        finish = 24 * nnz + 12 * nnz + 8 * nnz + 8 * entries + 12 * nnz + 12 * entries   # heads, scan, compact, sum
    return dict(passes=cp + rp, sort=sort, row_keys=keys, finish=finish + 4 * (rows + 1), total=sort + keys + finish + 4 * (rows + 1))


def assemble_bytes(nnz, entries, dup):
    return 20 * nnz if dup == "keep" else 12 * nnz + 12 * entries


def host_route(torch, dev, rows, cols, row, col, val, dup):
    """what a user did before: triplets to the host, numpy sort and sum there, CSR back to the device (host clock, ms)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r, c, v = row.cpu().numpy(), col.cpu().numpy(), val.cpu().numpy()
    order = np.lexsort((c, r))
    rs, cs, vs = r[order], c[order], v[order]
    if dup == "keep":
        rowptr, colidx, out = np.searchsorted(rs, np.arange(rows + 1)), cs, vs
    else:
        head = np.ones(len(rs), bool)
        head[1:] = (rs[1:] != rs[:-1]) | (cs[1:] != cs[:-1])
        start = np.flatnonzero(head)
        lens = np.diff(np.append(start, len(rs)))
        out = vs[start].copy()
        for j in range(1, int(lens.max())):
            m = lens > j
            out[m] += vs[start[m] + j]
        rowptr, colidx = np.searchsorted(rs[start], np.arange(rows + 1)), cs[start]
    for a in (rowptr.astype(np.int32), colidx, out):
        torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default=DEFAULT)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--host-max", type=int, default=50000000)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import sblas_amd as S
    if not torch.cuda.is_available():
        raise SystemExit("coo_bench needs a GPU")
    dev = torch.device("cuda:0")
    L = S.lib()
    results = []
    for spec in args.inputs.split(","):
        rows, cols, row, col, val = make_triplets(torch, dev, spec)
        nnz = int(row.numel())
        st = S._stream()
        r = lambda f: timed(torch, f, args.rounds, args.steps)
        rec = dict(input=spec, rows=rows, cols=cols, nnz=nnz)
        rowptr = torch.empty(rows + 1, dtype=torch.int32, device=dev)
        colidx = torch.empty(nnz, dtype=torch.int32, device=dev)
        out = torch.empty(nnz, dtype=torch.float64, device=dev)
        perm = torch.empty(nnz, dtype=torch.int32, device=dev)
        runptr = torch.empty(nnz + 1, dtype=torch.int32, device=dev)
        wsb = S.coo_workspace_bytes(rows, cols, nnz)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        rec["workspace_bytes"] = wsb

        def convert(mode):
            S.check(L.sblas_hip_coo_to_csr_f64_i32(-1, st, rows, cols, nnz, row.data_ptr(), col.data_ptr(), val.data_ptr(), mode,
                                                   rowptr.data_ptr(), colidx.data_ptr(), out.data_ptr(), perm.data_ptr(),
                                                   runptr.data_ptr(), ws.data_ptr(), wsb), "coo_to_csr")
        # the existing transpose of the same matrix (its KEEP CSR), alternated with the conversion
        convert(S.COO_KEEP)
        k_rowptr, k_colidx, k_val = rowptr.clone(), colidx.clone(), out.clone()
        colptr = torch.empty(cols + 1, dtype=torch.int32, device=dev)
        rowidx = torch.empty(nnz, dtype=torch.int32, device=dev)
        valT = torch.empty(nnz, dtype=torch.float64, device=dev)
        permT = torch.empty(nnz, dtype=torch.int32, device=dev)
        twsb = S.transpose_workspace_bytes(rows, cols, nnz)
        tws = torch.empty(max(twsb, 1), dtype=torch.uint8, device=dev)

        def transpose():
            S.check(L.sblas_hip_csr_transpose_f64_i32(-1, st, rows, cols, nnz, k_rowptr.data_ptr(), k_colidx.data_ptr(),
                                                      k_val.data_ptr(), colptr.data_ptr(), rowidx.data_ptr(), valT.data_ptr(),
                                                      permT.data_ptr(), tws.data_ptr(), twsb), "transpose")
        for _ in range(2):                 # alternate, twice; the second round's figures stay
            for dup, mode in (("keep", S.COO_KEEP), ("sum", S.COO_SUM)):
                rec["convert_%s_ms" % dup], rec["convert_%s_rounds" % dup] = r(lambda: convert(mode))
            rec["transpose_ms"], rec["transpose_rounds"] = r(transpose)
        del tws, colptr, rowidx, valT, permT
        tpasses = (bitlen(cols) + 7) // 8
        for dup, mode in (("keep", S.COO_KEEP), ("sum", S.COO_SUM)):
            convert(mode)
            torch.cuda.synchronize()
            entries = int(rowptr[rows].item())
            b = conversion_bytes(rows, cols, nnz, entries, dup)
            ms = rec["convert_%s_ms" % dup]
            rec["convert_%s" % dup] = dict(csr_nnz=entries, bytes=b, achieved_TBps=b["total"] / ms / 1e9,
                                           share_of_8TBps=b["total"] / (ms * 1e-3) / HBM_PEAK,
                                           over_transpose=ms / rec["transpose_ms"], pass_ratio=b["passes"] / max(tpasses, 1),
                                           limit_ms=b["passes"] / max(tpasses, 1) * rec["transpose_ms"] * 1.5)
        del ws, colidx, out, perm, runptr
        # plans: creation on the host clock, then assemble against update_values (the same gather in KEEP mode)
        tp = S.TransposePlan(rows, cols, k_rowptr, k_colidx, k_val)
        plans = {}
        for dup in ("keep", "sum"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            plans[dup] = S.CooPlan(rows, cols, row, col, dup=dup)
            rec["plan_create_%s_ms" % dup] = (time.perf_counter() - t0) * 1e3
            rec["plan_info_%s" % dup] = plans[dup].info()
        outs = {dup: torch.empty(plans[dup].csr_nnz, dtype=torch.float64, device=dev) for dup in plans}
        # the same triplets in CSR order: its KEEP assemble is the same kernel gathering through an identity perm, which
        # separates the kernel's own cost from the cost of gathering from a shuffled array
        srow = torch.repeat_interleave(torch.arange(rows, dtype=torch.int32, device=dev), (k_rowptr[1:] - k_rowptr[:-1]).long())
        sorted_plan = S.CooPlan(rows, cols, srow, k_colidx, dup="keep")
        for _ in range(2):
            rec["update_values_ms"], rec["update_values_rounds"] = r(lambda: tp.update_values(k_val))
            rec["assemble_keep_sorted_input_ms"], _ = r(lambda: sorted_plan.assemble(k_val, out=outs["keep"]))
            for dup in ("keep", "sum"):
                rec["assemble_%s_ms" % dup], rec["assemble_%s_rounds" % dup] = r(lambda: plans[dup].assemble(val, out=outs[dup]))
        for dup in ("keep", "sum"):
            b = assemble_bytes(nnz, plans[dup].csr_nnz, dup)
            ms = rec["assemble_%s_ms" % dup]
            rec["assemble_%s" % dup] = dict(bytes=b, achieved_TBps=b / ms / 1e9, share_of_8TBps=b / (ms * 1e-3) / HBM_PEAK,
                                            over_update_values=ms / rec["update_values_ms"])
            plans[dup].destroy()
        tp.destroy()
        sorted_plan.destroy()
        del k_rowptr, k_colidx, k_val, outs, rowptr, srow
        # for scale only: torch's coalesce on the device, and the host route
        idx = torch.stack([row.long(), col.long()])
        t = torch.sparse_coo_tensor(idx, val, (rows, cols))
        rec["comparison_torch_coalesce_ms"], _ = timed(torch, lambda: t.coalesce(), max(1, args.rounds // 2), 1)
        del idx, t
        if not args.no_host and nnz <= args.host_max:
            for dup in ("keep", "sum"):
                rec["comparison_host_route_%s_ms" % dup] = host_route(torch, dev, rows, cols, row, col, val, dup)
        else:
            rec["comparison_host_route"] = "not measured"
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del row, col, val
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
