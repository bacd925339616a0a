"""The eigenvalue plan (EigshPlan: sblas_hip_eigsh_*) on one GPU, in one process, the routes alternating inside every round
(tools/sptrsv_bench.py's timed: a warm call, then the median of --rounds rounds of device events).

  rotate   the rotation kernel alone at n = 10^6 for (mm, keep) = (20, 12), (32, 19), (64, 37): the time, the bytes it
           moves (8 n (mm + 1) read, 8 n (keep + 1) written) per second, and the same work composed from the older pieces:
           keep calls of gmres_combine into a scratch block, the copy back and the move of column mm.
  cycle    per matrix and (k, ncv): the first restart cycle behind a start (iterate(1), device events), the Ritz
           kernel alone on a T of the shape a restart leaves (the blocks restored outside the timed region), the rotation
           alone; the steps are the remainder.  The Ritz kernel's share of the cycle is reported.
  solve    whole solves to rtol 1e-8 by the host clock (start() to the status() that reports the end), which = LA, and,
           where scipy imports, scipy.sparse.linalg.eigsh on the host for scale.

  python tools/eigsh_bench.py [--inputs rotate,grid,nd24k] [--rounds 5] [--out profiles/r32_eigsh.json]

Matrices: the anisotropic five-point grid (coefficients 1.0 and 0.6) of --grid-side squared rows, and tools/amg_bench.py's
symmetrised nd24k-like matrix."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "s-blas_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ROTATE_SHAPES = ((20, 12), (32, 19), (64, 37))
SIZES = ((4, 20), (10, 64))


def anisotropic_grid(side, cx=1.0, cy=0.6):
    """the five-point grid of side x side points as CSR, rows ascending"""
    n = side * side
    idx = np.arange(n, dtype=np.int64)
    x, y = idx % side, idx // side
    cols = np.stack([idx - side, idx - 1, idx, idx + 1, idx + side], axis=1)
    vals = np.stack([np.full(n, -cy), np.full(n, -cx), np.full(n, 2 * cx + 2 * cy), np.full(n, -cx), np.full(n, -cy)], axis=1)
    live = np.stack([y > 0, x > 0, np.ones(n, bool), x < side - 1, y < side - 1], axis=1)
    rowptr = np.concatenate([[0], np.cumsum(live.sum(axis=1))]).astype(np.int32)
    return n, rowptr, cols[live].astype(np.int32), vals[live].astype(np.float64)


def restart_shaped(mm, kept, seed=0):
    """T as a restart leaves it one cycle later: diag(theta), the arrow in row and column `kept`, a tridiagonal behind it"""
    rng = np.random.default_rng(seed)
    T = np.diag(np.sort(rng.uniform(0.0, 4.0, mm))[::-1])
    T[:kept, kept] = T[kept, :kept] = 1e-3 * rng.standard_normal(kept)
    for j in range(kept, mm - 1):
        T[j, j + 1] = T[j + 1, j] = abs(rng.standard_normal())
    return T


def measure_rotate(torch, S, TB, args):
    dev = torch.device("cuda:0")
    n, out = args.rotate_n, []
    for mm, keep in ROTATE_SHAPES:
        rng = np.random.default_rng(mm)
        V = torch.from_numpy(rng.standard_normal((mm + 1, n))).to(dev)
        Q = torch.from_numpy(np.linalg.qr(rng.standard_normal((mm, mm)))[0][:, :keep].copy()).to(dev)
        Qt = Q.t().contiguous()
        scratch = torch.empty((keep, n), dtype=torch.float64, device=dev)

        def composed():
            for i in range(keep):
                S.gmres_combine(V[:mm], Qt[i], out=scratch[i])
            V[:keep].copy_(scratch)
            V[keep].copy_(V[mm])

        got = TB.timed(torch, {"kernel": lambda: S.eigsh_rotate(V, Q), "composed": composed}, args.rounds)
        moved = 8.0 * n * (mm + 1) + 8.0 * n * (keep + 1)
        out.append(dict(n=n, mm=mm, keep=keep, kernel_ms=got["kernel"][0], kernel_rounds=got["kernel"][1], composed_ms=got["composed"][0],
                        composed_rounds=got["composed"][1], bytes=moved, kernel_gb_per_s=moved / got["kernel"][0] / 1e6,
                        composed_over_kernel=got["composed"][0] / got["kernel"][0], passes_kernel=mm + keep + 2, passes_composed=(mm + 2) * keep))
    return out


def measure_matrix(torch, S, TB, name, args):
    dev = torch.device("cuda:0")
    if name == "grid":
        n, rp, ci, val = anisotropic_grid(args.grid_side)
        label = "anisotropic five-point grid %d^2 (1.0, 0.6)" % args.grid_side
    else:
        import amg_bench as AB
        label, n, rp, ci, val = AB.matrix("nd24k", args)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    drp, dci, dval = up(rp), up(ci), up(val)
    rec = dict(matrix=label, n=int(n), nnz=int(len(ci)), cases=[])
    spmv = S.SpmvPlan(n, n, drp, dci)
    lim = S.eigsh_limits()
    for k, ncv in SIZES:
        plan = S.EigshPlan(n, drp, dci, k, ncv=ncv, which="LA", spmv_plan=spmv)
        keep = plan.keep
        # the Ritz kernel on its own blocks, restored before every timed launch
        blk, mat = S._eigsh_blocks(restart_shaped(ncv, keep), 0.37, 0.0, 0.0, 0, 10 ** 9, False, 0)
        blk0, mat0 = up(blk), up(mat)
        dblk, dmat = blk0.clone(), mat0.clone()
        ritz = []
        for r in range(args.rounds + 1):
            dblk.copy_(blk0), dmat.copy_(mat0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            S.check(S.lib().sblas_hip_eigsh_ritz_f64(-1, None, k, keep, 0, dblk.data_ptr(), dmat.data_ptr()), "ritz")
            e1.record()
            e1.synchronize()
            if r:                                                           # the first loads the code object
                ritz.append(e0.elapsed_time(e1))
        V = torch.from_numpy(np.random.default_rng(1).standard_normal((ncv + 1, n))).to(dev)
        Q = up(np.linalg.qr(np.random.default_rng(2).standard_normal((ncv, ncv)))[0][:, :keep].copy())

        # A live cycle, and checked to be one: a solve that has found its Ritz pairs exactly (their arrow entries negligible,
        # so Jacobi decouples them and the estimates are exact zeros) meets even a zero tolerance, and the cycles behind that
        # are frozen and cost next to nothing.  So the cycle timed is the first, and then the second, behind a start of its
        # own, and the counts behind it must be those of full cycles on a running solve.
        def live_cycle(which_cycle):
            out = []
            for r in range(args.rounds + 1):
                plan.start(dval, rtol=0.0, atol=0.0, max_restarts=10 ** 9)
                plan.iterate(which_cycle - 1)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                plan.iterate(1)
                e1.record()
                e1.synchronize()
                st = plan.status()
                want = (st["status"], st["restarts"], st["matvecs"]) == ("running", which_cycle, keep + which_cycle * (ncv - keep))
                if not want:
                    raise RuntimeError("cycle %d of %s (%d, %d) was not a live one: %r" % (which_cycle, label, k, ncv, st))
                if r:
                    out.append(e0.elapsed_time(e1))
            return out

        cycles, second = live_cycle(1), live_cycle(2)
        got = TB.timed(torch, {"rotate": lambda: S.eigsh_rotate(V, Q), "spmv": lambda: spmv.spmv(dval, V[0], 1.0, 0.0, V[ncv])}, args.rounds)
        cyc, rot, rz = float(np.median(cycles)), got["rotate"][0], float(np.median(ritz))
        # the parts: the Ritz kernel and the rotation are timed alone, on a T of a restart's shape and on a V of the plan's
        # shape (neither kernel's time depends on V's values; Jacobi's sweeps depend on T, and ritz_sweeps says how many
        # this T took); the steps are what is left of the live cycle
        case = dict(k=k, ncv=ncv, keep=keep, cycle_ms=cyc, cycle_rounds=[round(v, 4) for v in cycles], second_cycle_ms=float(np.median(second)),
                    second_cycle_rounds=[round(v, 4) for v in second], ritz_ms=rz, ritz_rounds=[round(v, 4) for v in ritz],
                    ritz_sweeps=S.eigsh_jacobi_ref(restart_shaped(ncv, keep))["sweeps"],
                    rotate_ms=rot, rotate_rounds=got["rotate"][1], spmv_ms=got["spmv"][0], steps_ms=cyc - rz - rot,
                    step_ms=(cyc - rz - rot) / (ncv - keep), ritz_share=rz / cyc, rotate_share=rot / cyc, cycles_checked_live=True,
                    launches=plan.info()["cycle_launches"])
        # whole solves to 1e-8
        solves, rounds = [], args.rounds
        for r in range(args.rounds + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vals, vecs, st = plan.solve(dval, rtol=args.rtol, check_every=args.check_every, max_restarts=args.max_restarts)
            torch.cuda.synchronize()
            if r:
                solves.append((time.perf_counter() - t0) * 1e3)
            elif time.perf_counter() - t0 > args.slow_s:                     # a long solve is timed once, and the record says so
                rounds = 1
            if r >= rounds:
                break
        case.update(solve_ms=float(np.median(solves)), solve_rounds=[round(v, 3) for v in solves], solve_status=st["status"],
                    solve_converged=st["status"] == "converged",
                    restarts=st["restarts"], matvecs=st["matvecs"], theta=[float(v) for v in st["theta"]],
                    residuals=[float(v) for v in st["residuals"]])
        try:
            if n > args.scipy_max_n:
                raise ImportError
            import scipy.sparse as sp
            from scipy.sparse.linalg import eigsh as host_eigsh
            A = sp.csr_matrix((val, ci, rp), shape=(n, n))
            t0 = time.perf_counter()
            lam = host_eigsh(A, k=k, ncv=ncv, which="LA", tol=args.rtol, return_eigenvectors=True)[0]
            case.update(scipy_host_ms=(time.perf_counter() - t0) * 1e3, scipy_theta=[float(v) for v in lam[::-1]])
        except ImportError:
            case["scipy_host_ms"] = None                                     # not measured: no scipy here, or n above --scipy-max-n
        rec["cases"].append(case)
        plan.destroy()
    spmv.destroy()
    rec["limits"] = lim
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="rotate,grid,nd24k")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rotate-n", type=int, default=10 ** 6)
    ap.add_argument("--grid-side", type=int, default=1000)
    ap.add_argument("--nd24k-scale", type=float, default=1.0)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--check-every", type=int, default=4)
    ap.add_argument("--max-restarts", type=int, default=300)
    ap.add_argument("--slow-s", type=float, default=2.0)
    ap.add_argument("--scipy-max-n", type=int, default=100000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import sblas_amd as S
    import sptrsv_bench as TB
    result = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, not_measured=[])
    for name in args.inputs.split(","):
        if name == "rotate":
            result["rotate"] = measure_rotate(torch, S, TB, args)
        else:
            result.setdefault("matrices", []).append(measure_matrix(torch, S, TB, name, args))
        print(json.dumps({name: result["rotate"] if name == "rotate" else result["matrices"][-1]}), flush=True)
    for name in ("rotate", "grid", "nd24k"):
        if name not in args.inputs.split(","):
            result["not_measured"].append(name)
    for rec in result.get("matrices", []):
        for case in rec["cases"]:
            if case["scipy_host_ms"] is None:
                result["not_measured"].append("scipy's eigsh on %s at (%d, %d): no scipy, or n above --scipy-max-n" % (rec["matrix"], case["k"], case["ncv"]))
            if not case["solve_converged"]:
                result["not_measured"].append("a converged solve on %s at (%d, %d): it ended %s at %d restarts, so solve_ms is the time to the cap"
                                              % (rec["matrix"], case["k"], case["ncv"], case["solve_status"], case["restarts"]))
    result["not_measured"] += ["which = SA and LM", "the kernels under the profiler",
                               "the steps, the Ritz kernel and the rotation inside one iterate: the two kernels are timed alone and the steps are the remainder"]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
