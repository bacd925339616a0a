"""The device's parts of a lockstep loop (multi_compose.py, gmres_multi_compose.py) for tools/fuzz_multi.py, and the guarded
blocks its cases solve in.  Parts is the class of tests/test_gpu_gmres_multi.py with two more things a randomised case
needs: every AmgPlan kind (solver_compose.AMG_KINDS) under either smoother, and revalue(val) for a second solve with new
values on the same plans.  A V: an SpmmPlan of width s made as the solvers make theirs (an unsplit plan), called
row-major; the pinned dot per column (a vector met before is not sent again); M^-1 on ONE column: a numpy product with
dinv, AmgPlan.apply or Ilu0Plan.apply.  It is handed (sblas, torch, device) and imports neither."""
import numpy as np

import solver_compose as SC

SENTINEL = -7.0


def up(torch, cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


class Guarded:
    """host (n, s) as a device block at leading dimension ld whose first element sits `offset` elements into an
    allocation, with one guard row before and after and the padding columns all holding the sentinel"""

    def __init__(self, torch, cuda, host, ld=None, offset=0):
        n, s = host.shape
        self.n, self.s, self.ld, self.offset = n, s, (s if ld is None else ld), offset
        self.buf = torch.full((offset + (n + 2) * self.ld + 1,), SENTINEL, dtype=torch.float64, device=cuda)
        self.view = self.buf[offset + self.ld:offset + (n + 1) * self.ld].view(n, self.ld)[:, :s]
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(host)).to(cuda))

    def host(self):
        return self.view.cpu().numpy()

    def intact(self):
        """everything outside the block still holds the sentinel"""
        h = self.buf.cpu().numpy().copy()
        inner = h[self.offset + self.ld:self.offset + (self.n + 1) * self.ld].reshape(self.n, self.ld)
        inner[:, :self.s] = SENTINEL
        return bool((h == SENTINEL).all())


LAYOUTS = ["contiguous", "odd", "even"]


def layout_of(layout, s):
    """((ld, offset) of B, (ld, offset) of X).  "odd": X a slice at an odd offset of a tensor s + 3 wide and B a slice of
    one s + 1 wide, so no row of X starts on 16 bytes twice running; "even": both at an even offset with an even ld, so
    every row starts on 16 bytes -- the 16-byte path is open to the interior tiles and, at an odd s, closed at the tail"""
    if layout == "contiguous":
        return (s, 0), (s, 0)
    if layout == "odd":
        return (s + 1, 0), (s + 3, 1)
    even = s + 2 + s % 2
    return (even, 2), (even, 4)


def blocks(torch, cuda, layout, B, X):
    (ldb, ob), (ldx, ox) = layout_of(layout, B.shape[1])
    return Guarded(torch, cuda, B, ldb, ob), Guarded(torch, cuda, X, ldx, ox)


class Parts:
    """precond: None, "jacobi", "ilu0" or a key of solver_compose.AMG_KINDS; smoother: the AmgPlan's ("jacobi", "l1").
    seat is what KrylovMultiPlan / GmresMultiPlan take as precond, kw() what their start / solve take with it."""

    def __init__(self, env, A, s, precond=None, smoother="jacobi", dinv=None):
        S, torch, cuda = self.env = env
        self.n, self.rp, self.ci = A[0], np.asarray(A[1], np.int32), np.asarray(A[2], np.int32)
        self.s, self.precond, self.smoother, self.given_dinv = s, precond, smoother, dinv
        self.drp, self.dci = up(torch, cuda, self.rp, self.ci)
        self.spmm = S.SpmmPlan(self.n, self.n, self.drp, self.dci, s) if self.n else None      # without rows no loop multiplies
        self.ws = torch.empty(max(S.spmm_workspace_bytes(self.n, self.n, len(self.ci), s) // 8, 1), dtype=torch.float64, device=cuda)
        self.amg = self.ilu = None
        self.seat = precond
        if precond == "ilu0":
            self.ilu = S.Ilu0Plan(self.n, self.drp, self.dci)
            self.seat = self.ilu.solvers()
        elif precond in SC.AMG_KINDS:
            self.seat = self.amg = S.AmgPlan(self.n, self.drp, self.dci, **SC.AMG_KINDS[precond])
        elif precond not in (None, "jacobi"):
            raise KeyError(precond)
        self._sent = {}
        self.revalue(A[3])

    def revalue(self, val):
        """new values on the same structure: the factor and the AMG are set up again, on the same plans"""
        S, torch, cuda = self.env
        self.val = val
        self.dval, = up(torch, cuda, val)
        self.lu = self.dinv = self.ddinv = None
        if self.ilu is not None:
            self.lu = self.ilu.factor(self.dval)
        elif self.amg is not None:
            self.amg.setup(self.dval, smoother=self.smoother)
        elif self.precond == "jacobi":
            self.dinv = np.asarray(self.given_dinv, np.float64) if self.given_dinv is not None else 1.0 / val[SC.stored_diagonal(self.rp, self.ci)]
            self.ddinv, = up(torch, cuda, self.dinv)

    def kw(self):
        return dict(dinv=self.ddinv, lu=self.lu)

    def matvec(self, V):
        S, torch, cuda = self.env
        dv, = up(torch, cuda, V)
        out = torch.empty(self.n * self.s, dtype=torch.float64, device=cuda)
        self.spmm.spmm_ordered(self.dval, dv.reshape(-1), self.s, S.ROW_MAJOR, self.s, 1.0, 0.0, out, self.s, S.ROW_MAJOR, self.ws)
        return out.cpu().numpy().reshape(self.n, self.s)

    def _dev(self, a):
        hit = self._sent.get(id(a))
        if hit is None:
            if len(self._sent) > 256:
                self._sent.clear()
            hit = self._sent[id(a)] = (a, up(self.env[1], self.env[2], a)[0])  # the array is kept, so its id stays its own
        return hit[1]

    def dot(self, a, b):
        S = self.env[0]
        da = self._dev(a)
        same = a.shape == b.shape and a.strides == b.strides and a.__array_interface__["data"][0] == b.__array_interface__["data"][0]
        return float(S.krylov_dot(da, da if same else self._dev(b)).cpu().numpy()[0])    # (v, v): one vector, sent once

    def apply(self, v):
        S, torch, cuda = self.env
        if self.amg is not None:
            return self.amg.apply(up(torch, cuda, v)[0]).cpu().numpy()
        if self.ilu is not None:
            return self.ilu.apply(self.lu, up(torch, cuda, v)[0]).cpu().numpy()
        return self.dinv * v if self.dinv is not None else v

    def destroy(self):
        self._sent.clear()
        for p in (self.spmm, self.amg, self.ilu):
            if p is not None:
                p.destroy()
        self.spmm = self.amg = self.ilu = None
