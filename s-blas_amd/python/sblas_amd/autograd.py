"""Autograd for the sparse products: C = A B and y = A x differentiable in A's values and in the dense operand.

    op = CsrOperator(rows, cols, rowptr, colidx, n=64)
    C = op.matmul(val, B)         # val: nnz values (requires_grad or not), B: cols x n
    y = op.matvec(val, x)
    S = op.sddmm(X, Y)            # nnz scores on A's pattern: S[e] = <X[row e], Y[col e]>, differentiable in X and Y
    P = op.softmax(S, scale=s)    # softmax of scale * S over the stored entries of each row, differentiable in S
    O = op.attention(Q, K, V, scale=s)   # op.matmul(op.softmax(op.sddmm(Q, K), s), V) in one kernel, nothing nnz-sized kept

Forward is the library's SpMM / SpMV.  Backward computes only the halves autograd asks for:
    dval = SDDMM(X = dC, Y = B) on A's pattern        (sddmm_tensor; k = 1 for matvec)
    dB   = A^T dC                                     (a TransposePlan the operator makes on the first backward that needs
                                                       it and refreshes with the values of that forward)
sddmm is the same pair read the other way: dX = A(dout) Y through the SpMM path, dY = A(dout)^T X through the
TransposePlan.  softmax keeps its output and runs the library's softmax backward on it.  attention keeps Q, K, V and two
doubles per row; its backward recomputes the probabilities, takes dQ from the fused kernel and forms dK = A(dS)^T Q and
dV = A(P)^T dO through the TransposePlan, from P and dS that live only inside that backward.
csr_add(plan, val_a, val_b, alpha, beta), a function beside the operator, is the CSR sum on a GeamPlan, differentiable in
both value arrays: its backward is a gather over the plan's maps.
SpgemmOperator is the sparse-sparse product C = A B on a SpgemmPlan, differentiable in both value arrays:
    op = SpgemmOperator(m, k, n, rowptr_a, colidx_a, rowptr_b, colidx_b)
    rowptr_c, colidx_c = op.csr()
    val_c = op.multiply(val_a, val_b)    # spgemm_multiply(op, val_a, val_b): SpgemmPlan.multiply's bits
Both gradients are masked SpGEMMs (MaskedSpgemmPlan, out = M o (X Y^T)), each on a plan the first backward that needs it
makes, with no transposed kernel:
    dval_a = A's pattern o (dC B^T)               mask = A, X = dC on C's pattern, Y = B
    dval_b = B's pattern o (A^T (dC^T)^T)         mask = B, X = A^T, Y = C^T: two TransposePlans, refreshed with that
                                                  forward's val_a and with dC
A duplicated entry of A or B receives the full gradient of its position, since C depends on the sum of the duplicates.
TriangularOperator and SolveOperator make the solves differentiable in the matrix values and the right-hand side:
    x = TriangularOperator(n, rowptr, colidx, lower=True).solve(val, b, alpha)       # SptrsvPlan's solve, its bits
    x = SolveOperator(n, rowptr, colidx, method="gmres", precond="ilu0").solve(val, b)   # the Krylov plans
Backward is one more solve, with the transposed matrix, g = A^-T xbar, then bbar = g and valbar[e] = -<g[row e], x[col e]>
on the pattern, an SDDMM as narrow as the block of right-hand sides: sddmm_narrow on a triangle of up to four columns,
where it was measured faster, sddmm_tensor everywhere else (the two agree bit for bit).
Backward of backward is not supported.  float64 values, int32 indices, GPU tensors only: there is no CPU path.
torch is imported here, not by the package."""
import ctypes as C

import torch

from . import (ATTENTION_MAX_WIDTH, ROW_MAJOR, AmgPlan, GeamPlan, GmresMultiPlan, GmresPlan, Ilu0Plan, KrylovMultiPlan, KrylovPlan,
               MaskedSpgemmPlan, SblasError, SpgemmPlan, SpmmPlan, SpmvPlan, SptrsvPlan, TransposePlan, _DeviceArray,
               _layout, check, csr_attention,
               csr_attention_backward, csr_attention_workspace_bytes, csr_softmax, csr_softmax_backward,
               csr_softmax_workspace_bytes, gather, sddmm_narrow, sddmm_tensor, lib, sddmm_workspace_bytes, spmm_tensor, spmm_workspace_bytes)


class CsrOperator:
    """One CSR structure (rows x cols, int32 rowptr / colidx on the GPU) whose values change from call to call.  Owns the
    plans and workspaces of its products and reuses them: n > 0 makes an SpmmPlan of that width (other widths run
    unplanned) and the first matvec an SpmvPlan; split=True makes the split forms of the SpMM plans (very long rows and, in the transpose,
    very long columns).  One call at a time per operator, as for the plans."""

    def __init__(self, rows, cols, rowptr, colidx, n=0, split=False):
        if not isinstance(rowptr, torch.Tensor) or not isinstance(colidx, torch.Tensor):
            raise SblasError("rowptr and colidx must be torch tensors")
        if not rowptr.is_cuda or not colidx.is_cuda:
            raise SblasError("rowptr and colidx must be GPU tensors (no CPU path exists)")
        if rowptr.dtype != torch.int32 or colidx.dtype != torch.int32 or not rowptr.is_contiguous() or not colidx.is_contiguous():
            raise SblasError("rowptr and colidx must be contiguous int32 tensors")
        if rows < 0 or cols < 0 or rowptr.dim() != 1 or colidx.dim() != 1 or rowptr.numel() != rows + 1:
            raise SblasError("rowptr must hold rows + 1 = %d entries, got shape %s" % (rows + 1, tuple(rowptr.shape)))
        self.rows, self.cols, self.rowptr, self.colidx = int(rows), int(cols), rowptr, colidx
        self.nnz = int(colidx.numel())
        self.n, self.split = int(n), bool(split)
        self.device = rowptr.device
        self.spmm_plan = SpmmPlan(rows, cols, rowptr, colidx, n, split=split) if n > 0 and self.nnz else None
        self.spmv_plan = None            # made by the first matvec
        self.transpose_plan = None       # made by the first backward that needs dB / dx
        self._ws = {}                    # workspaces by purpose, grown on demand

    # ---- argument checks --------------------------------------------------------------------------------------------
    def _check_val(self, val):
        if not isinstance(val, torch.Tensor) or not val.is_cuda:
            raise SblasError("val must be a GPU tensor (no CPU path exists)")
        if val.dtype != torch.float64 or val.dim() != 1 or val.numel() != self.nnz:
            raise SblasError("val must be a float64 tensor of %d entries, got %s %s" % (self.nnz, val.dtype, tuple(val.shape)))

    def _check_dense(self, t, rows, what, dim):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise SblasError("%s must be a GPU tensor (no CPU path exists)" % what)
        if t.dtype != torch.float64:
            raise SblasError("%s must be float64, got %s" % (what, t.dtype))
        if t.dim() != dim or t.shape[0] != rows:
            raise SblasError("%s must have %d dimension(s) and %d rows, got shape %s" % (what, dim, rows, tuple(t.shape)))
        if dim == 2:
            _layout(t, rows, int(t.shape[1]), what)   # raises on strides no kernel reads
        elif t.numel() > 1 and t.stride(0) != 1:
            raise SblasError("%s must be contiguous, got stride %d" % (what, t.stride(0)))

    def _workspace(self, key, nbytes):
        ws = self._ws.get(key)
        if ws is None or ws.numel() * 8 < nbytes:
            ws = self._ws[key] = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=self.device)
        return ws

    # ---- products ---------------------------------------------------------------------------------------------------
    def matmul(self, val, B):
        """C (rows x n) = A(val) @ B (cols x n), differentiable in val and B."""
        self._check_val(val)
        self._check_dense(B, self.cols, "B", 2)
        return _Matmul.apply(val, B, self)

    def matvec(self, val, x):
        """y (rows) = A(val) @ x (cols), differentiable in val and x."""
        self._check_val(val)
        self._check_dense(x, self.cols, "x", 1)
        return _Matvec.apply(val, x, self)

    def sddmm(self, X, Y):
        """out (nnz) with out[e] = <X[row(e), :], Y[col(e), :]> on A's pattern; X rows x k, Y cols x k, differentiable in
        both."""
        self._check_dense(X, self.rows, "X", 2)
        self._check_dense(Y, self.cols, "Y", 2)
        if X.shape[1] != Y.shape[1]:
            raise SblasError("X and Y must have the same number of columns, got %d and %d" % (X.shape[1], Y.shape[1]))
        return _Sddmm.apply(X, Y, self)

    def softmax(self, val, scale=1.0):
        """P (nnz) = softmax of scale * val over the stored entries of each row of A, differentiable in val."""
        self._check_val(val)
        return _Softmax.apply(val, self, float(scale))

    def attention(self, Q, K, V, scale=1.0):
        """O (rows x dv) = softmax(scale * Q K^T on A's pattern) V: what op.matmul(op.softmax(op.sddmm(Q, K), scale), V)
        computes, in one fused kernel that writes no nnz-sized array and keeps only Q, K, V and two doubles per row for
        the backward (the composition holds 16 bytes per stored entry at the peak of its forward, S beside P, and keeps
        8, P, until its backward).  Q rows x d, K cols x d, V cols x dv;
        differentiable in all three, and the backward forms only the gradients autograd asks for.  The probabilities
        and score gradients are the composition's bit for bit, hence dK and dV too; O and dQ are accumulated in the
        fused kernels' own fixed order (include/sblas_hip.h, "Fused attention"), a function of the row alone.
        Inputs outside the fused kernels' limits -- d or dv above 128 (or 0), or a column-major Q, K or V -- run the
        composition itself, with its bits for O and dQ as well.
        Speed (measured against the composition in the same run): the fused route is slower wherever no
        row is long -- 1.6 to 3.8 x forward on the banded bench matrix, a Queen-like grid and banded rows of 5 at 16 and
        64 columns -- because a wave walks one row at a time and waits on the gathers of K and V rows through L2, where
        the composition's SDDMM and (LDS-tiled) SpMM keep far more loads in flight; it is faster (0.5 x at 64 columns,
        0.03 x at 16) on a power law with a 10^6-entry row, which it spreads over many waves.  It is kept for the memory."""
        self._check_dense(Q, self.rows, "Q", 2)
        self._check_dense(K, self.cols, "K", 2)
        self._check_dense(V, self.cols, "V", 2)
        if Q.shape[1] != K.shape[1]:
            raise SblasError("Q and K must have the same number of columns, got %d and %d" % (Q.shape[1], K.shape[1]))
        d, dv = int(Q.shape[1]), int(V.shape[1])
        fused = 1 <= d <= ATTENTION_MAX_WIDTH and 1 <= dv <= ATTENTION_MAX_WIDTH and all(
            _layout(t, r, w, what)[0] == ROW_MAJOR for t, r, w, what in ((Q, self.rows, d, "Q"), (K, self.cols, d, "K"),
                                                                        (V, self.cols, dv, "V")))
        if not fused:
            return self.matmul(self.softmax(self.sddmm(Q, K), scale), V)
        return _Attention.apply(Q, K, V, self, float(scale))

    # ---- the pieces the Functions call --------------------------------------------------------------------------------
    def _forward_mm(self, val, B):
        n = int(B.shape[1])
        C_ = torch.empty(self.rows, n, dtype=torch.float64, device=self.device)
        if n == 0 or self.rows == 0:
            return C_
        plan = self.spmm_plan if n == self.n else None
        ws = self._workspace("spmm", spmm_workspace_bytes(self.rows, self.cols, self.nnz, n))
        spmm_tensor((self.rows, self.cols, self.rowptr, self.colidx, val), B, C_, 1.0, 0.0, workspace=ws, plan=plan)
        return C_

    def _forward_mv(self, val, x):
        y = torch.empty(self.rows, dtype=torch.float64, device=self.device)
        if self.rows == 0:
            return y
        if self.nnz == 0 or self.cols == 0:
            return y.zero_()
        if self.spmv_plan is None:
            self.spmv_plan = SpmvPlan(self.rows, self.cols, self.rowptr, self.colidx)
        self.spmv_plan(val, x, 1.0, 0.0, y)
        return y

    def _grad_val(self, dC, B):
        """dval[e] = <dC[row(e), :], B[col(e), :]>"""
        out = torch.empty(self.nnz, dtype=torch.float64, device=self.device)
        k = int(dC.shape[1])
        need = sddmm_workspace_bytes(self.rows, self.cols, self.nnz, k, _layout(dC, self.rows, k, "dC")[0],
                                     _layout(B, self.cols, k, "B")[0])
        sddmm_tensor((self.rows, self.cols, self.rowptr, self.colidx), dC, B, out, 1.0, 0.0,
                     workspace=self._workspace("sddmm", need) if need else None)
        return out

    def _transpose(self, val):
        """A^T with the values of `val`: the plan keeps its own copy, so it is refreshed on every use"""
        if self.transpose_plan is None:
            self.transpose_plan = TransposePlan(self.rows, self.cols, self.rowptr, self.colidx, val, n=self.n, split=self.split)
        else:
            self.transpose_plan.update_values(val)
        return self.transpose_plan

    def _grad_dense_mm(self, val, dC):
        n = int(dC.shape[1])
        dB = torch.empty(self.cols, n, dtype=torch.float64, device=self.device)
        if n == 0 or self.cols == 0:
            return dB
        tp = self._transpose(val)
        ws = self._workspace("spmm_t", spmm_workspace_bytes(self.cols, self.rows, self.nnz, n))
        tp.spmm_tensor(dC, dB, 1.0, 0.0, workspace=ws)
        return dB

    def _grad_dense_mv(self, val, dy):
        dx = torch.empty(self.cols, dtype=torch.float64, device=self.device)
        if self.cols == 0:
            return dx
        self._transpose(val).spmv(dy, 1.0, 0.0, dx)
        return dx

    def _softmax_workspace(self):
        need = csr_softmax_workspace_bytes(self.rows, self.nnz)
        return self._workspace("softmax", need) if need else None

    def _forward_softmax(self, val, scale):
        out = torch.empty(self.nnz, dtype=torch.float64, device=self.device)
        return csr_softmax(self.rowptr, val.contiguous(), out, scale, workspace=self._softmax_workspace())

    def _grad_softmax(self, p, dp, scale):
        dx = torch.empty(self.nnz, dtype=torch.float64, device=self.device)
        return csr_softmax_backward(self.rowptr, p, dp, dx, scale, workspace=self._softmax_workspace())

    def _attention_workspace(self, d, dv):
        need = csr_attention_workspace_bytes(self.rows, self.nnz, d, dv)
        return self._workspace("attention", need) if need else None

    def _pattern(self):
        return self.rows, self.cols, self.rowptr, self.colidx

    def destroy(self):
        for p in (self.spmm_plan, self.spmv_plan, self.transpose_plan):
            if p is not None:
                p.destroy()
        self.spmm_plan = self.spmv_plan = self.transpose_plan = None
        self._ws.clear()


def _laid_out(g):
    """An incoming gradient as a tensor the kernels can read: an expanded one (C.sum().backward() delivers strides
    (0, 0)) or any other view that is neither (ld, 1) nor (1, ld) is made contiguous."""
    if g.dim() == 1:
        return g if g.numel() <= 1 or g.stride(0) == 1 else g.contiguous()
    s0, s1 = g.stride()
    r, c = g.shape
    if (s1 == 1 and s0 >= max(c, 1)) or (s0 == 1 and s1 >= max(r, 1)):
        return g
    return g.contiguous()


class _Matmul(torch.autograd.Function):
    @staticmethod
    def forward(ctx, val, B, op):
        ctx.op = op
        ctx.save_for_backward(val, B)
        return op._forward_mm(val.detach(), B.detach())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dC):
        val, B = ctx.saved_tensors
        op = ctx.op
        dC = _laid_out(dC)
        dval = op._grad_val(dC, B) if ctx.needs_input_grad[0] else None
        dB = op._grad_dense_mm(val, dC) if ctx.needs_input_grad[1] else None
        return dval, dB, None


class _Matvec(torch.autograd.Function):
    @staticmethod
    def forward(ctx, val, x, op):
        ctx.op = op
        ctx.save_for_backward(val, x)
        return op._forward_mv(val.detach(), x.detach())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        val, x = ctx.saved_tensors
        op = ctx.op
        dy = _laid_out(dy)
        dval = op._grad_val(dy.view(-1, 1), x.view(-1, 1)) if ctx.needs_input_grad[0] else None
        dx = op._grad_dense_mv(val, dy) if ctx.needs_input_grad[1] else None
        return dval, dx, None


class _Sddmm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, Y, op):
        ctx.op = op
        ctx.save_for_backward(X, Y)
        return op._grad_val(X.detach(), Y.detach())      # the SDDMM itself: <X[row], Y[col]> per stored entry

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        X, Y = ctx.saved_tensors
        op = ctx.op
        dout = _laid_out(dout)
        dX = op._forward_mm(dout, Y) if ctx.needs_input_grad[0] else None        # A(dout) Y
        dY = op._grad_dense_mm(dout, X) if ctx.needs_input_grad[1] else None     # A(dout)^T X
        return dX, dY, None


class _Softmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, val, op, scale):
        ctx.op, ctx.scale = op, scale
        p = op._forward_softmax(val.detach(), scale)
        ctx.save_for_backward(p)
        return p

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dp):
        p, = ctx.saved_tensors
        return ctx.op._grad_softmax(p, _laid_out(dp), ctx.scale), None, None


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Q, K, V, op, scale):
        ctx.op, ctx.scale = op, scale
        Q, K, V = Q.detach(), K.detach(), V.detach()
        d, dv = int(Q.shape[1]), int(V.shape[1])
        O = torch.empty(op.rows, dv, dtype=torch.float64, device=op.device)
        m = z = None
        if any(ctx.needs_input_grad[:3]):                # inference keeps nothing
            m = torch.empty(op.rows, dtype=torch.float64, device=op.device)
            z = torch.empty(op.rows, dtype=torch.float64, device=op.device)
            ctx.save_for_backward(Q, K, V, m, z)
        csr_attention(op._pattern(), Q, K, V, scale, O, m, z, workspace=op._attention_workspace(d, dv))
        return O

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dO):
        Q, K, V, m, z = ctx.saved_tensors
        op = ctx.op
        need_q, need_k, need_v = ctx.needs_input_grad[:3]
        dO = _laid_out(dO)
        dO_rows = dO if _layout(dO, op.rows, int(dO.shape[1]), "dO")[0] == ROW_MAJOR else dO.contiguous()
        d, dv = int(Q.shape[1]), int(V.shape[1])
        new = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=op.device)
        dQ = new(op.rows, d) if need_q else None
        P = new(op.nnz) if need_v else None              # transient: nothing nnz-sized outlives this call
        dS = new(op.nnz) if need_k else None
        csr_attention_backward(op._pattern(), Q, K, V, dO_rows, m, z, ctx.scale, dQ, P, dS, workspace=op._attention_workspace(d, dv))
        dK = op._grad_dense_mm(dS, Q) if need_k else None    # A(dS)^T Q
        dV = op._grad_dense_mm(P, dO) if need_v else None    # A(P)^T dO
        return dQ, dK, dV, None, None


class _CsrAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, val_a, val_b, plan, alpha, beta):
        ctx.plan, ctx.alpha, ctx.beta = plan, alpha, beta
        return plan.add(val_a.detach(), val_b.detach(), alpha, beta)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dC):
        plan = ctx.plan
        dC = _laid_out(dC)
        grads = []
        for need, dest, scale in zip(ctx.needs_input_grad[:2], plan.maps(), (ctx.alpha, ctx.beta)):
            g = None
            if need:                                     # dval[e] = scale * dC[dest[e]]: the library's gather, then one rounding
                g = torch.empty(dest.numel(), dtype=torch.float64, device=plan.device)
                gather(dest, dC, g)
                g.mul_(scale)
            grads.append(g)
        return grads[0], grads[1], None, None, None


def csr_add(plan, val_a, val_b, alpha=1.0, beta=1.0):
    """C's values of alpha * A + beta * B on a GeamPlan, differentiable in val_a and val_b (alpha and beta are plain
    numbers): dval_a = alpha * dC[dest_a] and dval_b = beta * dC[dest_b] over the plan's maps, so a run of duplicates
    that shares one entry of C shares its gradient.  Only the halves autograd asks for are computed; backward of backward
    is not supported."""
    if not isinstance(plan, GeamPlan):
        raise SblasError("csr_add needs a GeamPlan")
    return _CsrAdd.apply(val_a, val_b, plan, float(alpha), float(beta))


class SpgemmOperator:
    """C = A B for two CSR structures (A m x k, B k x n, int32 rowptr / colidx on the GPU; rows may be unsorted and hold
    duplicates) whose values change from call to call.  Owns the SpgemmPlan -- csr() passes through -- and, each made by
    the first backward that needs it, the two MaskedSpgemmPlans of the gradients and the two TransposePlans dval_b reads
    (grad_a_plan; grad_b_plan, transpose_a, transpose_c).  general=True sends the product and both gradients through their
    general paths.  One call at a time per operator, as for the plans."""

    def __init__(self, m, k, n, rowptr_a, colidx_a, rowptr_b, colidx_b, general=False):
        for name, t in (("rowptr_a", rowptr_a), ("colidx_a", colidx_a), ("rowptr_b", rowptr_b), ("colidx_b", colidx_b)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise SblasError("%s must be a GPU tensor (no CPU path exists)" % name)
        self.m, self.k, self.n, self.general = int(m), int(k), int(n), bool(general)
        self.a, self.b = (rowptr_a, colidx_a), (rowptr_b, colidx_b)
        self.plan = SpgemmPlan(m, k, n, rowptr_a, colidx_a, rowptr_b, colidx_b, general=general)
        self.device = self.plan.device
        self.nnz_a, self.nnz_b, self.nnz_c = self.plan.nnz_a, self.plan.nnz_b, self.plan.nnz_c
        self.grad_a_plan = self.grad_b_plan = self.transpose_a = self.transpose_c = None

    def csr(self):
        """(rowptr_c, colidx_c): the SpgemmPlan's views; they live as long as the operator."""
        return self.plan.csr()

    def multiply(self, val_a, val_b):
        """C's values (nnz_c of them), differentiable in val_a and val_b: spgemm_multiply(self, val_a, val_b)."""
        return spgemm_multiply(self, val_a, val_b)

    def _no_pairs(self):
        return self.nnz_a == 0 or self.nnz_b == 0 or self.nnz_c == 0     # every entry of both gradients is the empty sum, +0.0

    def _grad_a(self, dC, val_b):
        if self._no_pairs():
            return torch.zeros(self.nnz_a, dtype=torch.float64, device=self.device)
        if self.grad_a_plan is None:
            self.grad_a_plan = MaskedSpgemmPlan(self.m, self.k, self.n, *self.a, *self.plan.csr(), *self.b, general=self.general)
        return self.grad_a_plan.multiply(dC, val_b)

    def _transposed(self, which, rows, cols, structure, val):
        """the TransposePlan `which`, made with or refreshed to the values of `val`"""
        tp = getattr(self, which)
        if tp is None:
            tp = TransposePlan(rows, cols, structure[0], structure[1], val)
            setattr(self, which, tp)
        else:
            tp.update_values(val)
        return tp

    def _grad_b(self, val_a, dC):
        if self._no_pairs():
            return torch.zeros(self.nnz_b, dtype=torch.float64, device=self.device)
        ta = self._transposed("transpose_a", self.m, self.k, self.a, val_a)
        tc = self._transposed("transpose_c", self.m, self.n, self.plan.csr(), dC)
        if self.grad_b_plan is None:                                     # the plan copies the structures it is given
            self.grad_b_plan = MaskedSpgemmPlan(self.k, self.n, self.m, *self.b, *ta.csc()[:2], *tc.csc()[:2], general=self.general)
        return self.grad_b_plan.multiply(_transposed_values(ta), _transposed_values(tc))

    def destroy(self):
        for p in (self.plan, self.grad_a_plan, self.grad_b_plan, self.transpose_a, self.transpose_c):
            if p is not None:
                p.destroy()
        self.grad_a_plan = self.grad_b_plan = self.transpose_a = self.transpose_c = None


def _transposed_values(tp):
    """a view of a TransposePlan's own transposed values (nnz > 0): read at once, on the stream that refreshed them"""
    vt = C.c_void_p()
    check(lib().sblas_hip_transpose_plan_csc(tp.handle, None, None, C.byref(vt)), "sblas_hip_transpose_plan_csc")
    return torch.as_tensor(_DeviceArray(vt.value, tp.nnz, "<f8"), device=tp.device)


class _SpgemmMultiply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, val_a, val_b, op):
        ctx.op = op
        ctx.save_for_backward(val_a, val_b)
        return op.plan.multiply(val_a.detach(), val_b.detach())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dC):
        val_a, val_b = ctx.saved_tensors
        op = ctx.op
        dC = _laid_out(dC)
        dA = op._grad_a(dC, val_b) if ctx.needs_input_grad[0] else None
        dB = op._grad_b(val_a, dC) if ctx.needs_input_grad[1] else None
        return dA, dB, None


def spgemm_multiply(op, val_a, val_b):
    """C's values of A B on a SpgemmOperator, differentiable in val_a and val_b: dval_a = (dC B^T) on A's pattern and
    dval_b = (A^T dC) on B's, both masked SpGEMMs in the contract's fixed order.  Only the halves autograd asks for are
    computed; backward of backward is not supported."""
    if not isinstance(op, SpgemmOperator):
        raise SblasError("spgemm_multiply needs a SpgemmOperator")
    for name, t in (("val_a", val_a), ("val_b", val_b)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise SblasError("%s must be a GPU tensor (no CPU path exists)" % name)
    return _SpgemmMultiply.apply(val_a, val_b, op)


# ----------------------------------------------------------------------------------------------------------------------
# Differentiable solves.  From T x = alpha b:  dx = -T^-1 dT x + alpha T^-1 db.  With g = T^-T xbar this gives
#     bbar = alpha g        valbar[e] = -<g[row(e), :], x[col(e), :]>   on the stored entries the solve reads
# an SDDMM at k = the number of right-hand sides.  sddmm_narrow and sddmm_tensor agree bit for bit, so the choice between
# them is a question of time only, and the rule is: the narrow kernel where tools/solve_grad_bench.py measured it faster
# on most of its matrices, sddmm_tensor everywhere else (profiles/r30_solve_grad.json).  On the whole pattern it is not
# (1.02 - 1.03 x sddmm_tensor's time at k = 1 and 2 on three matrices of four, more beyond), so a SolveOperator's values
# gradient is sddmm_tensor at every width.  On a triangle sddmm_tensor computes every entry and needs a mask pass after
# it, while the narrow kernel reads only the rows of the entries inside the part: 0.66 - 0.79 x the time of sddmm_tensor
# + masked_fill_ at k = 1, 2 and 4 on all four matrices, but 0.83 - 1.07 x at k = 8, faster on two of four.  So a
# TriangularOperator takes the narrow kernel up to NARROW_TRIANGLE_MAX = 4 columns (3 lies between two measured widths;
# 5 to 7 were not measured and go with 8).
# ----------------------------------------------------------------------------------------------------------------------
NARROW_TRIANGLE_MAX = 4


def _row_major(g):
    """an incoming gradient as the solves read it: 1-D contiguous, or 2-D with strides (ld, 1)"""
    g = _laid_out(g)
    if g.dim() == 2 and g.shape[1] > 1 and g.stride(1) != 1:
        g = g.contiguous()
    return g


def _check_solve_args(n, nnz, val, b, what):
    for name, t in (("val", val), ("b", b)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise SblasError("%s: %s must be a GPU tensor (no CPU path exists)" % (what, name))
        if t.dtype != torch.float64:
            raise SblasError("%s: %s must be float64, got %s" % (what, name, t.dtype))
    if val.dim() != 1 or val.numel() != nnz:
        raise SblasError("%s: val must hold one value per stored entry (%d), got shape %s" % (what, nnz, tuple(val.shape)))
    if b.dim() not in (1, 2) or b.shape[0] != n:
        raise SblasError("%s: b must hold %d entries or be %d x s, got shape %s" % (what, n, n, tuple(b.shape)))


def _values_gradient(pattern, g, x, part, mask):
    """-<g[row(e), :], x[col(e), :]> on the part of the pattern; mask() gives the part as a bool tensor for the wide route"""
    out = torch.empty(int(pattern[3].numel()), dtype=torch.float64, device=pattern[2].device)
    s = 1 if g.dim() == 1 else int(g.shape[1])
    if part != "all" and s <= NARROW_TRIANGLE_MAX:
        return sddmm_narrow(pattern, g, x, out, -1.0, 0.0, part=part)
    if g.dim() == 1:
        g, x = g.view(-1, 1), x.view(-1, 1)
    sddmm_tensor(pattern, g, x, out, -1.0, 0.0)
    if part != "all":
        out.masked_fill_(~mask(), 0.0)                   # beyond the narrow kernel's widths the part is cut out afterwards
    return out


class TriangularOperator:
    """T x = alpha b on the lower or upper triangle of one n x n CSR structure (int32 rowptr / colidx on the GPU; rows may
    be unsorted, hold duplicates and entries of the other triangle) whose values change from call to call, differentiable
    in val and b:

        op = TriangularOperator(n, rowptr, colidx, lower=True, unit_diag=False)
        x = op.solve(val, b, alpha=1.0)        # triangular_solve(op, val, b, alpha); b: n entries, or n x s row-major

    Forward is SptrsvPlan.solve (b 1-D) or solve_multi (b 2-D), with their bits.  Backward solves T^T g = xbar on a second
    SptrsvPlan with the opposite `lower` over TransposePlan.csc()'s arrays -- both made by the first backward, the
    transposed values refreshed from that forward's val -- and returns bbar = alpha g and valbar[e] = -<g[row(e)],
    x[col(e)]> on the part of the pattern the solve reads: LOWER / UPPER, STRICT_* with unit_diag.  Entries the solve
    ignores receive exactly +0.0; a duplicated off-diagonal entry receives the full gradient of its position.  Only the
    halves autograd asks for are computed; backward of backward is not supported.  One call at a time per operator."""

    def __init__(self, n, rowptr, colidx, lower=True, unit_diag=False, mode="auto"):
        self.plan = SptrsvPlan(n, rowptr, colidx, lower=lower, unit_diag=unit_diag, mode=mode)
        self.n, self.rowptr, self.colidx, self.nnz = int(n), rowptr, colidx, int(colidx.numel())
        self.lower, self.unit_diag, self.mode, self.device = bool(lower), bool(unit_diag), mode, rowptr.device
        self.part = ("strict_" if unit_diag else "") + ("lower" if lower else "upper")
        self.transpose_plan = self.adjoint_plan = None   # made by the first backward
        self._csc = self._mask = None

    def solve(self, val, b, alpha=1.0):
        """x with T(val) x = alpha b, differentiable in val and b."""
        return triangular_solve(self, val, b, alpha)

    def _pattern(self):
        return self.n, self.n, self.rowptr, self.colidx

    def _part_mask(self):
        if self._mask is None:
            rows = torch.repeat_interleave(torch.arange(self.n, dtype=torch.int32, device=self.device),
                                           (self.rowptr[1:] - self.rowptr[:-1]).long())
            c = self.colidx
            self._mask = {"lower": c <= rows, "upper": c >= rows, "strict_lower": c < rows, "strict_upper": c > rows}[self.part]
        return self._mask

    def _forward(self, val, b, alpha):
        if b.dim() == 1:
            return self.plan.solve(val, b.contiguous(), alpha=alpha)
        return self.plan.solve_multi(val, _row_major(b), alpha=alpha)

    def _adjoint(self, val, dx):
        """g with T(val)^T g = dx"""
        if self.transpose_plan is None:
            self.transpose_plan = TransposePlan(self.n, self.n, self.rowptr, self.colidx, val)
            self._csc = self.transpose_plan.csc()[:2]    # the adjoint plan keeps these copies alive and solves on them
            self.adjoint_plan = SptrsvPlan(self.n, self._csc[0], self._csc[1], lower=not self.lower, unit_diag=self.unit_diag,
                                           mode=self.mode)
        else:
            self.transpose_plan.update_values(val)
        val_t = _transposed_values(self.transpose_plan) if self.nnz else val
        return self.adjoint_plan.solve(val_t, dx) if dx.dim() == 1 else self.adjoint_plan.solve_multi(val_t, dx)

    def destroy(self):
        for p in (self.plan, self.adjoint_plan, self.transpose_plan):
            if p is not None:
                p.destroy()
        self.adjoint_plan = self.transpose_plan = self._csc = self._mask = None


class _TriangularSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, val, b, op, alpha):
        ctx.op, ctx.alpha = op, alpha
        x = op._forward(val.detach().contiguous(), b.detach(), alpha)
        ctx.save_for_backward(val, x)
        return x

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dx):
        val, x = ctx.saved_tensors
        op = ctx.op
        g = op._adjoint(val.detach().contiguous(), _row_major(dx))
        dval = _values_gradient(op._pattern(), g, x, op.part, op._part_mask) if ctx.needs_input_grad[0] else None
        db = (g if ctx.alpha == 1.0 else g * ctx.alpha) if ctx.needs_input_grad[1] else None
        return dval, db, None, None


def triangular_solve(op, val, b, alpha=1.0):
    """x with T(val) x = alpha b on a TriangularOperator, differentiable in val and b (alpha is a plain number)."""
    if not isinstance(op, TriangularOperator):
        raise SblasError("triangular_solve needs a TriangularOperator")
    _check_solve_args(op.n, op.nnz, val, b, "triangular_solve")
    return _TriangularSolve.apply(val, b, op, float(alpha))


_SOLVE_METHODS = ("pcg", "bicgstab", "gmres")
_SOLVE_PRECONDS = (None, "jacobi", "ilu0", "amg", "amg_smoothed")


class _SolveSide:
    """The plans of one system of a SolveOperator -- A's or A^T's: the preconditioner it owns and refreshes from the values,
    and a solver plan per width (0: one right-hand side on KrylovPlan / GmresPlan; s: KrylovMultiPlan / GmresMultiPlan)."""

    def __init__(self, op, rowptr, colidx, dinv_from=None):
        self.op, self.rowptr, self.colidx = op, rowptr, colidx
        self.plans, self.ilu, self.amg, self.dinv, self.lu = {}, None, None, None, None
        self.dinv_from = dinv_from                       # Jacobi: diag(A^T) = diag(A), the forward side's dinv serves
        n = op.n
        if op.precond == "ilu0" or (op.precond == "jacobi" and dinv_from is None):
            self.ilu = Ilu0Plan(n, rowptr, colidx)       # Jacobi takes only the diagonal's positions from it
        elif op.precond in ("amg", "amg_smoothed"):
            self.amg = AmgPlan(n, rowptr, colidx, prolongator="smoothed" if op.precond == "amg_smoothed" else "plain")

    def _refresh(self, val):
        """the preconditioner for these values -> what solve() takes beside them"""
        p = self.op.precond
        if p == "jacobi":
            if self.dinv_from is not None:
                return dict(dinv=self.dinv_from.dinv)
            self.dinv = self.ilu.pivots(val, out=self.dinv).reciprocal_()
            return dict(dinv=self.dinv)
        if p == "ilu0":
            self.lu = self.ilu.factor(val, out=self.lu)
            return dict(lu=self.lu)
        if self.amg is not None:
            self.amg.setup(val)
        return {}

    def _plan(self, s):
        if s not in self.plans:
            op, p = self.op, self.op.precond
            seat = p if p in (None, "jacobi") else self.amg if self.amg is not None else self.ilu if s == 0 else self.ilu.solvers()
            args = (op.n, self.rowptr, self.colidx) + ((s,) if s else ())
            if op.method == "gmres":
                self.plans[s] = (GmresMultiPlan if s else GmresPlan)(*args, restart=op.restart, precond=seat)
            else:
                self.plans[s] = (KrylovMultiPlan if s else KrylovPlan)(*args, method=op.method, precond=seat)
        return self.plans[s]

    def solve(self, val, b, max_iter):
        op = self.op
        plan = self._plan(0 if b.dim() == 1 else int(b.shape[1]))
        return plan.solve(val, b, None, rtol=op.rtol, atol=op.atol, max_iter=max_iter, check_every=op.check_every, **self._refresh(val))

    def destroy(self):
        for p in list(self.plans.values()) + [self.ilu, self.amg]:
            if p is not None:
                p.destroy()
        self.plans, self.ilu, self.amg = {}, None, None


class SolveOperator:
    """x = A(val)^-1 b by a Krylov solve on one n x n CSR structure (int32 rowptr / colidx on the GPU) whose values change
    from call to call, differentiable in val and b:

        op = SolveOperator(n, rowptr, colidx, method="bicgstab", precond="ilu0", rtol=1e-10)
        x = op.solve(val, b)                   # sparse_solve(op, val, b); b: n entries, or n x s row-major, 1 <= s <= 64

    method: "pcg" (A symmetric positive definite), "bicgstab" or "gmres" (restart).  precond: None, "jacobi", "ilu0", "amg"
    or "amg_smoothed" (ILU(0), AMG and Jacobi's diagonal need ascending rows that store their diagonal); "chebyshev" is
    refused.  A 1-D b runs on KrylovPlan / GmresPlan, an (n, s) b on KrylovMultiPlan / GmresMultiPlan, one plan per s, made
    at first use and kept.  The operator owns its preconditioner and refreshes it from val in every forward (Ilu0Plan.factor,
    AmgPlan.setup, or the inverse diagonal).

    Backward solves A^T g = xbar with the same method, preconditioner kind, tolerances and limits (backward_max_iter, when
    set, replaces max_iter there), then bbar = g and valbar[e] = -<g[row(e)], x[col(e)]> on the whole pattern.  With "pcg"
    the adjoint system is the forward's own and reuses its plans.  Otherwise the first backward makes a TransposePlan and,
    on its csc() arrays, a SECOND set of solver plans and a preconditioner of the same kind, so a non-symmetric operator
    holds two sets of plans; Jacobi's inverse diagonal is shared.  A zero xbar, or a zero column of it, gives zeros.

    The gradient is exact only up to kappa(A) * rtol: both solves stop at |r| <= max(rtol |b|, atol), and neither the
    forward's error in x nor the backward's in g is differentiated.  op.last = dict(forward=status, backward=status) keeps
    the plans' status dicts.  strict=True raises SblasError, naming the phase, the status and |r|, when a solve ends other
    than "converged"; strict=False returns what the solve left.  Only the halves autograd asks for are computed; backward
    of backward is not supported.  One call at a time per operator."""

    def __init__(self, n, rowptr, colidx, method="pcg", precond=None, restart=30, rtol=1e-8, atol=0.0, max_iter=1000, check_every=8,
                 strict=True):
        if precond == "chebyshev":
            raise SblasError("SolveOperator: the 'chebyshev' preconditioner is not supported (None, 'jacobi', 'ilu0', 'amg', 'amg_smoothed')")
        if method not in _SOLVE_METHODS:
            raise SblasError("SolveOperator: method must be 'pcg', 'bicgstab' or 'gmres', not %r" % (method,))
        if precond not in _SOLVE_PRECONDS:
            raise SblasError("SolveOperator: precond must be None, 'jacobi', 'ilu0', 'amg' or 'amg_smoothed', not %r" % (precond,))
        for name, t in (("rowptr", rowptr), ("colidx", colidx)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise SblasError("SolveOperator: %s must be a GPU tensor (no CPU path exists)" % name)
        self.n, self.rowptr, self.colidx, self.nnz, self.device = int(n), rowptr, colidx, int(colidx.numel()), rowptr.device
        self.method, self.precond, self.restart = method, precond, int(restart)
        self.rtol, self.atol, self.max_iter, self.check_every, self.strict = float(rtol), float(atol), int(max_iter), int(check_every), bool(strict)
        self.backward_max_iter = None
        self.last = dict(forward=None, backward=None)
        self.forward_side = _SolveSide(self, rowptr, colidx)
        self.adjoint_side = self.forward_side if method == "pcg" else None
        self.transpose_plan = self._csc = None

    def solve(self, val, b):
        """x with A(val) x = b, differentiable in val and b."""
        return sparse_solve(self, val, b)

    def _pattern(self):
        return self.n, self.n, self.rowptr, self.colidx

    def _finish(self, phase, st):
        self.last[phase] = st
        names = st["status"] if isinstance(st["status"], list) else [st["status"]]
        if self.strict and any(s != "converged" for s in names):
            j = [s != "converged" for s in names].index(True)
            rnorm = float(st["rnorm"][j]) if isinstance(st["status"], list) else float(st["rnorm"])
            why = st["breakdown"][j] if isinstance(st["status"], list) else st["breakdown"]
            raise SblasError("sparse_solve: the %s solve ended with status %r (|r| = %g%s%s)"
                             % (phase, names[j], rnorm, ", column %d" % j if len(names) > 1 else "",
                                ", denominator %s" % why if why else ""))

    def _forward(self, val, b):
        x, st = self.forward_side.solve(val, b, self.max_iter)
        self._finish("forward", st)
        return x

    def _adjoint(self, val, dx):
        """g with A(val)^T g = dx"""
        if self.method == "pcg":
            side, val_t = self.forward_side, val
        else:
            if self.transpose_plan is None:
                self.transpose_plan = TransposePlan(self.n, self.n, self.rowptr, self.colidx, val)
                self._csc = self.transpose_plan.csc()[:2]
                self.adjoint_side = _SolveSide(self, self._csc[0], self._csc[1], dinv_from=self.forward_side)
            else:
                self.transpose_plan.update_values(val)
            side, val_t = self.adjoint_side, (_transposed_values(self.transpose_plan) if self.nnz else val)
            if self.precond == "jacobi":
                self.forward_side._refresh(val)          # the shared inverse diagonal, of these values
        g, st = side.solve(val_t, dx, self.max_iter if self.backward_max_iter is None else int(self.backward_max_iter))
        self._finish("backward", st)
        return g

    def destroy(self):
        for p in (self.forward_side, self.adjoint_side if self.adjoint_side is not self.forward_side else None, self.transpose_plan):
            if p is not None:
                p.destroy()
        self.adjoint_side = self.transpose_plan = self._csc = None


class _SparseSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, val, b, op):
        ctx.op = op
        b = b.detach()
        x = op._forward(val.detach().contiguous(), b.contiguous() if b.dim() == 1 else _row_major(b))
        ctx.save_for_backward(val, x)
        return x

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dx):
        val, x = ctx.saved_tensors
        op = ctx.op
        g = op._adjoint(val.detach().contiguous(), _row_major(dx))
        dval = _values_gradient(op._pattern(), g, x, "all", None) if ctx.needs_input_grad[0] else None
        return dval, (g if ctx.needs_input_grad[1] else None), None


def sparse_solve(op, val, b):
    """x with A(val) x = b on a SolveOperator, differentiable in val and b."""
    if not isinstance(op, SolveOperator):
        raise SblasError("sparse_solve needs a SolveOperator")
    _check_solve_args(op.n, op.nnz, val, b, "sparse_solve")
    if b.dim() == 2 and not 1 <= int(b.shape[1]) <= 64:
        raise SblasError("sparse_solve: b must have between 1 and 64 columns, got %d" % b.shape[1])
    return _SparseSolve.apply(val, b, op)
