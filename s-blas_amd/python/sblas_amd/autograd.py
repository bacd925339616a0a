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
Backward of backward is not supported.  float64 values, int32 indices, GPU tensors only: there is no CPU path.
torch is imported here, not by the package."""
import ctypes as C

import torch

from . import (ATTENTION_MAX_WIDTH, ROW_MAJOR, GeamPlan, MaskedSpgemmPlan, SblasError, SpgemmPlan, SpmmPlan, SpmvPlan, TransposePlan, _DeviceArray,
               _layout, check, csr_attention,
               csr_attention_backward, csr_attention_workspace_bytes, csr_softmax, csr_softmax_backward,
               csr_softmax_workspace_bytes, gather, sddmm_tensor, lib, sddmm_workspace_bytes, spmm_tensor, spmm_workspace_bytes)


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
