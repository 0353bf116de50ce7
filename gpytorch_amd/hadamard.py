"""Hadamard multitask GPs on the fused path: ``K[i, j] = k(x_i, x_j) * K_TT[task_i, task_j]``.

Mirrors ``IndexKernel.forward`` (``gpytorch/kernels/index_kernel.py:101-112``: the task covariance looked up at the task index of
every point) and ``covar_x.mul(covar_i)`` in ``test/examples/test_hadamard_multitask_gp_regression.py:33-54``.  The reference
forms the elementwise product of an n x n kernel matrix with an interpolated task matrix; here K is never formed:

    (K o B)[i, :] v  =  sum_tau' K_TT[task_i, tau'] * ( k(x_i, X) (v o 1[task = tau']) )

i.e. ONE fused K*V launch with T * t columns (every right-hand side masked to one task) followed by an O(n T t) gather -- the
same "T*t columns" trick as the Kronecker operator of :mod:`gpytorch_amd.multitask`.  Solves, SLQ log-determinants and Lanczos
decompositions run on it; the A.6 backward is one fused bilinear derivative (T * t masked columns) for the data-kernel
hyper-parameters and one fused K*V for dK_TT.
"""
from __future__ import annotations

import torch

from . import backend as B
from .bbmm import allreduce_grads_, backward_vectors, grouped_matvec64, preconditioner_for_diag, structured_backward_tail, structured_forward
from .functions import KernelSpec, _prep, hyper_grads
from .operators import DiagLinearOperator, FusedKernelLinearOperator, LinearOperator, SolverTerms, StructuredAddedDiagLinearOperator, split_diag


class IndexedTaskCovar(LinearOperator):
    """K_TT[i1, i2]: what ``IndexKernel.forward(i1, i2)`` returns (an ``InterpolatedLinearOperator`` in the reference)."""

    def __init__(self, ktt: torch.Tensor, i1: torch.Tensor, i2: torch.Tensor):
        self.ktt = ktt
        self.i1, self.i2 = i1.reshape(-1).long(), i2.reshape(-1).long()

    dtype = property(lambda self: self.ktt.dtype)
    device = property(lambda self: self.ktt.device)

    def _size(self):
        return torch.Size([self.i1.numel(), self.i2.numel()])

    def to_dense(self):
        return self.ktt[self.i1][:, self.i2]

    def _matmul(self, rhs):
        return self.to_dense() @ rhs

    def _transpose_nonbatch(self):
        return IndexedTaskCovar(self.ktt.mT, self.i2, self.i1)

    def diagonal(self, offset=0, dim1=-2, dim2=-1):
        return self.ktt[self.i1, self.i2]

    def __getitem__(self, index):
        from .operators import _strip_ellipsis

        index = _strip_ellipsis(index)
        r, c = index if isinstance(index, tuple) else (index, slice(None))
        return IndexedTaskCovar(self.ktt, self.i1[r], self.i2[c])

    def detach(self):
        return IndexedTaskCovar(self.ktt.detach(), self.i1, self.i2)

    def mul(self, other):
        if isinstance(other, FusedKernelLinearOperator):
            return HadamardFusedLinearOperator(other, self)
        return super().mul(other)

    __mul__ = mul


def hadamard_matvec(p1, p2, os_, ktt, i1, i2, vt):
    """((os * k(x1, x2)) o K_TT[i1, i2]) @ V for V = vt [t, >= m] probe-major; returns [t, ld_n]."""
    T, t = ktt.shape[-1], vt.shape[0]
    n, m = p1.n, p2.n
    ldm = B.round_up(m, 4)
    mask2 = torch.nn.functional.one_hot(i2, T).t().to(vt.dtype)                    # [T, m]
    w = torch.zeros(t, T, ldm, device=vt.device, dtype=vt.dtype)
    w[:, :, :m] = vt[:, None, :m] * mask2[None]
    q = B.kv(p1, p2, w.reshape(t * T, ldm), scale=os_)                              # [(t T), ld_n]
    bsel = ktt.to(vt.dtype)[i1].t()                                                 # [T, n]: K_TT[task_i, tau']
    out = torch.zeros(t, q.shape[1], device=vt.device, dtype=vt.dtype)
    out[:, :n] = (q[:, :n].reshape(t, T, n) * bsel[None]).sum(1)
    return out


class HadamardFusedLinearOperator(LinearOperator):
    """(outputscale * k(x1, x2)) o K_TT[i1, i2], matrix-free."""

    def __init__(self, kx: FusedKernelLinearOperator, tasks: IndexedTaskCovar):
        if kx.shape != tasks.shape:
            raise RuntimeError(f"data covariance {tuple(kx.shape)} and task covariance {tuple(tasks.shape)} sizes do not match")
        self.kx, self.tasks = kx, tasks

    dtype = property(lambda self: self.kx.dtype)
    device = property(lambda self: self.kx.device)

    @property
    def requires_grad(self):
        return self.kx.requires_grad or self.tasks.ktt.requires_grad

    def _size(self):
        return self.kx._size()

    def _matmul(self, rhs):
        p1, p2 = self.kx.prepared()
        out_t = hadamard_matvec(p1, p2, self.kx._os(), self.tasks.ktt.detach(), self.tasks.i1, self.tasks.i2, B.to_probe_major(rhs.detach(), p1.dtype))
        return B.from_probe_major(out_t, self.shape[0]).to(rhs.dtype)

    def _transpose_nonbatch(self):
        return HadamardFusedLinearOperator(self.kx._transpose_nonbatch(), self.tasks._transpose_nonbatch())

    def _mul_constant(self, c):
        return HadamardFusedLinearOperator(self.kx._mul_constant(c), self.tasks)

    def diagonal(self, offset=0, dim1=-2, dim2=-1):
        return self.kx.diagonal() * self.tasks.diagonal()

    def to_dense(self):
        return self.kx.to_dense() * self.tasks.to_dense().to(self.dtype)

    def __getitem__(self, index):
        a, b = self.kx[index], self.tasks[index]
        if isinstance(a, FusedKernelLinearOperator):
            return HadamardFusedLinearOperator(a, b)
        return a * b.to_dense()

    def detach(self):
        return HadamardFusedLinearOperator(self.kx.detach(), self.tasks.detach())

    def __add__(self, other):
        if isinstance(other, DiagLinearOperator) and self.is_square and not other.batch_shape:
            noise, vec = split_diag(other, self.device, self.dtype)
            return HadamardFusedAddedDiagLinearOperator(self, noise, noise_vec=vec)
        return super().__add__(other)


class HadamardFusedAddedDiagLinearOperator(StructuredAddedDiagLinearOperator):
    """(k o K_TT) + noise I: the operator the MLL and the prediction caches of a Hadamard multitask GP solve with.  The solver takes the whole
    diagonal as ``dvec``; products leave the diagonal off the autograd path."""

    had = property(lambda self: self.inner)

    def _matmul(self, rhs):
        return self.had._matmul(rhs) + self._diag_total().detach().unsqueeze(-1) * rhs

    def _solver_terms(self):
        p1, _ = self.had.kx.prepared()
        os_, ktt, ti = self.had.kx._os(), self.had.tasks.ktt.detach(), self.had.tasks.i1

        def partials(dt):
            out = hadamard_matvec(p1, p1, os_, ktt, ti, ti, dt)
            return out, 1, out.stride(0)

        return SolverTerms(partials, None, None, self._dvec(p1.dtype), p1.dtype)

    def _build_precond(self):
        p1, _ = self.had.kx.prepared()
        return hadamard_preconditioner(p1, self.had.kx._os(), self.had.tasks.ktt, self.had.tasks.i1, self._dvec(p1.dtype))

    def _mll(self, rhs):
        kx = self.had.kx
        nvec = None if self.noise_vec is None else self.noise_vec.detach().to(B.work_dtype(kx.x1))
        return HadamardInvQuadLogdetFn.apply(kx.x1, kx.lengthscale, kx.outputscale, self.had.tasks.ktt, self.noise, rhs, kx.spec,
                                             self.had.tasks.i1, nvec, self.bbmm_opts, kx.spec.param)

    def _matvec64(self):
        """a64 [c, ld] (probe-major, float64) -> ((theta K_XX) o K_TT[i, i] + D) a in float64: ``hadamard_matvec`` on the prepared points widened to
        float64 (the fused float64 product with T x columns, ``csrc/kv_f64.hpp``), groups of at most 80 / T columns."""
        p1, _ = self.had.kx.prepared()
        if not (p1.fused and p1.dp <= B.FUSED_F64_MAX_DP):
            return None
        x64 = B.PreparedPoints(p1.xp.to(torch.float64), p1.n, p1.d, p1.dp, p1.kind, p1.param)
        os_ = self.had.kx._os()
        os64 = None if os_ is None else os_.detach().to(torch.float64)
        ktt, ti = self.had.tasks.ktt.detach().to(torch.float64), self.had.tasks.i1
        return grouped_matvec64(lambda blk: hadamard_matvec(x64, x64, os64, ktt, ti, ti, blk), self._dvec(torch.float64), max(1, 80 // ktt.shape[-1]))


def hadamard_preconditioner(xp, os_, ktt, ti, diag_total, rank=None, tol=None, min_size=None):
    """Pivoted-Cholesky preconditioner of (theta k(x, x)) o K_TT[ti, ti] + diag: row p is the data-kernel row of point p
    (``gpamd_kernel_rows_f32``) times K_TT[task_p, task_.] (the reference preconditions the product operator + diagonal like any other
    ``AddedDiagLinearOperator``: ``kernels/index_kernel.py:101-112`` + ``settings.py:6-31``)."""
    if not xp.fused:
        return None
    ktt_d = ktt.detach().to(xp.dtype)

    def row_fn(p):
        return B.kernel_rows(xp, p, xp, os_).reshape(-1) * ktt_d[ti[p]].reshape(-1)[ti]

    return preconditioner_for_diag(row_fn, B.kernel_diag(xp, xp, os_) * ktt_d[ti, ti], diag_total, rank, tol, min_size)


class HadamardInvQuadLogdetFn(torch.autograd.Function):
    """(inv_quad[c], logdet) of (theta k(x, x)) o K_TT[ti, ti] + noise I (+ diag(noise_vec)) by preconditioned mBCG + SLQ
    (``bbmm.inv_quad_logdet_forward`` on the masked-column product; probe columns shardable over ``opts["group"]``)."""

    @staticmethod
    def forward(ctx, x, lengthscale, outputscale, ktt, noise, rhs, spec: KernelSpec, ti, noise_vec, opts, kparam=None):
        n, T = x.shape[-2], ktt.shape[-1]
        dev = x.device
        xp = _prep(spec, x, lengthscale)
        wd = xp.dtype
        os_ = None if outputscale is None else outputscale.detach().reshape(-1)[:1].to(wd).contiguous()
        ktt_d = ktt.detach().to(wd)
        ld = B.round_up(n, 4)
        dv = torch.zeros(ld, device=dev, dtype=wd)
        dv[:n] = noise.detach().reshape(()).to(wd)
        if noise_vec is not None:
            dv[:n] += noise_vec

        def partials(dt):
            out = hadamard_matvec(xp, xp, os_, ktt_d, ti, ti, dt)
            return out, 1, out.stride(0)

        res, ctx.group, ctx.t_total = structured_forward(opts, B.to_probe_major(rhs, wd), None, None, dv, partials, n,
                                                         lambda: hadamard_preconditioner(xp, os_, ktt_d, ti, dv))
        ctx.xp, ctx.n, ctx.T, ctx.ti, ctx.res = xp, n, T, ti, res
        ctx.kparam = kparam
        ctx.has_os = outputscale is not None
        ctx.save_for_backward(lengthscale, outputscale if outputscale is not None else torch.empty(0), ktt, noise, rhs)
        return res.inv_quad.to(rhs.dtype), res.logdet.to(rhs.dtype)

    @staticmethod
    def backward(ctx, g_iq, g_ld):
        lengthscale, outputscale, ktt, noise, rhs = ctx.saved_tensors
        outputscale = outputscale if ctx.has_os else None
        xp, n, T, ti, res = ctx.xp, ctx.n, ctx.T, ctx.ti, ctx.res
        wd = xp.dtype
        left, right, s_y = backward_vectors(res, g_iq, g_ld, ctx.t_total)
        tc = left.shape[0]
        left, right = left[:, :n], right[:, :n]
        ktt_d = ktt.detach().to(wd)
        mask = torch.nn.functional.one_hot(ti, T).t().to(wd)            # [T, n]
        ld = B.round_up(n, 4)

        def pad(v3):                                                    # [tc, T, n] -> probe-major [(tc T), ld]
            out = torch.zeros(tc * T, ld, device=v3.device, dtype=wd)
            out[:, :n] = v3.reshape(tc * T, n)
            return out

        l_m = left[:, None, :] * mask[None]                             # L_c o 1[task = tau]
        r_b = right[:, None, :] * ktt_d[:, ti][None]                    # R_c[j] * K_TT[tau, task_j]
        kp = ctx.kparam if (ctx.kparam is not None and ctx.needs_input_grad[10]) else None
        out = hyper_grads(xp, xp, lengthscale, outputscale, pad(l_m), pad(r_b), kparam=kp)
        d_ls, d_os = out[:2]
        d_par = out[-1] if kp is not None else None
        # d/dK_TT[tau, tau'] = sum_c (L_c o 1[tau])^T (theta K) (R_c o 1[tau'])
        os_ = None if outputscale is None else outputscale.detach().reshape(-1)[:1].to(wd).contiguous()
        mq = B.kv(xp, xp, pad(right[:, None, :] * mask[None]), scale=os_)[:, :n].reshape(tc, T, n)
        d_ktt = torch.einsum("cti,csi->ts", l_m, mq).to(ktt.dtype)
        d_noise = (left * right).sum().reshape(noise.shape).to(noise.dtype)
        allreduce_grads_([d_ls, d_os, d_ktt, d_noise, d_par], ctx.group)
        d_rhs = structured_backward_tail(left, right, s_y, n, g_iq, rhs, ctx.needs_input_grad[5])[2]
        return None, d_ls, d_os, d_ktt, d_noise, d_rhs, None, None, None, None, d_par
