"""Sums of fused kernel operators: ``AdditiveKernel`` (``gpytorch/kernels/kernel.py:592-632``) on the matrix-free path.

``K = sum_i theta_i k_i(x, x)`` stays a list of :class:`~gpytorch_amd.operators.FusedKernelLinearOperator` members; products,
mBCG solves, SLQ log-determinants and Lanczos decompositions use the members' fused K*V launches summed per product (the
``kv_partials`` hook of :func:`gpytorch_amd.linear_cg.linear_cg`), and the A.6 backward runs one fused bilinear derivative per
member.  Preconditioner: pivoted Cholesky on rows of the SUMMED kernel (``sum_preconditioner``; ``bbmm.pivoted_cholesky_rows``).
"""
from __future__ import annotations

import torch

from . import backend as B
from .bbmm import (allreduce_grads_, backward_vectors, build_preconditioner_rows, preconditioner_for_diag, structured_backward_tail,
                   structured_forward)
from .functions import _prep, hyper_grads
from .operators import (
    DiagLinearOperator,
    FusedKernelLinearOperator,
    LinearOperator,
    SolverTerms,
    StructuredAddedDiagLinearOperator,
    ZeroLinearOperator,
    split_diag,
)


class SumFusedLinearOperator(LinearOperator):
    """sum_i members[i], every member a (scaled) fused kernel operator over the same pair of point clouds."""

    def __init__(self, ops):
        self.ops = list(ops)

    @classmethod
    def of(cls, terms):
        flat = []
        for t in terms:
            flat.extend(t.ops if isinstance(t, SumFusedLinearOperator) else [t])
        if len(flat) == 1:
            return flat[0]
        if not all(isinstance(t, FusedKernelLinearOperator) for t in flat):
            from .operators import SumLinearOperator

            return SumLinearOperator(*flat)  # generic (dense-capable) sum
        return cls(flat)

    dtype = property(lambda self: self.ops[0].dtype)
    device = property(lambda self: self.ops[0].device)

    @property
    def requires_grad(self):
        return any(o.requires_grad for o in self.ops)

    def _size(self):
        return self.ops[0].shape

    def _matmul(self, rhs):
        out = self.ops[0]._matmul(rhs)
        for o in self.ops[1:]:
            out = out + o._matmul(rhs)
        return out

    def _transpose_nonbatch(self):
        return SumFusedLinearOperator([o._transpose_nonbatch() for o in self.ops])

    def _mul_constant(self, c):
        return SumFusedLinearOperator([o._mul_constant(c) for o in self.ops])

    def to_dense(self):
        return sum((o.to_dense() for o in self.ops[1:]), self.ops[0].to_dense())

    def diagonal(self, offset=0, dim1=-2, dim2=-1):
        return sum((o.diagonal() for o in self.ops[1:]), self.ops[0].diagonal())

    def __getitem__(self, index):
        parts = [o[index] for o in self.ops]
        if all(isinstance(p, FusedKernelLinearOperator) for p in parts):
            return SumFusedLinearOperator(parts)
        return sum(parts[1:], parts[0])

    def detach(self):
        return SumFusedLinearOperator([o.detach() for o in self.ops])

    def __add__(self, other):
        if isinstance(other, ZeroLinearOperator):
            return self
        if isinstance(other, (FusedKernelLinearOperator, SumFusedLinearOperator)):
            return SumFusedLinearOperator.of([self, other])
        if isinstance(other, DiagLinearOperator) and self.is_square and not other.batch_shape:
            noise, vec = split_diag(other, self.device, self.dtype)
            return SumFusedAddedDiagLinearOperator(self, noise, noise_vec=vec)
        return super().__add__(other)

    __radd__ = __add__


def _sum_partials(prepared):
    """The ``kv_partials`` product of a sum: the members' fused K*V launches (each scaled by its own outputscale), added up."""

    def partials(dt):
        out = None
        for xp, os_ in prepared:
            q = B.kv(xp, xp, dt, scale=os_)
            out = q.clone() if out is None else out.add_(q)
        return out, 1, out.stride(0)

    return partials


class SumFusedAddedDiagLinearOperator(StructuredAddedDiagLinearOperator):
    """(sum_i theta_i k_i(x, x)) + noise I (+ diag(noise_vec)): the operator the MLL and the prediction caches solve with.  The solver takes the
    scalar noise as ``sigma2`` and the fixed per-point vector, where there is one, as ``dvec``."""

    kernel_sum = property(lambda self: self.inner)

    def restrict(self, idx):
        nv = None if self.noise_vec is None else self.noise_vec[idx]
        return SumFusedAddedDiagLinearOperator(self.kernel_sum[idx, idx], self.noise, nv, self.bbmm_opts)

    def _prepared(self):
        return [(o.prepared()[0], o._os()) for o in self.kernel_sum.ops]

    def _vec(self, wd):
        return None if self.noise_vec is None else self._dvec(wd, self.noise_vec)

    def _solver_terms(self):
        prepared = self._prepared()
        wd = prepared[0][0].dtype
        return SolverTerms(_sum_partials(prepared), None, self.noise.detach().reshape(-1)[:1].to(wd).contiguous(), self._vec(wd), wd)

    def _build_precond(self):
        _, _, nz, dv, _, _ = self._solver_terms()
        return sum_preconditioner(self._prepared(), nz, dv, self.shape[-1])

    def _mll(self, rhs):
        flat = []
        empty = torch.empty(0, device=self.device)
        for o in self.kernel_sum.ops:
            flat += [o.x1, o.lengthscale, o.outputscale if o.outputscale is not None else empty,
                     o.spec.param if o.spec.param is not None else empty]
        specs = [o.spec for o in self.kernel_sum.ops]
        return SumInvQuadLogdetFn.apply(self.noise, rhs, specs, self._vec(B.work_dtype(self.kernel_sum.ops[0].x1)), self.bbmm_opts, *flat)

    def _matvec64(self):
        """a64 [c, ld] (probe-major, float64) -> (sum_i theta_i K_i + sigma^2 I + D) a in float64: one fused float64 product per member
        (``bbmm.matvec64``), the diagonal once.  None unless every member has a fused float64 product."""
        from .bbmm import matvec64

        prepared = self._prepared()
        if not all(B.f64_widenable(xp) for xp, _ in prepared):
            return None
        mvs = [matvec64(xp, os_, None) for xp, os_ in prepared]
        nz = self.noise.detach().reshape(()).to(torch.float64)
        dv = self._vec(torch.float64)

        def mv(a64):
            out = mvs[0](a64)
            for m_ in mvs[1:]:
                out = out + m_(a64)
            out = out + nz * a64
            return out if dv is None else out + dv.unsqueeze(0) * a64

        return mv


def sum_preconditioner(prepared, noise, dvec, n, rank=None, tol=None, min_size=None):
    """Pivoted-Cholesky preconditioner of (sum_i theta_i k_i) + noise I (+ diag(dvec)): a row of the sum is the sum of the members'
    ``gpamd_kernel_rows_f32`` rows (the reference preconditions a SumLinearOperator + diagonal the same way, through its generic
    ``pivoted_cholesky``; ``gpytorch/kernels/kernel.py:592-632`` + ``settings.py:6-31``)."""
    if not all(xp.fused for xp, _ in prepared):
        return None
    wd = prepared[0][0].dtype

    def row_fn(p):
        out = None
        for xp, os_ in prepared:
            r = B.kernel_rows(xp, p, xp, os_).reshape(-1)
            out = r if out is None else out + r
        return out

    kdiag = None
    for xp, os_ in prepared:
        dg = B.kernel_diag(xp, xp, os_)
        kdiag = dg if kdiag is None else kdiag + dg
    nz = noise.detach().reshape(-1)[:1].to(wd)
    if dvec is None:
        return build_preconditioner_rows(row_fn, kdiag, nz, False, rank, tol, min_size)
    return preconditioner_for_diag(row_fn, kdiag, nz + dvec[:n].to(wd), rank, tol, min_size)


class SumInvQuadLogdetFn(torch.autograd.Function):
    """(inv_quad[c], logdet) of sum_i theta_i k_i(x_i, x_i) + noise I by preconditioned mBCG + SLQ (``bbmm.inv_quad_logdet_forward`` on the
    summed product; probe columns shardable over ``opts["group"]``); backward: one fused bilinear derivative per member with the shared
    left / right vectors of A.6.  ``flat``: (x, lengthscale, outputscale-or-empty, shape-parameter-or-empty) per member -- RQ members
    carry their alpha as an explicit argument all the way into the kernels (C ABI version 2), so two RQ members with different alpha
    interleave freely."""

    @staticmethod
    def forward(ctx, noise, rhs, specs, dvec, opts, *flat):
        nm = len(specs)
        members = [(flat[4 * i], flat[4 * i + 1], flat[4 * i + 2] if flat[4 * i + 2].numel() else None,
                    flat[4 * i + 3] if flat[4 * i + 3].numel() else None) for i in range(nm)]
        n = members[0][0].shape[-2]
        prepared = []
        for (x, ls, os_, _), spec in zip(members, specs):
            xp = _prep(spec, x, ls)
            prepared.append((xp, None if os_ is None else os_.detach().reshape(-1)[:1].to(xp.dtype).contiguous()))
        wd = prepared[0][0].dtype
        nz = noise.detach().reshape(-1)[:1].to(wd).contiguous()
        res, ctx.group, ctx.t_total = structured_forward(opts, B.to_probe_major(rhs, wd), None, nz, dvec, _sum_partials(prepared), n,
                                                         lambda: sum_preconditioner(prepared, nz, dvec, n))
        ctx.prepared, ctx.n, ctx.res = prepared, n, res
        ctx.members = members
        ctx.save_for_backward(noise, rhs)
        return res.inv_quad.to(rhs.dtype), res.logdet.to(rhs.dtype)

    @staticmethod
    def backward(ctx, g_iq, g_ld):
        noise, rhs = ctx.saved_tensors
        n, res = ctx.n, ctx.res
        left, right, s_y = backward_vectors(res, g_iq, g_ld, ctx.t_total)
        grads = []
        for i, ((x, ls, os_, kpar), (xp, _)) in enumerate(zip(ctx.members, ctx.prepared)):
            need_x = ctx.needs_input_grad[5 + 4 * i]
            kp = kpar if (kpar is not None and ctx.needs_input_grad[5 + 4 * i + 3]) else None
            out = hyper_grads(xp, xp, ls, os_, left, right, want_x1=need_x, want_x2=need_x, kparam=kp)
            d_ls, d_os = out[:2]
            d_x = (out[2] + out[3]).to(x.dtype) if need_x else None
            d_par = out[-1] if kp is not None else None
            grads += [d_x, d_ls if ls.requires_grad else None, d_os, d_par]
        d_noise, _, d_rhs = structured_backward_tail(left, right, s_y, n, g_iq, rhs, ctx.needs_input_grad[1], noise=noise)
        allreduce_grads_([d_noise] + grads, ctx.group)
        return (d_noise, d_rhs, None, None, None, *grads)
