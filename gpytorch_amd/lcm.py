"""The linear model of coregionalisation, K = sum_q theta_q K_q(X, X') (x) B_q: exact multi-output GPs whose Q latent processes have families and
lengthscales of their own (``gpytorch/kernels/lcm_kernel.py:14-75``: one ``MultitaskKernel`` per base kernel, summed).

A sum of Kronecker products has no per-factor eigen-structure, so the nT x nT system is solved by mBCG over the product
    (sum_q theta_q K_q (x) B_q) V = sum_q K_q (V_mat (theta_q B_q)^T),
which is ONE fused kernel over all members on an interleaved right-hand side (``csrc/kv_lcm.hpp``, ``backend.LcmPlan``) where the reference forms Q dense
n x n matrices.  The backward runs once per evaluation and uses the single-family kernels, Q times.  Layout: row = i*T + tau, as in :mod:`.multitask`.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import backend as B
from .bbmm import allreduce_grads_, backward_vectors, preconditioner_for_diag, structured_backward_tail, structured_forward
from .functions import hyper_grads
from .kernels import Kernel, MaternKernel, RBFKernel, ScaleKernel, stationary_dense
from .multitask import MultitaskKernel, TaskNoiseDiagLinearOperator
from .operators import LinearOperator, SolverTerms, StructuredAddedDiagLinearOperator


class LCMMember(NamedTuple):
    """One latent process: family name, lengthscale ([1, 1] or [1, d]), outputscale (a ``ScaleKernel``'s, or None) and task covariance B_q [T, T]."""

    kind: str
    lengthscale: torch.Tensor
    outputscale: object
    task_covar: torch.Tensor

    def scaled_task_covar(self):
        return self.task_covar if self.outputscale is None else self.task_covar * self.outputscale.reshape(())

    def os_(self):
        return None if self.outputscale is None else self.outputscale.detach().reshape(-1)[:1].to(torch.float32).contiguous()

    def detach(self):
        return LCMMember(self.kind, self.lengthscale.detach(), None if self.outputscale is None else self.outputscale.detach(), self.task_covar.detach())


def _member_points(members, x, shift):
    return [B.prep_points(mb.kind, x, mb.lengthscale, shift) for mb in members]


def _block(members, d):
    return B.lcm_block([mb.kind for mb in members], [mb.lengthscale for mb in members], [mb.scaled_task_covar() for mb in members], d)


def lcm_dense_members(members, x1, x2, shift=None):
    """sum_q kron(theta_q k_q(x1, x2), B_q) in autograd-visible torch ops, interleaved rows i*T + tau (any dtype and device)."""
    out = 0
    for mb in members:
        z1, z2 = x1 / mb.lengthscale, x2 / mb.lengthscale
        kq = stationary_dense(mb.kind, (z1.unsqueeze(-2) - z2.unsqueeze(-3)).pow(2).sum(-1))
        out = out + torch.kron(kq, mb.scaled_task_covar().to(kq.dtype))
    return out


class LCMFusedLinearOperator(LinearOperator):
    """sum_q theta_q K_q(x1, x2) (x) B_q, matrix-free: every product is one launch of the fused multi-member kernel."""

    def __init__(self, x1, x2, shift, members):
        self.x1, self.x2, self.shift, self.members = x1, x2, shift, tuple(members)
        self.T = members[0].task_covar.shape[-1]
        self._cache = {}

    dtype = property(lambda self: self.x1.dtype)
    device = property(lambda self: self.x1.device)

    @property
    def requires_grad(self):
        return any(t is not None and t.requires_grad for mb in self.members for t in (mb.lengthscale, mb.outputscale, mb.task_covar))

    def _size(self):
        return torch.Size([self.x1.shape[-2] * self.T, self.x2.shape[-2] * self.T])

    @property
    def _same(self):
        """x1 and x2 are the same points: identical storage, or -- compared once, on first use, and cached -- identical values."""
        if "same" not in self._cache:
            x1, x2 = self.x1, self.x2
            self._cache["same"] = x1 is x2 or (x1.shape == x2.shape and (x1.data_ptr() == x2.data_ptr() or bool(torch.equal(x1, x2))))
        return self._cache["same"]

    def clouds(self):
        """(x1c, x2c, block): the centred unscaled clouds and the device parameter block of the fused product."""
        if "clouds" not in self._cache:
            x1c = B.lcm_points(self.x1, self.shift)
            self._cache["clouds"] = (x1c, x1c if self._same else B.lcm_points(self.x2, self.shift), _block(self.members, self.x1.shape[-1]))
        return self._cache["clouds"]

    def prepared(self):
        """Per member, the single-family prepared clouds (rows, diagonals, dense blocks, the backward)."""
        if "prep" not in self._cache:
            p1 = _member_points(self.members, self.x1, self.shift)
            self._cache["prep"] = (p1, p1 if self._same else _member_points(self.members, self.x2, self.shift))
        return self._cache["prep"]

    def plan(self, probes):
        x1c, x2c, block = self.clouds()
        return B.LcmPlan(x1c, x2c, block, self.x1.shape[-1], self.T, probes)

    def _matmul(self, rhs):
        vt = B.to_probe_major(rhs, torch.float32)
        return B.from_probe_major(self.plan(vt.shape[0]).product(vt), self.shape[0]).to(rhs.dtype)

    def _transpose_nonbatch(self):
        return LCMFusedLinearOperator(self.x2, self.x1, self.shift, [mb._replace(task_covar=mb.task_covar.mT) for mb in self.members])

    def diagonal(self, offset=0, dim1=-2, dim2=-1):
        p1, p2 = self.prepared()
        out = 0
        for mb, a, b in zip(self.members, p1, p2):
            out = out + (B.kernel_diag(a, b, mb.os_()).reshape(-1, 1) * mb.task_covar.detach().diagonal().reshape(1, -1)).reshape(-1)
        return out.to(self.dtype)

    def to_dense(self):
        p1, p2 = self.prepared()
        out = 0
        for mb, a, b in zip(self.members, p1, p2):
            out = out + torch.kron(B.kernel_dense(a, b, mb.os_()), mb.task_covar.detach().to(torch.float32))
        return out.to(self.dtype)

    def _row(self, p):
        return lcm_row(*self.prepared(), self.members, p).to(self.dtype)

    def __getitem__(self, index):
        if isinstance(index, tuple) and len(index) == 3 and index[0] is Ellipsis:
            index = index[1:]
        r, c = index if isinstance(index, tuple) else (index, slice(None))
        T = self.T

        def data_slice(sl, n):
            a, b, step = sl.indices(n * T)
            if step != 1 or a % T or b % T:
                raise NotImplementedError("LCM operator slices must be aligned to whole data points")
            return slice(a // T, b // T)

        if isinstance(r, slice) and isinstance(c, slice):
            x1 = self.x1[data_slice(r, self.x1.shape[-2])]
            x2 = x1 if (self.x2 is self.x1 and r == c) else self.x2[data_slice(c, self.x2.shape[-2])]
            return LCMFusedLinearOperator(x1, x2, self.shift, self.members)
        return self.to_dense()[index]

    def __add__(self, other):
        if isinstance(other, TaskNoiseDiagLinearOperator) and self.is_square:
            return LCMFusedAddedDiagLinearOperator(self, other.task_noise)
        return super().__add__(other)

    def detach(self):
        x1 = self.x1.detach()
        return LCMFusedLinearOperator(x1, x1 if self.x2 is self.x1 else self.x2.detach(), self.shift, [mb.detach() for mb in self.members])


def lcm_row(preps1, preps2, members, p):
    """Row p = i*T + tau of sum_q theta_q K_q (x) B_q: sum_q theta_q k_q(x_i, .) (x) B_q[tau, :], one ``gpamd_kernel_rows_f32`` row per member."""
    T, m = members[0].task_covar.shape[-1], preps2[0].n
    p = torch.as_tensor(p, device=preps1[0].xp.device).reshape(1)
    i, tau = torch.div(p, T, rounding_mode="floor"), p % T
    return sum((B.kernel_rows(a, i, b, mb.os_()).reshape(m, 1) * mb.task_covar.detach().to(torch.float32)[tau].reshape(1, T)).reshape(-1)
               for a, b, mb in zip(preps1, preps2, members))


def lcm_preconditioner(preps, members, diag_total, rank=None, tol=None, min_size=None):
    """Pivoted-Cholesky preconditioner of sum_q theta_q K_q (x) B_q + diag(diag_total), built from rows (``lcm_row``) and the diagonal on the per-member
    prepared clouds (the pattern of ``multitask.kron_preconditioner``)."""
    n, T = preps[0].n, members[0].task_covar.shape[-1]
    kdiag = sum((B.kernel_diag(xp, xp, mb.os_()).reshape(n, 1) * mb.task_covar.detach().to(torch.float32).diagonal().reshape(1, T)).reshape(-1)
                for xp, mb in zip(preps, members))
    return preconditioner_for_diag(lambda p: lcm_row(preps, preps, members, p), kdiag, diag_total, rank, tol, min_size)


class LCMFusedAddedDiagLinearOperator(StructuredAddedDiagLinearOperator):
    """sum_q theta_q K_q (x) B_q + I_n (x) diag(task_noise) (+ diag(noise_vec)): solved by mBCG over the fused multi-member product.  As in the
    Kronecker operator the base's scalar noise is zero: the per-task noise takes its place, and the solver takes the whole diagonal as ``dvec``."""

    def __init__(self, inner: LCMFusedLinearOperator, task_noise: torch.Tensor, bbmm_opts=None, noise_vec=None):
        super().__init__(inner, torch.zeros(1, device=inner.device, dtype=inner.dtype), noise_vec, bbmm_opts)
        self.task_noise = task_noise

    @property
    def requires_grad(self):
        return super().requires_grad or self.task_noise.requires_grad

    def _diag_total(self):
        d = self.task_noise.repeat(self.inner.x1.shape[-2])
        return d if self.noise_vec is None else d + self.noise_vec

    def _matmul(self, rhs):
        return self.inner._matmul(rhs) + self._diag_total().detach().unsqueeze(-1) * rhs

    def detach(self):
        return LCMFusedAddedDiagLinearOperator(self.inner.detach(), self.task_noise.detach(), self.bbmm_opts,
                                               None if self.noise_vec is None else self.noise_vec.detach())

    def _add_diag(self, noise, vec):
        nv = self.noise_vec if vec is None else (vec if self.noise_vec is None else self.noise_vec + vec)
        return LCMFusedAddedDiagLinearOperator(self.inner, self.task_noise + noise, self.bbmm_opts, nv)

    def __add__(self, other):
        if isinstance(other, TaskNoiseDiagLinearOperator):
            return LCMFusedAddedDiagLinearOperator(self.inner, self.task_noise + other.task_noise, self.bbmm_opts, self.noise_vec)
        return super().__add__(other)

    def _solver_terms(self):
        plans = {}

        def partials(dt):
            if dt.shape[0] not in plans:
                plans[dt.shape[0]] = self.inner.plan(dt.shape[0])
            return plans[dt.shape[0]](dt)

        return SolverTerms(partials, None, None, self._dvec(torch.float32), torch.float32, self.bbmm_opts.get("group"))

    def _build_precond(self):
        return lcm_preconditioner(self.inner.prepared()[0], self.inner.members, self._diag_total())

    def _mll(self, rhs):
        op = self.inner
        flat = [t for mb in op.members for t in (mb.lengthscale, mb.outputscale, mb.task_covar)]
        return LCMInvQuadLogdetFn.apply(op.x1, op.shift, tuple(mb.kind for mb in op.members), self.bbmm_opts, self.noise_vec, self.task_noise, rhs, *flat)

    def _dense64(self, differentiable=True):
        return (self.to_dense_differentiable() if differentiable else self.to_dense()).to(torch.float64)

    def to_dense_differentiable(self):
        """Small-n Cholesky branch: dense K_hat built with autograd-visible torch ops on the device."""
        op = self.inner
        return lcm_dense_members(op.members, op.x1, op.x1) + torch.diag(self._diag_total())


class LCMInvQuadLogdetFn(torch.autograd.Function):
    """inv_quad / log-det of sum_q theta_q K_q (x) B_q + I (x) diag(task_noise) by preconditioned mBCG + SLQ over the fused multi-member product; the
    backward per member on the single-family kernels: ``hyper_grads`` with (L, R B_q^T) for its lengthscale and outputscale, one ``B.kv`` for
    dB_q = sum L_mat^T (theta_q K_q R_mat).  ``flat`` = (lengthscale, outputscale or None, B_q) per member."""

    @staticmethod
    def forward(ctx, x, shift, kinds, opts, noise_vec, task_noise, rhs, *flat):
        members = [LCMMember(k, flat[3 * q], flat[3 * q + 1], flat[3 * q + 2]) for q, k in enumerate(kinds)]
        n, d = x.shape[-2:]
        T = members[0].task_covar.shape[-1]
        N = n * T
        preps = _member_points(members, x, shift)
        xc = B.lcm_points(x, shift)
        block = _block(members, d)
        dv = torch.zeros(B.round_up(N, 4), device=x.device, dtype=torch.float32)
        dv[:N] = task_noise.detach().to(torch.float32).repeat(n)
        if noise_vec is not None:
            dv[:N] += noise_vec.detach().to(torch.float32)
        plans = {}

        def partials(dt):
            if dt.shape[0] not in plans:
                plans[dt.shape[0]] = B.LcmPlan(xc, xc, block, d, T, dt.shape[0])
            return plans[dt.shape[0]](dt)

        res, ctx.group, ctx.t_total = structured_forward(opts, B.to_probe_major(rhs, torch.float32), None, None, dv, partials, N,
                                                         lambda: lcm_preconditioner(preps, members, dv))
        ctx.preps, ctx.kinds, ctx.n, ctx.T, ctx.res = preps, kinds, n, T, res
        ctx.vec = noise_vec if (noise_vec is not None and ctx.needs_input_grad[4]) else None
        ctx.has_os = [mb.outputscale is not None for mb in members]
        ctx.save_for_backward(task_noise, rhs, *[t if t is not None else torch.empty(0) for t in flat])
        return res.inv_quad.to(rhs.dtype), res.logdet.to(rhs.dtype)

    @staticmethod
    def backward(ctx, g_iq, g_ld):
        task_noise, rhs, *flat = ctx.saved_tensors
        n, T, res = ctx.n, ctx.T, ctx.res
        N = n * T
        left, right, s_y = backward_vectors(res, g_iq, g_ld, ctx.t_total)
        tc = left.shape[0]
        l3 = left[:, :N].reshape(tc, n, T).permute(0, 2, 1).contiguous()   # [tc, T, n]
        r3 = right[:, :N].reshape(tc, n, T).permute(0, 2, 1).contiguous()
        ld_n = B.round_up(n, 4)

        def pad(v3):
            out = torch.zeros(tc * T, ld_n, device=v3.device, dtype=torch.float32)
            out[:, :n] = v3.reshape(tc * T, n)
            return out

        lp, rp = pad(l3), pad(r3)
        grads = []
        for q, xp in enumerate(ctx.preps):
            ls, os_, bq = flat[3 * q], (flat[3 * q + 1] if ctx.has_os[q] else None), flat[3 * q + 2]
            r3b = torch.einsum("ab,cbn->can", bq.detach().to(torch.float32), r3)
            d_ls, d_os = hyper_grads(xp, xp, ls, os_, lp, pad(r3b))[:2]
            osq = None if os_ is None else os_.detach().reshape(-1)[:1].to(torch.float32).contiguous()
            m3 = B.kv(xp, xp, rp, scale=osq)[:, :n].reshape(tc, T, n)
            grads += [d_ls, d_os, torch.einsum("ctn,csn->ts", l3, m3).to(bq.dtype)]
        d_noise = (l3 * r3).sum(dim=(0, 2)).to(task_noise.dtype)
        _, d_vec, d_rhs = structured_backward_tail(left, right, s_y, N, g_iq, rhs, ctx.needs_input_grad[6], noise_vec=ctx.vec)
        allreduce_grads_(grads + [d_noise, d_vec], ctx.group)
        return (None, None, None, None, d_vec, d_noise, d_rhs, *grads)


# ------------------------------------------------------------------------------------------------ the kernel module
def _lcm_member_kernels(kernel):
    """Per member (base, ScaleKernel or None) with the base exactly an ``RBFKernel`` / ``MaternKernel``, bare or inside ONE unbatched ``ScaleKernel``,
    without ``active_dims``; None where any member is something else."""
    found = []
    for mt in kernel.covar_module_list:
        base, scale = mt.data_covar_module, None
        if type(base) is ScaleKernel:
            if len(base.batch_shape):
                return None
            base, scale = base.base_kernel, base
        if type(base) not in (RBFKernel, MaternKernel) or len(base.batch_shape) or base.active_dims is not None:
            return None
        found.append((base, scale))
    return found


def lcm_native(kernel, x1, x2=None, last_dim_is_batch=False) -> bool:
    """The fused multi-member form applies to this call of an ``LCMKernel``.  Pure: it looks at the kernel's structure and at the shapes and dtypes of
    the inputs, never at the device.  All of: float32 inputs and parameters, no batch; 1 <= d <= 4, 1 <= Q <= 4, 2 <= T <= 8; every base an
    ``RBFKernel`` or ``MaternKernel`` with one or d lengthscales, bare or inside one ``ScaleKernel``, over the whole input (no ``active_dims``); inputs
    without ``requires_grad``.  Everything else takes ``lcm_dense``."""
    x2 = x1 if x2 is None else x2
    if last_dim_is_batch or x1.dim() != 2 or x2.dim() != 2 or x1.dtype != torch.float32 or x2.dtype != torch.float32:
        return False
    if x1.requires_grad or x2.requires_grad:
        return False
    d, Q, T = x1.shape[-1], len(kernel.covar_module_list), kernel.covar_module_list[0].num_tasks
    if not (1 <= d <= B.LCM_MAX_DIM and x2.shape[-1] == d and 1 <= Q <= B.LCM_MAX_MEMBERS and B.LCM_MIN_TASKS <= T <= B.LCM_MAX_TASKS):
        return False
    found = _lcm_member_kernels(kernel)
    if found is None:
        return False
    for (base, _), mt in zip(found, kernel.covar_module_list):
        if base.raw_lengthscale.dtype != torch.float32 or mt.task_covar_module.covar_factor.dtype != torch.float32:
            return False
        if tuple(base.raw_lengthscale.shape) not in ((1, 1), (1, d)):
            return False
    return True


def _members_of(kernel, found):
    return [LCMMember(base.kind, base.lengthscale, None if scale is None else scale.outputscale, mt.task_covar_module.covar_matrix)
            for (base, scale), mt in zip(found, kernel.covar_module_list)]


def lcm_dense(kernel, x1, x2, diag=False, **params):
    """sum_q kron(K_q, B_q) in autograd-visible torch ops (any dtype and device; batches broadcast); members other than RBF / Matern through their own
    kernel's dense form."""
    from .operators import to_dense

    found = _lcm_member_kernels(kernel)
    if found is not None and not params.get("last_dim_is_batch", False):   # RBF / Matern members: plain torch, on any device
        out = lcm_dense_members(_members_of(kernel, found), x1, x2)
        return out.diagonal(dim1=-2, dim2=-1) if diag else out
    out = 0
    for mt in kernel.covar_module_list:
        kq = to_dense(mt.data_covar_module(x1, x2, **params))
        out = out + torch.kron(kq, mt.task_covar_module.covar_matrix.to(kq.dtype))
    return out.diagonal(dim1=-2, dim2=-1) if diag else out


class LCMKernel(Kernel):
    """``gpytorch/kernels/lcm_kernel.py:14-75``: one :class:`MultitaskKernel` per base kernel, summed.  Native inputs (:func:`lcm_native`) return ONE
    :class:`LCMFusedLinearOperator`; everything else the dense sum :func:`lcm_dense`."""

    def __init__(self, base_kernels, num_tasks, rank=1, task_covar_prior=None):
        if len(base_kernels) < 1:
            raise ValueError("At least one base kernel must be provided.")
        for k in base_kernels:
            if not isinstance(k, Kernel):
                raise ValueError("base_kernels must only contain Kernel objects")
        if not isinstance(rank, list):
            rank = [rank] * len(base_kernels)
        super().__init__()
        self.covar_module_list = torch.nn.ModuleList(
            [MultitaskKernel(base, num_tasks=num_tasks, rank=r, task_covar_prior=task_covar_prior) for base, r in zip(base_kernels, rank, strict=True)])

    def __call__(self, x1, x2=None, diag=False, **params):
        return self.forward(x1, x2, diag=diag, **params)

    def forward(self, x1, x2, diag=False, **params):
        x1 = x1.unsqueeze(1) if x1.dim() == 1 else x1
        x2 = x1 if x2 is None else (x2.unsqueeze(1) if x2.dim() == 1 else x2)
        if x1.device.type == "cuda" and lcm_native(self, x1, x2, params.get("last_dim_is_batch", False)):
            res = LCMFusedLinearOperator(x1, x2, x1.detach().mean(dim=-2), _members_of(self, _lcm_member_kernels(self)))
            return res.diagonal() if diag else res
        from .operators import to_linear_operator

        res = lcm_dense(self, x1, x2, diag=diag, **params)
        return res if diag else to_linear_operator(res)

    def num_outputs_per_input(self, x1, x2):
        return self.covar_module_list[0].num_outputs_per_input(x1, x2)
