"""Exact GPs that observe gradients, matrix-free: the RBF and the Matern-5/2 kernel over function values AND partial derivatives.

Mirrors ``gpytorch/kernels/rbf_kernel_grad.py:60-104`` (the n (d + 1) x m (d + 1) matrix [[K, dK/dx2], [dK/dx1, d2K/dx1 dx2]], put into the
multitask ordering by a perfect shuffle: row i (d + 1) + a is component a of point i, a = 0 the value, a = 1..d the partial derivatives).  The
reference materialises that matrix; here every entry is k = exp(-|delta|^2 / 2) times a polynomial of degree <= 2 in delta = (x_i - x_j) / l, so
the whole (d + 1) x (d + 1) block of a pair costs one covariance evaluation inside ONE fused launch (``csrc/kv_rbfgrad.hpp``) and is never stored:

    q_ij   = r_j0 + delta . r~_j                      (r~_b = r_b / l_b)
    out_i0 = sum_j k q_ij
    out_ia = (1 / l_a) sum_j k (r~_ja - delta_a q_ij)

Solves, SLQ log-determinants and Lanczos decompositions run on it through the ``kv_partials`` hook of the mBCG driver; the A.6 backward is one fused
bilinear derivative (``kv_grad_rbfgrad_kernel``: 1 + d sums for the outputscale and the lengthscales).  ``rbfgrad_dense`` is the same formula as an
autograd-visible torch expression: float64 models, batches, d > 4, input gradients and the small Cholesky branch take it.

The Matern-5/2 family (``gpytorch/kernels/matern52_kernel_grad.py:102-196``) is the same operator with three radial factors in place of the one k:
with rho = |delta|^2, s = sqrt(5 rho), e = exp(-s):  k = (1 + s + s^2 / 3) e,  g = (5/3) (1 + s) e = -2 dk/drho,  w = (25/3) e = -2 dg/drho, and

    K[i0, j0] = k    K[i0, jb] = g delta_b / l_b    K[ia, j0] = -g delta_a / l_a    K[ia, jb] = (g [a = b] - w delta_a delta_b) / (l_a l_b)
    out_i0 = sum_j [ k r_j0 + g B ],   out_ia = (1 / l_a) sum_j [ g r~_ja - delta_a (g r_j0 + w B) ],   B = delta . r~_j

(RBF: k = g = w).  Every class and function here carries a ``family`` ("rbf" | "matern52": the covariance family whose prepared points the kernels
read); ``RBFGradFusedLinearOperator`` / ``Matern52GradFusedLinearOperator`` fix it, ``matern52grad_dense`` is the Matern twin of ``rbfgrad_dense``.

Second derivatives (``gpytorch/kernels/rbf_kernel_gradgrad.py:60-166``, RBF only) are the same operator at ``order = 2``: C = 2 d + 1 components per
point -- the value, d/dx_a, then d2/dx_a^2 -- and with u = delta, derivative orders alpha, beta in {0, e_a, 2 e_a} and Hermite polynomials He_n

    K[(i, alpha), (j, beta)] = k prod_q (-1)^{alpha_q} He_{alpha_q + beta_q}(u_q) / l_q^{alpha_q + beta_q}

(``csrc/kv_rbfgradgrad.hpp``; ``rbfgradgrad_dense`` the dense form, rectangular inputs included -- the reference's ``forward`` fails for n1 != n2;
``RBFGradGradFusedLinearOperator`` the operator).  The prepared points are the RBF family's, so the order travels with the operator class, not with
the points: every backend call passes ``order``.
"""
from __future__ import annotations

import torch

from . import backend as B
from .bbmm import allreduce_grads_, backward_vectors, preconditioner_for_diag, structured_backward_tail, structured_forward
from .functions import rbfgrad_hyper_grads
from .operators import (ConstantDiagLinearOperator, DenseLinearOperator, DiagLinearOperator, FixedPlusConstantDiagLinearOperator, LinearOperator, SolverTerms,
                        StructuredAddedDiagLinearOperator, _same_index, _strip_ellipsis, split_diag)


def rbfgrad_dense(x1: torch.Tensor, x2: torch.Tensor, lengthscale: torch.Tensor, diag: bool = False) -> torch.Tensor:
    """The covariance of values and gradients under the RBF kernel in autograd-visible torch ops, any dtype, any batch shape: x1 [..., n, d],
    x2 [..., m, d], lengthscale [..., 1, 1 or d].  Returns [..., n (d + 1), m (d + 1)] in the interleaved ordering; with ``diag`` the diagonal
    [..., n (d + 1)] (value entries 1, derivative entries 1 / l_a^2), which, as in the reference, exists only for x1 == x2."""
    n, d = x1.shape[-2:]
    m = x2.shape[-2]
    il = (1.0 / lengthscale).expand(*lengthscale.shape[:-1], d)                        # [..., 1, d]
    if diag:
        if not (n == m and torch.equal(x1, x2)):
            raise RuntimeError("diag=True only works when x1 == x2")
        batch = torch.broadcast_shapes(x1.shape[:-2], il.shape[:-2])
        return torch.cat([torch.ones(*batch, n, 1, dtype=x1.dtype, device=x1.device), il.pow(2).expand(*batch, n, d)], -1).reshape(*batch, n * (d + 1))
    delta = (x1 * il).unsqueeze(-2) - (x2 * il).unsqueeze(-3)                          # [..., n, m, d]
    k = torch.exp(-0.5 * delta.pow(2).sum(-1)).unsqueeze(-1)                           # [..., n, m, 1]
    ilb = il.unsqueeze(-2)                                                             # [..., 1, 1, d]
    kd = k * delta * ilb                                                               # k delta_b / l_b
    eye = torch.eye(d, dtype=x1.dtype, device=x1.device)
    hess = k.unsqueeze(-1) * (eye - delta.unsqueeze(-1) * delta.unsqueeze(-2)) * (ilb.unsqueeze(-1) * ilb.unsqueeze(-2))   # [..., n, m, d, d]
    top = torch.cat([k, kd], -1).unsqueeze(-2)                                         # [..., n, m, 1, d + 1]
    rest = torch.cat([-kd.unsqueeze(-1), hess], -1)                                    # [..., n, m, d, d + 1]
    blk = torch.cat([top, rest], -2)                                                   # [..., n, m, a, b]
    return blk.transpose(-3, -2).reshape(*blk.shape[:-4], n * (d + 1), m * (d + 1))


def matern52grad_dense(x1: torch.Tensor, x2: torch.Tensor, lengthscale: torch.Tensor, diag: bool = False) -> torch.Tensor:
    """``rbfgrad_dense`` for the Matern-5/2 kernel: same arguments, shapes, ordering and ``diag`` rule (value entries 1, derivative entries
    (5/3) / l_a^2).  The radial factors g and w are written out, not differentiated, and the square root carries the epsilon of
    ``kernels.stationary_dense``, so the matrix and its gradients are finite at coincident points."""
    n, d = x1.shape[-2:]
    m = x2.shape[-2]
    il = (1.0 / lengthscale).expand(*lengthscale.shape[:-1], d)                        # [..., 1, d]
    if diag:
        if not (n == m and torch.equal(x1, x2)):
            raise RuntimeError("diag=True only works when x1 == x2")
        batch = torch.broadcast_shapes(x1.shape[:-2], il.shape[:-2])
        return torch.cat([torch.ones(*batch, n, 1, dtype=x1.dtype, device=x1.device), (5.0 / 3.0) * il.pow(2).expand(*batch, n, d)],
                         -1).reshape(*batch, n * (d + 1))
    delta = (x1 * il).unsqueeze(-2) - (x2 * il).unsqueeze(-3)                          # [..., n, m, d]
    s = ((delta.pow(2).sum(-1) + 1e-20).sqrt() * 5.0 ** 0.5).unsqueeze(-1)             # [..., n, m, 1]
    e = torch.exp(-s)
    k, g, w = (1.0 + s + s * s / 3.0) * e, (5.0 / 3.0) * (1.0 + s) * e, (25.0 / 3.0) * e
    ilb = il.unsqueeze(-2)                                                             # [..., 1, 1, d]
    gd = g * delta * ilb                                                               # g delta_b / l_b
    eye = torch.eye(d, dtype=x1.dtype, device=x1.device)
    hess = (g.unsqueeze(-1) * eye - w.unsqueeze(-1) * delta.unsqueeze(-1) * delta.unsqueeze(-2)) * (ilb.unsqueeze(-1) * ilb.unsqueeze(-2))
    top = torch.cat([k, gd], -1).unsqueeze(-2)                                         # [..., n, m, 1, d + 1]
    rest = torch.cat([-gd.unsqueeze(-1), hess], -1)                                    # [..., n, m, d, d + 1]
    blk = torch.cat([top, rest], -2)                                                   # [..., n, m, a, b]
    return blk.transpose(-3, -2).reshape(*blk.shape[:-4], n * (d + 1), m * (d + 1))


def _gradgrad_block(u: torch.Tensor, il: torch.Tensor) -> torch.Tensor:
    """The (2 d + 1) x (2 d + 1) Hermite block of every pair WITHOUT its factor k: u [..., d] the scaled differences, il (broadcastable to u) the
    inverse lengthscales; [..., 2 d + 1 (row component), 2 d + 1 (column component)].  Entries of two different dimensions (or with the value)
    factor into a row vector [1, -He_1 / l, He_2 / l^2] times a column vector [1, He_1 / l, He_2 / l^2]; the same-dimension entries
    (-1)^a He_{a+b} / l^{a+b} differ from that outer product by 1 / l^2, +-2 u / l^3 and (2 - 4 u^2) / l^4 on the diagonals of the four
    derivative sub-blocks."""
    d = u.shape[-1]
    il = il.expand_as(u)
    il2 = il * il
    one = torch.ones(*u.shape[:-1], 1, dtype=u.dtype, device=u.device)
    h2 = (u * u - 1.0) * il2
    rho = torch.cat([one, -u * il, h2], -1)
    gam = torch.cat([one, u * il, h2], -1)
    c12 = torch.diag_embed(2.0 * u * il * il2)
    corr = torch.cat([torch.cat([torch.diag_embed(il2), c12], -1), torch.cat([-c12, torch.diag_embed((2.0 - 4.0 * u * u) * il2 * il2)], -1)], -2)
    blk = rho.unsqueeze(-1) * gam.unsqueeze(-2)
    return blk + torch.nn.functional.pad(corr, (1, 0, 1, 0))


def rbfgradgrad_dense(x1: torch.Tensor, x2: torch.Tensor, lengthscale: torch.Tensor, diag: bool = False) -> torch.Tensor:
    """The covariance of values, gradients and non-mixed second derivatives under the RBF kernel (``gpytorch/kernels/rbf_kernel_gradgrad.py:60-166``)
    in autograd-visible torch ops, any dtype, any batch shape, rectangular inputs included: x1 [..., n, d], x2 [..., m, d], lengthscale
    [..., 1, 1 or d].  With u = (x_i - x_j) / l, k = exp(-|u|^2 / 2) and derivative orders alpha, beta in {0, e_a, 2 e_a}

        K[(i, alpha), (j, beta)] = k prod_q (-1)^{alpha_q} He_{alpha_q + beta_q}(u_q) / l_q^{alpha_q + beta_q}

    Returns [..., n (2 d + 1), m (2 d + 1)] in the interleaved ordering (row i (2 d + 1) + c: the value, d/dx_c or d2/dx_{c-d}^2 of point i); with
    ``diag`` the diagonal [..., n (2 d + 1)] (1, 1 / l_a^2, 3 / l_a^4), which, as in the reference, exists only for x1 == x2."""
    n, d = x1.shape[-2:]
    m = x2.shape[-2]
    c = 2 * d + 1
    il = (1.0 / lengthscale).expand(*lengthscale.shape[:-1], d)                        # [..., 1, d]
    if diag:
        if not (n == m and torch.equal(x1, x2)):
            raise RuntimeError("diag=True only works when x1 == x2")
        batch = torch.broadcast_shapes(x1.shape[:-2], il.shape[:-2])
        return torch.cat([torch.ones(*batch, n, 1, dtype=x1.dtype, device=x1.device), il.pow(2).expand(*batch, n, d), 3.0 * il.pow(4).expand(*batch, n, d)],
                         -1).reshape(*batch, n * c)
    u = (x1 * il).unsqueeze(-2) - (x2 * il).unsqueeze(-3)                              # [..., n, m, d]
    k = torch.exp(-0.5 * u.pow(2).sum(-1))                                             # [..., n, m]
    blk = _gradgrad_block(u, il.unsqueeze(-2)) * k.unsqueeze(-1).unsqueeze(-1)         # [..., n, m, a, b]
    return blk.transpose(-3, -2).reshape(*blk.shape[:-4], n * c, m * c)


GRAD_DENSE = {"rbf": rbfgrad_dense, "matern52": matern52grad_dense}                    # family -> the autograd-visible dense form
GRAD_G0 = {"rbf": 1.0, "matern52": 5.0 / 3.0}                                          # g(0): the derivative entries of the diagonal are g(0) / l_a^2


def _probe_major(rhs: torch.Tensor, wd) -> torch.Tensor:
    return B.to_probe_major(rhs.detach(), wd)


def _split_noise(other: DiagLinearOperator, device, dtype):
    """``split_diag`` for the constant diagonals; any other diagonal (the per-task noise of ``MultitaskGaussianLikelihood``, repeated over the
    points) stays WHOLE as the vector, equal entries or not, so that every entry keeps its own autograd path."""
    if isinstance(other, (ConstantDiagLinearOperator, FixedPlusConstantDiagLinearOperator)):
        return split_diag(other, device, dtype)
    return torch.zeros(1, device=device, dtype=dtype), other._diag


class GradMatmulFn(torch.autograd.Function):
    """(outputscale * K_grad(x1, x2)) @ rhs on the fused kernel, with the hyper-parameter gradients of the fused bilinear derivative; the family is
    the operator's (its prepared points carry it to the backend)."""

    @staticmethod
    def forward(ctx, op, lengthscale, outputscale, rhs):
        p1, p2 = op.prepared()
        out_t = B.rbfgrad_kv(p1, p2, op._invl(), _probe_major(rhs, torch.float32), scale=op._os(), order=op.order)
        ctx.op = op
        ctx.save_for_backward(lengthscale, outputscale if outputscale is not None else torch.empty(0), rhs)
        ctx.has_os = outputscale is not None
        return B.from_probe_major(out_t, op.shape[0]).to(rhs.dtype)

    @staticmethod
    def backward(ctx, g):
        lengthscale, outputscale, rhs = ctx.saved_tensors
        outputscale = outputscale if ctx.has_os else None
        op = ctx.op
        p1, p2 = op.prepared()
        d_ls = d_os = d_rhs = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            sums = B.rbfgrad_kv_grad(p1, p2, op._invl(), _probe_major(g, torch.float32), _probe_major(rhs, torch.float32), order=op.order)
            d_ls, d_os = rbfgrad_hyper_grads(sums, lengthscale, outputscale)
        if ctx.needs_input_grad[3]:
            d_rhs = B.from_probe_major(B.rbfgrad_kv(p2, p1, op._invl(), _probe_major(g, torch.float32), scale=op._os(), order=op.order),
                                       op.shape[1]).to(rhs.dtype)
        return None, d_ls, d_os, d_rhs


RBFGradMatmulFn = GradMatmulFn


class GradFusedLinearOperator(LinearOperator):
    """outputscale * K_grad(x1, x2): n (d + 1) x m (d + 1), matrix-free (float32, d <= 4, no batch; ``kernels.rbfgrad_native`` /
    ``kernels.matern52grad_native`` have the rule).  ``family``: "rbf" | "matern52"; ``order``: 1 (value + gradient, d + 1 components per point)
    or 2 (+ the d non-mixed second derivatives: 2 d + 1 components, RBF only); the subclasses below fix both."""

    family = None
    order = 1

    def __init__(self, x1, x2, lengthscale, outputscale=None, shift=None):
        if self.family not in GRAD_DENSE:
            raise TypeError("construct RBFGradFusedLinearOperator, Matern52GradFusedLinearOperator or RBFGradGradFusedLinearOperator")
        self.x1, self.x2 = x1, x2
        self.lengthscale, self.outputscale = lengthscale, outputscale
        self.shift = x1.detach().mean(dim=-2) if shift is None else shift
        self.d = x1.shape[-1]
        self.comps = self.order * self.d + 1
        self._prep = None
        self._same = None

    dtype = property(lambda self: self.x1.dtype)
    device = property(lambda self: self.x1.device)

    @property
    def requires_grad(self):
        return bool(self.lengthscale.requires_grad or (self.outputscale is not None and self.outputscale.requires_grad))

    @property
    def square_same_inputs(self):
        if self._same is None:
            x1, x2 = self.x1, self.x2
            self._same = x1 is x2 or (x1.shape == x2.shape and (x1.data_ptr() == x2.data_ptr() or bool(torch.equal(x1, x2))))
        return self._same

    def _size(self):
        c = self.comps
        return torch.Size([self.x1.shape[-2] * c, self.x2.shape[-2] * c])

    def _dense_fn(self):
        return rbfgradgrad_dense if self.order == 2 else GRAD_DENSE[self.family]

    def _os(self):
        return None if self.outputscale is None else self.outputscale.detach().reshape(-1)[:1].to(torch.float32).contiguous()

    def _invl(self):
        return B.rbfgrad_inv_ls(self.lengthscale, self.d, self.device)

    def prepared(self):
        """The family's prepared points of both clouds (shared shift: the mean of x1 of the original kernel call; slices keep it)."""
        if self._prep is None:
            p1 = B.prep_points(self.family, self.x1, self.lengthscale, self.shift)
            p2 = p1 if self.square_same_inputs else B.prep_points(self.family, self.x2.to(self.x1.dtype), self.lengthscale, self.shift)
            self._prep = (p1, p2)
        return self._prep

    def _matmul(self, rhs):
        return GradMatmulFn.apply(self, self.lengthscale, self.outputscale, rhs)

    def _transpose_nonbatch(self):
        # K_ab(i, j) with delta -> -delta is K_ba(j, i): the transposed operator is the same operator on the exchanged clouds
        return type(self)(self.x2, self.x1, self.lengthscale, self.outputscale, self.shift)

    def _mul_constant(self, c):
        if c.numel() > 1:
            return super()._mul_constant(c)
        os_ = c if self.outputscale is None else self.outputscale.reshape(()) * c.reshape(())
        return type(self)(self.x1, self.x2, self.lengthscale, os_.reshape(1), self.shift)

    def _scaled(self, k):
        return k if self.outputscale is None else k * self.outputscale.reshape(())

    def diagonal(self, offset=0, dim1=-2, dim2=-1):
        if self.square_same_inputs:
            return self._scaled(self._dense_fn()(self.x1, self.x1, self.lengthscale, diag=True))
        return self.to_dense().diagonal()

    def to_dense(self, dtype=None):
        """The dense matrix by the family's dense form on the centred clouds (autograd-visible; ``dtype``: evaluate in that dtype)."""
        dt = self.dtype if dtype is None else dtype
        sh = self.shift.to(self.x1.dtype)
        x1 = (self.x1 - sh).to(dt)
        x2 = x1 if self.square_same_inputs else (self.x2 - sh).to(dt)
        k = self._dense_fn()(x1, x2, self.lengthscale.to(dt))
        return k if self.outputscale is None else k * self.outputscale.reshape(()).to(dt)

    def _point_slice(self, sl, npts):
        """The slice of points a slice of rows / columns covers, or None when it cuts through a point."""
        if not isinstance(sl, slice):
            return None
        c = self.comps
        a, b, step = sl.indices(npts * c)
        if step != 1 or a % c or b % c:
            return None
        return slice(a // c, max(a, b) // c)

    def __getitem__(self, index):
        index = _strip_ellipsis(index)
        if not isinstance(index, tuple):
            index = (index, slice(None))
        r, c = index
        pr, pc = self._point_slice(r, self.x1.shape[-2]), self._point_slice(c, self.x2.shape[-2])
        if pr is None or pc is None:
            return DenseLinearOperator(self.to_dense()[index])
        x1 = self.x1[pr]
        x2 = x1 if (self.square_same_inputs and _same_index(pr, pc)) else self.x2[pc]
        return type(self)(x1, x2, self.lengthscale, self.outputscale, self.shift)

    def _row(self, p):
        """Row p of the matrix: the radial factors of point p // C against every point times the block polynomials of component p % C."""
        p1, p2 = self.prepared()
        return rbfgrad_rows(p1, p2, self._invl(), self._os(), p, self.order)

    def detach(self):
        x1 = self.x1.detach()
        x2 = x1 if self.x2 is self.x1 else self.x2.detach()
        return type(self)(x1, x2, self.lengthscale.detach(), None if self.outputscale is None else self.outputscale.detach(), self.shift)

    def __add__(self, other):
        if isinstance(other, DiagLinearOperator) and self.is_square and not other.batch_shape:
            noise, vec = _split_noise(other, self.device, self.dtype)
            return self.added_diag_cls(self, noise, noise_vec=vec)
        return super().__add__(other)


def rbfgrad_rows(p1, p2, inv_ls, os_, p, order=1):
    """Row p (a 1-element index tensor) of outputscale * K_grad over the prepared clouds, [m C], C = order d + 1; the family is that of the prepared
    points.  RBF: k by the family's ``kernel_rows`` (order 2: times the Hermite block of ``rbfgradgrad_dense``).  Matern-5/2: a row needs g and w
    as well as k, so the three come from delta in torch."""
    d, c = p1.d, order * p1.d + 1
    i, comp = torch.div(p.reshape(1), c, rounding_mode="floor"), p.reshape(1) % c
    invc = 1.0 / B.prep_coef(p1.kind)
    delta = (p1.xp[i, :d] - p2.xp[:, :d]) * invc                                       # [m, d], units of the lengthscale
    il = inv_ls.reshape(1, d)
    if order == 2:
        k = B.kernel_rows(p1, i, p2, os_).reshape(-1, 1, 1)                            # [m, 1, 1]
        return (_gradgrad_block(delta, il) * k).index_select(1, comp).reshape(-1)
    if p1.kind == "rbf":
        k = B.kernel_rows(p1, i, p2, os_).reshape(-1, 1)                               # [m, 1]
        kd = k * delta * il
        top = torch.cat([k, kd], -1)                                                   # component 0: [k, k delta_b / l_b]
        eye = torch.eye(d, device=k.device, dtype=k.dtype)
        hess = k.unsqueeze(-1) * (eye - delta.unsqueeze(-1) * delta.unsqueeze(-2)) * (il.unsqueeze(-1) * il.unsqueeze(-2))   # [m, a, b]
    else:
        s = delta.pow(2).sum(-1, keepdim=True).sqrt() * 5.0 ** 0.5                     # [m, 1]
        e = torch.exp(-s) * (1.0 if os_ is None else os_.reshape(()))
        k, g, w = (1.0 + s + s * s / 3.0) * e, (5.0 / 3.0) * (1.0 + s) * e, (25.0 / 3.0) * e
        kd = g * delta * il
        top = torch.cat([k, kd], -1)                                                   # component 0: [k, g delta_b / l_b]
        eye = torch.eye(d, device=k.device, dtype=k.dtype)
        hess = (g.unsqueeze(-1) * eye - w.unsqueeze(-1) * delta.unsqueeze(-1) * delta.unsqueeze(-2)) * (il.unsqueeze(-1) * il.unsqueeze(-2))
    rest = torch.cat([-kd.unsqueeze(-1), hess], -1)                                    # [m, a, d + 1]
    rows = torch.cat([top.unsqueeze(1), rest], 1)                                      # [m, d + 1 (component of p), d + 1]
    return rows.index_select(1, comp).reshape(-1)


def rbfgrad_preconditioner(xp, inv_ls, os_, diag_total, rank=None, tol=None, min_size=None, order=1):
    """Pivoted-Cholesky preconditioner of outputscale * K_grad(x, x) + diag (the reference preconditions this operator like any other
    ``AddedDiagLinearOperator``, ``settings.py:6-31``; derivative GPs are badly conditioned, so it matters here): rows by ``rbfgrad_rows``, the
    family that of the prepared points."""
    if not xp.fused:
        return None
    theta = 1.0 if os_ is None else os_.reshape(())
    point = [torch.ones(1, device=inv_ls.device), GRAD_G0[xp.kind] * inv_ls.pow(2)] + ([3.0 * inv_ls.pow(4)] if order == 2 else [])
    kdiag = (torch.cat(point) * theta).repeat(xp.n)
    return preconditioner_for_diag(lambda p: rbfgrad_rows(xp, xp, inv_ls, os_, p, order), kdiag, diag_total, rank, tol, min_size)


class GradFusedAddedDiagLinearOperator(StructuredAddedDiagLinearOperator):
    """outputscale * K_grad(x, x) + noise I + diag(noise_vec): the operator the MLL and the prediction caches of a derivative GP solve with.  The
    per-task noise of ``MultitaskGaussianLikelihood`` arrives as the vector (``_split_noise``); both parts stay on the autograd path.  The family is
    ``kg``'s.  The solver takes the whole diagonal as ``dvec`` and scales the unscaled slabs of the fused product itself."""

    kg = property(lambda self: self.inner)

    def __add__(self, other):
        if isinstance(other, DiagLinearOperator) and not other.batch_shape:
            return self._add_diag(*_split_noise(other, self.device, self.dtype))
        return super().__add__(other)

    def _plans(self):
        """t -> the launch plan of a t-column product (one per width the solver asks for)."""
        (p1, _), inv_ls, order, plans = self.kg.prepared(), self.kg._invl(), self.kg.order, {}

        def plan(t):
            if t not in plans:
                plans[t] = B.RbfGradPlan(p1, p1, inv_ls, t, order=order)
            return plans[t]

        return plan

    def _solver_terms(self):
        plan = self._plans()
        return SolverTerms(lambda dt: plan(dt.shape[0])(dt), self.kg._os(), None, self._dvec(torch.float32), torch.float32)

    def _root_matvec(self, terms):
        plan, os_, dv = self._plans(), terms.scale, terms.dvec
        return lambda q_row: plan(q_row.shape[0]).product(q_row, os_, dv, q_row)      # the fused product with the diagonal epilogue

    def _build_precond(self):
        p1, _ = self.kg.prepared()
        return rbfgrad_preconditioner(p1, self.kg._invl(), self.kg._os(), self._dvec(torch.float32), order=self.kg.order)

    def _mll(self, rhs):
        nvec = self.noise_vec if self.noise_vec is not None else torch.zeros(0, device=self.device, dtype=self.dtype)
        return GradInvQuadLogdetFn.apply(self.kg.lengthscale, self.kg.outputscale, self.noise, nvec, rhs, self, self.bbmm_opts)

    def _dense64(self, differentiable=True):
        return self.to_dense(torch.float64)                                            # (the dense form is autograd-visible)


class RBFGradFusedAddedDiagLinearOperator(GradFusedAddedDiagLinearOperator):
    """``GradFusedAddedDiagLinearOperator`` of the RBF family."""


class Matern52GradFusedAddedDiagLinearOperator(GradFusedAddedDiagLinearOperator):
    """``GradFusedAddedDiagLinearOperator`` of the Matern-5/2 family."""


class RBFGradGradFusedAddedDiagLinearOperator(GradFusedAddedDiagLinearOperator):
    """``GradFusedAddedDiagLinearOperator`` of the RBF family with second derivatives."""


class RBFGradFusedLinearOperator(GradFusedLinearOperator):
    """``GradFusedLinearOperator`` of the RBF family (``kernels.RBFKernelGrad``)."""

    family = "rbf"
    added_diag_cls = RBFGradFusedAddedDiagLinearOperator


class Matern52GradFusedLinearOperator(GradFusedLinearOperator):
    """``GradFusedLinearOperator`` of the Matern-5/2 family (``kernels.Matern52KernelGrad``)."""

    family = "matern52"
    added_diag_cls = Matern52GradFusedAddedDiagLinearOperator


class RBFGradGradFusedLinearOperator(GradFusedLinearOperator):
    """``GradFusedLinearOperator`` of the RBF family at derivative order 2 (``kernels.RBFKernelGradGrad``): outputscale * K(x1, x2) over the value,
    the d first and the d non-mixed second partial derivatives of every point, n (2 d + 1) x m (2 d + 1), matrix-free (csrc/kv_rbfgradgrad.hpp)."""

    family = "rbf"
    order = 2
    added_diag_cls = RBFGradGradFusedAddedDiagLinearOperator


class GradInvQuadLogdetFn(torch.autograd.Function):
    """(inv_quad[c], logdet) of outputscale * K_grad(x, x) + noise I + diag(noise_vec) by preconditioned mBCG + SLQ (``bbmm.inv_quad_logdet_forward``
    on the fused product, one launch per four columns plus the solver's reduce); the backward is one fused bilinear derivative."""

    @staticmethod
    def forward(ctx, lengthscale, outputscale, noise, noise_vec, rhs, op, opts):
        n = op.shape[-1]
        partials, os_, _, dv, wd, _ = op._solver_terms()
        res, ctx.group, ctx.t_total = structured_forward(opts, _probe_major(rhs, wd), os_, None, dv, partials, n, op._precond)
        ctx.xp, ctx.inv_ls, ctx.n, ctx.res, ctx.order = op.kg.prepared()[0], op.kg._invl(), n, res, op.kg.order
        ctx.has_os = outputscale is not None
        ctx.save_for_backward(lengthscale, outputscale if outputscale is not None else torch.empty(0), noise, noise_vec, rhs)
        return res.inv_quad.to(rhs.dtype), res.logdet.to(rhs.dtype)

    @staticmethod
    def backward(ctx, g_iq, g_ld):
        lengthscale, outputscale, noise, noise_vec, rhs = ctx.saved_tensors
        outputscale = outputscale if ctx.has_os else None
        xp, n, res = ctx.xp, ctx.n, ctx.res
        left, right, s_y = backward_vectors(res, g_iq, g_ld, ctx.t_total)
        sums = B.rbfgrad_kv_grad(xp, xp, ctx.inv_ls, left, right, order=ctx.order)
        d_ls, d_os = rbfgrad_hyper_grads(sums, lengthscale, outputscale)
        d_noise, d_vec, d_rhs = structured_backward_tail(left, right, s_y, n, g_iq, rhs, ctx.needs_input_grad[4], noise=noise, entrywise=True,
                                                         noise_vec=noise_vec if (noise_vec.numel() and ctx.needs_input_grad[3]) else None)
        allreduce_grads_([d_ls, d_os, d_noise, d_vec], ctx.group)
        return d_ls, d_os, d_noise, d_vec, d_rhs, None, None


RBFGradInvQuadLogdetFn = GradInvQuadLogdetFn
