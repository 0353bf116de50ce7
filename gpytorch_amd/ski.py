"""Structured kernel interpolation (KISS-GP): K ~= W K_UU W^T on a regular grid, matrix-free.

Mirrors ``gpytorch/kernels/grid_interpolation_kernel.py``, ``grid_kernel.py`` and ``utils/interpolation.py`` (Wilson & Nickisch 2015): W [n, M] holds
the 4^d cubic-convolution weights of every point (Keys 1981), K_UU = T_0 kron T_1 kron ... is a Kronecker product of per-axis symmetric Toeplitz
matrices, axis 0 slowest -- the same order as the node index of the interpolation.  The reference stores W as n x 4^d indices plus n x 4^d values
and multiplies through generic sparse operations; here W is never stored: the gather W U and the scatter W^T V (``csrc/kv_ski.hpp``, the scatter
without atomics) recompute every stencil from the d coordinates of its point.  The grid-side product stays in torch, one product per axis with the
T_i built from the first columns (dense up to 1024 nodes, the FFT of the circulant embedding beyond) -- which is what hands the hyper-parameter gradients to autograd: every derivative of a SKI quantity is the
derivative of  sum_c a_c^T (kron T_i) b_c  with a = W^T left, b = W^T right, through the Toeplitz columns.

The rule, per axis (``interp_axis``): g0 = grid[0], h = grid[1] - grid[0]; s = (x - g0) / h, f = floor(s), r = s - f in float64; base node
b = f - 1; weights u(r + 1), u(r), u(r - 1), u(r - 2); b < 0 or b > m - 4: the base is clamped and the weights become one-hot at the node of the
first / last four nearest to x.  ``ski_dense`` is the same operator as an autograd-visible torch expression (any dtype, batches, the CPU).

ADDITIVE FORM (``AdditiveStructureKernel`` over ``GridInterpolationKernel(num_dims=1)``; ``backend.SkiGridSpec(grid, additive=True)``): input column q
is interpolated onto its own one-dimensional axis q, W_add = [W_0 | .. | W_{d-1}] with 4 d non-zeros per row, K_UU = blockdiag(T_q) and
K = scale W_add K_UU W_add^T = scale sum_q W_q T_q W_q^T (``csrc/kv_ski_add.hpp``, 2 <= d <= 16).  Everything below serves both structures: the
axis factors of ``ski_dense`` / ``_row`` are summed instead of multiplied, the grid-side product is ``backend.grid_matmul``, and ``columns`` may
hold ONE column shared by all axes.

INPUT GRADIENTS (deep kernel learning: a network in front of the kernel).  The weights are differentiable in x (``interp_axis``: r carries d/dx, the
floor and a one-hot boundary row none), so ``ski_dense`` is.  The matrix-free operator keeps the graph-attached inputs beside the detached clouds and
returns their gradients from ``input_grads``: for sum_c l_c^T K r_c, d/dx1[p, a] = sum_c l_c[p] sum_k (dw_pk / dx_a) G_R[c][node_pk] with
G_R = scale K_UU W_2^T R, two more grid-side products of the scatters the hyper-gradients form anyway and ONE launch of the derivative-stencil kernel
(``backend.ski_interp_grad``).  Kronecker grids only: the additive form keeps its dense branch for such inputs.

AXIS ORDER.  The reference assembles its Kronecker factors in reversed order through ``linear_operator``; the contract here is the kernel being
approximated: W K_UU W^T -> base_kernel(x1, x2) as the grid refines, every ARD lengthscale on its own axis.
"""
from __future__ import annotations

import torch

from . import backend as B
from . import settings
from .bbmm import backward_vectors, preconditioner_for_diag, structured_backward_tail, structured_forward
from .operators import (DenseLinearOperator, DiagLinearOperator, LinearOperator, SolverTerms, StructuredAddedDiagLinearOperator, _same_index,
                        _strip_ellipsis, split_diag)


# ---------------------------------------------------------------------------------------------- interpolation rule (pure torch)
def cubic_weight(a: torch.Tensor) -> torch.Tensor:
    """Keys' cubic convolution kernel u(a), |a| <= 2."""
    a = a.abs()
    inner = ((1.5 * a - 2.5) * a) * a + 1.0
    outer = ((-0.5 * a + 2.5) * a - 4.0) * a + 2.0
    return torch.where(a < 1.0, inner, outer)


def interp_axis(x: torch.Tensor, g0: float, h: float, m: int):
    """One axis of the rule for coordinates x [...]: (base [...] int64 in 0 .. m - 4, weights [..., 4] in x's dtype, boundary mask [...]).  The
    weights are differentiable in x as the reference's are (``Interpolation.interpolate`` detaches the stencil base only): r carries d/dx = 1 / h,
    the floor and the base none, and a one-hot boundary row none."""
    s = (x.to(torch.float64) - g0) / h
    f = torch.floor(s.detach())
    r = s - f
    s = s.detach()
    b = f.to(torch.int64) - 1
    off = torch.tensor([1.0, 0.0, -1.0, -2.0], dtype=torch.float64, device=x.device)
    w = cubic_weight(r.unsqueeze(-1) + off)
    left, right = b < 0, b > m - 4
    pos = torch.where(left, (s > 0.5).to(torch.int64), 2 + (s > m - 1.5).to(torch.int64))
    onehot = torch.nn.functional.one_hot(pos, 4).to(torch.float64)
    edge = left | right
    w = torch.where(edge.unsqueeze(-1), onehot, w)
    return b.clamp(0, m - 4), w.to(x.dtype), edge


def check_bounds(x: torch.Tensor, spec: B.SkiGridSpec) -> None:
    """The reference's bounds check (``Interpolation.interpolate``): a point more than 1e-7 outside [grid.min, grid.max] is an error.  Made on the
    host, before any launch."""
    flat = x.detach().reshape(-1, x.shape[-1])
    if flat.shape[0] == 0:
        return
    lo, hi = flat.min(0)[0].tolist(), flat.max(0)[0].tolist()
    for i in range(spec.d):
        if lo[i] - spec.lo[i] < -1e-7 or hi[i] - spec.hi[i] > 1e-7:
            raise RuntimeError("Received data that was out of bounds for the specified grid. Grid bounds were ({:.3f}, {:.3f}), but min = {:.3f}, "
                               "max = {:.3f}".format(spec.lo[i], spec.hi[i], lo[i], hi[i]))


def interp_dense_w(x: torch.Tensor, grid, additive: bool = False) -> torch.Tensor:
    """The dense interpolation matrix W [n, M] (small problems and tests).  ``additive``: W_add = [W_0 | .. | W_{d-1}], column q of x on axis q."""
    if additive:
        return torch.cat([interp_dense_w(x[:, q: q + 1], [g]) for q, g in enumerate(grid)], dim=1)
    spec = B.SkiGridSpec(grid)
    n = x.shape[0]
    idx = torch.zeros(n, 1, dtype=torch.int64, device=x.device)
    val = torch.ones(n, 1, dtype=x.dtype, device=x.device)
    ar = torch.arange(4, device=x.device)
    for i in range(spec.d):
        b, w, _ = interp_axis(x[:, i], spec.g0[i], spec.h[i], spec.m[i])
        idx = (idx.unsqueeze(-1) * spec.m[i] + (b.unsqueeze(-1) + ar).unsqueeze(1)).reshape(n, -1)
        val = (val.unsqueeze(-1) * w.unsqueeze(1)).reshape(n, -1)
    out = torch.zeros(n, spec.nodes, dtype=x.dtype, device=x.device)
    return out.scatter_add_(1, idx, val)


def _axis_factor(col, b1, w1, b2, w2):
    """w1^T T[b1 : b1 + 4, b2 : b2 + 4] w2 for every pair: [..., n, m] (T symmetric Toeplitz with first column ``col``)."""
    ar = torch.arange(4, device=col.device)
    rows = (b1.unsqueeze(-1) + ar)[..., :, None, :, None]
    cols = (b2.unsqueeze(-1) + ar)[..., None, :, None, :]
    sub = col[(rows - cols).abs()]                                                     # [..., n, m, 4, 4]
    return torch.einsum("...na,...nmac,...mc->...nm", w1.to(col.dtype), sub, w2.to(col.dtype))


def _axis_diag(col, w):
    """The diagonal of one axis factor: sum_ac w_a w_c col[|a - c|], [..., n]."""
    ar = torch.arange(4, device=col.device)
    sub = col[(ar.unsqueeze(0) - ar.unsqueeze(1)).abs()]
    return torch.einsum("...a,ac,...c->...", w.to(col.dtype), sub, w.to(col.dtype))


def ski_dense(x1: torch.Tensor, x2: torch.Tensor, grid, columns, diag: bool = False, additive: bool = False) -> torch.Tensor:
    """W_1 (kron T_i) W_2^T in autograd-visible torch ops, any dtype, any batch shape, any d: x1 [..., n, d], x2 [..., m, d]; ``grid``: the d axes;
    ``columns``: the first column of every T_i.  An entry separates across the axes,
    K[p, q] = prod_i w_pi^T T_i[b_pi : b_pi + 4, b_qi : b_qi + 4] w_qi, so neither W nor K_UU is formed.  ``diag``: the diagonal, x1 == x2 only.
    ``additive``: the axis factors are SUMMED, K = sum_i W_i T_i W_i^T (d one-dimensional grids; one column in ``columns`` is shared by all axes)."""
    spec = B.SkiGridSpec(grid, additive)
    same = x1 is x2
    out = None
    for i in range(spec.d):
        col = columns[i if len(columns) > 1 else 0]
        b1, w1, _ = interp_axis(x1[..., i], spec.g0[i], spec.h[i], spec.m[i])
        if diag:
            f = _axis_diag(col, w1)
        else:
            b2, w2 = (b1, w1) if same else interp_axis(x2[..., i], spec.g0[i], spec.h[i], spec.m[i])[:2]
            f = _axis_factor(col, b1, w1, b2, w2)
        out = f if out is None else (out + f if additive else out * f)
    return out


# ---------------------------------------------------------------------------------------------- Toeplitz columns of the base kernel
def toeplitz_columns(base_kernel, grid):
    """The first column of every T_i: what ``base_kernel(grid_i[0], grid_i, last_dim_is_batch=True)`` evaluates (the reference's call,
    ``grid_kernel.py:142-146``), one [m_i] vector per axis, differentiable with respect to the kernel's parameters.  A ``ScaleKernel`` contributes
    its outputscale once per axis, as in the reference.  The stationary families are written out in torch (they run on the CPU and in float64 too);
    any other kernel is called as the reference calls it, on the device."""
    from . import kernels as K

    d = len(grid)
    if isinstance(base_kernel, K.ScaleKernel) and not len(base_kernel.batch_shape):
        os_ = base_kernel.outputscale
        return [c * os_.to(c.dtype) for c in toeplitz_columns(base_kernel.base_kernel, grid)]
    closed = type(base_kernel) in (K.RBFKernel, K.MaternKernel, K.RQKernel, K.PiecewisePolynomialKernel, K.PeriodicKernel)
    if closed and not len(base_kernel.batch_shape) and base_kernel.active_dims is None:
        ls = base_kernel.lengthscale.reshape(-1)
        cols = []
        for i, g in enumerate(grid):
            li = (ls[i] if ls.numel() > 1 else ls[0]).to(g.dtype)
            delta = g - g[0]
            if isinstance(base_kernel, K.PeriodicKernel):
                pl = base_kernel.period_length.reshape(-1)
                pi = (pl[i] if pl.numel() > 1 else pl[0]).to(g.dtype)
                cols.append(torch.exp(-2.0 * torch.sin(torch.pi * delta / pi).pow(2) / li))
                continue
            tau = delta / li
            if isinstance(base_kernel, K.RQKernel):
                alpha = base_kernel.alpha.reshape(()).to(g.dtype)
                cols.append((1.0 + tau.pow(2) / (2.0 * alpha)).pow(-alpha))
            elif isinstance(base_kernel, K.PiecewisePolynomialKernel):
                cols.append(K.pp_dense(tau.abs(), base_kernel.shape_code(d)))
            else:
                cols.append(K.stationary_dense(base_kernel.kind, tau.pow(2)))
        return cols
    mmax = max(g.numel() for g in grid)
    first = torch.stack([g[:1] for g in grid], dim=-1)
    full = torch.stack([torch.cat([g, g.new_zeros(mmax - g.numel())]) for g in grid], dim=-1)
    from .operators import to_dense

    covars = to_dense(base_kernel(first, full, last_dim_is_batch=True))                # [d, 1, mmax]
    return [covars[i, 0, : g.numel()] for i, g in enumerate(grid)]


def _innermost(base_kernel):
    from . import kernels as K

    while isinstance(base_kernel, K.ScaleKernel):
        base_kernel = base_kernel.base_kernel
    return base_kernel


def additive_columns(base_kernel, axis, d):
    """The Toeplitz columns of the additive composition: d copies of ONE grid axis, input column q on copy q.  The reference evaluates the base
    kernel on the one-column grid under ``last_dim_is_batch`` (``grid_kernel.py:142-146``, ``:161-164``): the grid is divided by the lengthscale
    [1, k] FIRST (``rbf_kernel.py:77-79``) and every resulting column becomes a batch member (``kernel.py:336-338``) -- k Toeplitz matrices, member
    j with lengthscale l_j.  k = 1 is repeated over the d dimensions (``grid_interpolation_kernel.py:184-185``); k = d puts l_q on input column q
    (the reference's own test model, ``RBFKernel(ard_num_dims=2)`` at d = 2); any other k fails to broadcast there and is refused here.
    Returns ONE column when every axis carries the same one (a single lengthscale / period), else d columns."""
    from . import kernels as K

    inner = _innermost(base_kernel)
    counts = [p.numel() for p in (getattr(inner, "lengthscale", None), getattr(inner, "period_length", None) if isinstance(inner, K.PeriodicKernel) else None)
              if p is not None]
    if any(k not in (1, d) for k in counts):
        raise RuntimeError(f"GridInterpolationKernel under last_dim_is_batch: {max(counts)} lengthscales do not broadcast against {d} input dimensions")
    if columns_native(base_kernel) and all(k == 1 for k in counts):
        return toeplitz_columns(base_kernel, [axis])
    return toeplitz_columns(base_kernel, [axis] * d)


def columns_native(base_kernel) -> bool:
    """The base kernel's Toeplitz columns come from a differentiable dense torch expression: the stationary families, bare or under ScaleKernels."""
    from . import kernels as K

    while isinstance(base_kernel, K.ScaleKernel):
        if len(base_kernel.batch_shape):
            return False
        base_kernel = base_kernel.base_kernel
    return (type(base_kernel) in (K.RBFKernel, K.MaternKernel, K.RQKernel, K.PiecewisePolynomialKernel, K.PeriodicKernel)
            and not len(base_kernel.batch_shape) and base_kernel.active_dims is None)


def bilinear(at: torch.Tensor, bt: torch.Tensor, columns, spec=None):
    """sum_c a_c^T (kron T_i) b_c for grid vectors A, B [t, >= M], and its gradient with respect to every Toeplitz column: (value, [d columns]).
    Evaluated in float64 (M t numbers per axis).  ``spec``: the grid, where it is additive (K_UU block-diagonal, ``backend.grid_matmul``)."""
    cols = [c.detach().to(torch.float64).requires_grad_(True) for c in columns]
    with torch.enable_grad():
        ops = [B.toeplitz_prepare(c) for c in cols]
        if spec is not None and spec.additive:
            val = (at[:, : spec.nodes].to(torch.float64) * B.grid_matmul(spec, ops, bt.to(torch.float64))).sum()
            grads = torch.autograd.grad(val, cols)
            return val.detach(), [g.to(c.dtype) for g, c in zip(grads, columns)]
        total = 1
        for c in cols:
            total *= c.numel()
        val = (at[:, :total].to(torch.float64) * B.kron_matmul(ops, bt.to(torch.float64))).sum()
        grads = torch.autograd.grad(val, cols)
    return val.detach(), [g.to(c.dtype) for g, c in zip(grads, columns)]


def _no_sharding():
    s = settings.sharding
    if s.is_auto() or s._probe_group is not None or s._row_group is not None or s._mll_row_group is not None:
        raise NotImplementedError("structured kernel interpolation does not shard its probes or rows (settings.sharding)")


def _probe_major(rhs: torch.Tensor) -> torch.Tensor:
    return B.to_probe_major(rhs.detach(), torch.float32)


# ---------------------------------------------------------------------------------------------- operator
def input_grads(op, left, right, at, bt, need1: bool, need2: bool):
    """The gradients of sum_c l_c^T (scale W_1 K_UU W_2^T) r_c with respect to the inputs of ``op`` (an ``SKIFusedLinearOperator``): (d x1, d x2),
    None where not needed.  ``left`` [t, >= n] / ``right`` [t, >= m]: the point vectors; ``at`` = W_1^T left, ``bt`` = W_2^T right [t, M]: their
    scatters, which the hyper-parameter gradients form anyway.
      d x1[p, a] = sum_c l_c[p] sum_k (dw_pk / dx_a) G_R[c][node_pk],   G_R = scale K_UU W_2^T R
      d x2[q, a] = sum_c r_c[q] sum_k (dw_qk / dx_a) G_L[c][node_qk],   G_L = scale K_UU W_1^T L
    each ONE launch of the derivative-stencil kernel (``backend.ski_interp_grad``); where both inputs are the same tensor, one launch with both
    pairs, and the sum is returned as d x1."""
    if not (need1 or need2):
        return None, None
    c1, c2 = op.clouds()
    mats, os_ = op.mats(), op._os()

    def grid(ut):
        u = B.grid_matmul(op.spec, mats, ut)
        return (u if os_ is None else u * os_).contiguous()

    if need1 and need2 and c1 is c2 and op.a1 is op.a2:
        return B.ski_interp_grad(c1, grid(bt), left, grid(at), right).to(op.a1.dtype), None
    d1 = B.ski_interp_grad(c1, grid(bt), left).to(op.a1.dtype) if need1 else None
    d2 = B.ski_interp_grad(c2, grid(at), right).to(op.a2.dtype) if need2 else None
    return d1, d2


class SKIMatmulFn(torch.autograd.Function):
    """(scale * W_1 K_UU W_2^T) @ rhs on the interpolation kernels; the gradients of the Toeplitz columns and of the scale come from ``bilinear``,
    those of the graph-attached inputs ``x1`` / ``x2`` (None: not wanted) from ``input_grads``."""

    @staticmethod
    def forward(ctx, op, scale, rhs, x1, x2, *columns):
        out_t = op.plan().product(_probe_major(rhs), scale=op._os())
        ctx.op = op
        ctx.save_for_backward(rhs, *columns)
        ctx.has_scale = scale is not None
        return B.from_probe_major(out_t, op.shape[0]).to(rhs.dtype)

    @staticmethod
    def backward(ctx, g):
        rhs, *columns = ctx.saved_tensors
        op = ctx.op
        d_scale = d_rhs = d_x1 = d_x2 = None
        d_cols = [None] * len(columns)
        need_x = ctx.needs_input_grad[3] or ctx.needs_input_grad[4]
        if ctx.needs_input_grad[1] or need_x or any(ctx.needs_input_grad[5:]):
            c1, c2 = op.clouds()
            left, right = _probe_major(g), _probe_major(rhs)
            at, bt = B.ski_interp_t(c1, left), B.ski_interp_t(c2, right)
            if ctx.needs_input_grad[1] or any(ctx.needs_input_grad[5:]):
                val, grads = bilinear(at, bt, columns, op.spec)
                sc = 1.0 if op.scale is None else op.scale.detach().reshape(()).to(torch.float64)
                d_cols = [(gc.to(torch.float64) * sc).to(gc.dtype) for gc in grads]
                if ctx.needs_input_grad[1]:
                    d_scale = val.to(op.scale.dtype).reshape(op.scale.shape)
            d_x1, d_x2 = input_grads(op, left, right, at, bt, ctx.needs_input_grad[3], ctx.needs_input_grad[4])
        if ctx.needs_input_grad[2]:
            d_rhs = B.from_probe_major(op._transpose_nonbatch().plan().product(_probe_major(g), scale=op._os()), op.shape[1]).to(rhs.dtype)
        return (None, d_scale, d_rhs, d_x1, d_x2, *d_cols)


class SKIFusedLinearOperator(LinearOperator):
    """scale * W_1 (kron T_i) W_2^T: n x m, matrix-free (float32, d <= 3, no batch; ``kernels.ski_native`` has the rule).  ``grid``: the d axes;
    ``columns``: the first column of every T_i (differentiable); ``scale``: an outer outputscale [1] or None.  With an additive ``spec``
    (``kernels.ski_additive_native``): scale * W_add blockdiag(T_q) W_add^T over d one-dimensional axes, 2 <= d <= 16; ``columns`` then holds one
    column per axis, or ONE column shared by all axes.

    INPUT GRADIENTS (``kernels.ski_input_grad_native``; deep kernel learning: a network in front of the kernel).  An input that requires grad is
    detached ONCE, here: ``x1`` / ``x2`` are the detached tensors every kernel launch and the cloud cache (``backend.ski_cloud``, keyed on the
    tensor's identity) see, forward and backward alike; ``a1`` / ``a2`` keep the graph-attached tensors (None: the input does not require grad)
    and travel with every derived operator (``attached``).  The products (``SKIMatmulFn``), the marginal log likelihood (``SKIInvQuadLogdetFn``)
    and ``to_dense`` (the Cholesky branch) hand them their gradients.  NOT provided: gradients of PREDICTIONS with respect to the inputs -- the
    prediction caches, ``diagonal`` and the preconditioner work from the detached points, so an eval-mode call returns the numbers it returns for
    detached inputs and no gradient reaches the inputs through it."""

    def __init__(self, x1, x2, grid, columns, scale=None, spec=None, attached=None):
        if attached is None:
            a1 = x1 if x1.requires_grad else None
            a2 = a1 if x2 is x1 else (x2 if x2.requires_grad else None)
            d1 = x1.detach() if a1 is not None else x1
            x1, x2 = d1, (d1 if x2 is x1 else (x2.detach() if a2 is not None else x2))
            attached = (a1, a2)
        self.x1, self.x2 = x1, x2
        self.a1, self.a2 = attached
        self.grid, self.columns, self.scale = list(grid), list(columns), scale
        self.spec = B.SkiGridSpec(self.grid) if spec is None else spec      # (an additive spec is always passed in)
        self._same = None
        self._plan = None
        self._axes = {}

    dtype = property(lambda self: self.x1.dtype)
    device = property(lambda self: self.x1.device)

    @property
    def requires_grad(self):
        return bool(any(c.requires_grad for c in self.columns) or (self.scale is not None and self.scale.requires_grad)
                    or self.a1 is not None or self.a2 is not None)

    @property
    def square_same_inputs(self):
        if self._same is None:
            x1, x2 = self.x1, self.x2
            self._same = x1 is x2 or (x1.shape == x2.shape and (x1.data_ptr() == x2.data_ptr() or bool(torch.equal(x1, x2))))
        return self._same

    def _size(self):
        return torch.Size([self.x1.shape[-2], self.x2.shape[-2]])

    def _os(self):
        return None if self.scale is None else self.scale.detach().reshape(-1)[:1].to(torch.float32).contiguous()

    def _new(self, x1, x2, columns=None, scale="keep", attached="keep"):
        """A derived operator on the (detached) points x1, x2; ``attached``: their graph-attached twins (default: this operator's own)."""
        return SKIFusedLinearOperator(x1, x2, self.grid, self.columns if columns is None else columns, self.scale if isinstance(scale, str) else scale,
                                      self.spec, attached=(self.a1, self.a2) if isinstance(attached, str) else attached)

    def clouds(self):
        c1 = B.ski_cloud(self.x1, self.spec)
        return c1, (c1 if self.square_same_inputs else B.ski_cloud(self.x2, self.spec))

    def mats(self):
        """The T_i of the grid-side product (float32, detached): dense, or the circulant spectrum of a long axis (``backend.toeplitz_prepare``)."""
        return [B.toeplitz_prepare(c.detach().to(torch.float32)) for c in self.columns]

    def plan(self) -> B.SkiPlan:
        if self._plan is None:
            c1, c2 = self.clouds()
            self._plan = B.SkiPlan(c1, c2, self.mats())
        return self._plan

    def _matmul(self, rhs):
        return SKIMatmulFn.apply(self, self.scale, rhs, self.a1, self.a2, *self.columns)

    def _transpose_nonbatch(self):
        return self._new(self.x2, self.x1, attached=(self.a2, self.a1))

    def _mul_constant(self, c):
        if c.numel() > 1:
            return super()._mul_constant(c)
        sc = c.reshape(1) if self.scale is None else (self.scale.reshape(()) * c.reshape(())).reshape(1)
        return self._new(self.x1, self.x2, scale=sc)

    def _scaled(self, k):
        return k if self.scale is None else k * self.scale.reshape(()).to(k.dtype)

    def to_dense(self, dtype=None):
        """The dense matrix by ``ski_dense`` (autograd-visible; ``dtype``: evaluate in that dtype)."""
        dt = self.dtype if dtype is None else dtype
        i1, i2 = (self.x1 if self.a1 is None else self.a1), (self.x2 if self.a2 is None else self.a2)       # (the inputs get their gradients)
        x1 = i1.to(dt)
        x2 = x1 if (self.square_same_inputs and self.a2 is self.a1) else i2.to(dt)
        return self._scaled(ski_dense(x1, x2, self.grid, [c.to(dt) for c in self.columns], additive=self.spec.additive))

    def diagonal(self, offset=0, dim1=-2, dim2=-1):
        if self.square_same_inputs:
            return self._scaled(ski_dense(self.x1, self.x1, self.grid, self.columns, diag=True, additive=self.spec.additive))
        n = min(self.shape)
        return self._new(self.x1[:n], self.x2[:n], attached=(None, None)).to_dense().diagonal()

    def _axis(self, which: int):
        """(base [n], weights [n, 4]) per axis of cloud ``which``, cached (the row function of the preconditioner reads them)."""
        if which not in self._axes:
            x = self.x1 if which == 0 else self.x2
            sp = self.spec
            self._axes[which] = [interp_axis(x[:, i], sp.g0[i], sp.h[i], sp.m[i])[:2] for i in range(sp.d)]
        return self._axes[which]

    def _row(self, p):
        """Row p (a 1-element index tensor) of the matrix, [m]: per axis, the four rows of T_i of point p's stencil combined, then gathered."""
        ar = torch.arange(4, device=self.device)
        a1, a2 = self._axis(0), self._axis(0 if self.square_same_inputs else 1)
        p = p.reshape(1)
        out = None
        for i in range(self.spec.d):
            col = self.columns[i if len(self.columns) > 1 else 0].detach()
            (b1, w1), (b2, w2) = a1[i], a2[i]
            nodes = torch.arange(col.numel(), device=self.device)
            tp = (w1[p].reshape(4, 1).to(col.dtype) * col[((b1[p] + ar).unsqueeze(-1) - nodes).abs()]).sum(0)      # [m_i]
            f = (tp[b2.unsqueeze(-1) + ar] * w2.to(col.dtype)).sum(-1)
            out = f if out is None else (out + f if self.spec.additive else out * f)
        return self._scaled(out).detach()

    def __getitem__(self, index):
        index = _strip_ellipsis(index)
        if not isinstance(index, tuple):
            index = (index, slice(None))
        r, c = index
        if isinstance(r, int) or isinstance(c, int):
            return self.to_dense()[index]
        x1 = self.x1[r]
        a1 = None if self.a1 is None else self.a1[r]
        if self.square_same_inputs and _same_index(r, c):
            return self._new(x1, x1, attached=(a1, a1 if self.a2 is self.a1 else (None if self.a2 is None else self.a2[c])))
        return self._new(x1, self.x2[c], attached=(a1, None if self.a2 is None else self.a2[c]))

    def detach(self):
        x1 = self.x1.detach()
        x2 = x1 if self.x2 is self.x1 else self.x2.detach()
        return self._new(x1, x2, [c.detach() for c in self.columns], None if self.scale is None else self.scale.detach(), attached=(None, None))

    def __add__(self, other):
        if isinstance(other, DiagLinearOperator) and self.is_square and not other.batch_shape:
            noise, vec = split_diag(other, self.device, self.dtype)
            return SKIFusedAddedDiagLinearOperator(self, noise, noise_vec=vec)
        return super().__add__(other)

    def prediction_strategy(self, train_inputs, train_prior_dist, train_labels, likelihood):
        return InterpolatedPredictionStrategy(train_inputs, train_prior_dist, train_labels, likelihood)

    # ---- grid-side quantities of the prediction caches
    def grid_product(self, vt: torch.Tensor) -> torch.Tensor:
        """scale * K_UU W_2^T V for point vectors V [t, >= m]: [t, M] grid vectors."""
        _, c2 = self.clouds()
        u = B.grid_matmul(self.spec, self.mats(), B.ski_interp_t(c2, vt))
        return u if self.scale is None else u * self._os()

    def interp_left(self, ut: torch.Tensor) -> torch.Tensor:
        """W_1 U for grid vectors U [t, M]: [n, t]."""
        c1, _ = self.clouds()
        return B.from_probe_major(B.ski_interp(c1, ut.to(torch.float32).contiguous()), self.shape[0])


class SKIFusedAddedDiagLinearOperator(StructuredAddedDiagLinearOperator):
    """scale * W K_UU W^T + noise I + diag(noise_vec): the operator the MLL and the prediction caches of a KISS-GP model solve with.  The solver
    takes the whole diagonal as ``dvec`` and scales the unscaled slabs of the interpolation product itself."""

    ks = property(lambda self: self.inner)

    def restrict(self, idx):
        """The operator of the points ``idx`` alone (the masked mean cache of ``observation_nan_policy``)."""
        x = self.ks.x1[idx]
        a = None if self.ks.a1 is None else self.ks.a1[idx]
        return SKIFusedAddedDiagLinearOperator(self.ks._new(x, x, attached=(a, a)), self.noise, None if self.noise_vec is None else self.noise_vec[idx], self.bbmm_opts)

    def _check(self):
        _no_sharding()

    def _solver_terms(self):
        return SolverTerms(self.ks.plan(), self.ks._os(), None, self._dvec(torch.float32), torch.float32)

    def _root_matvec(self, terms):
        plan, os_, dv = terms.kv_partials, terms.scale, terms.dvec
        return lambda q_row: plan.product(q_row, os_, dv, q_row)                       # the fused product with the diagonal epilogue

    def _build_precond(self):
        return preconditioner_for_diag(self.ks._row, self.ks.diagonal().detach().to(torch.float32), self._diag_total())

    def _mll(self, rhs):
        nvec = self.noise_vec if self.noise_vec is not None else torch.zeros(0, device=self.device, dtype=self.dtype)
        scale = self.ks.scale if self.ks.scale is not None else torch.zeros(0, device=self.device, dtype=self.dtype)
        return SKIInvQuadLogdetFn.apply(scale, self.noise, nvec, rhs, self, self.bbmm_opts, self.ks.a1, self.ks.a2, *self.ks.columns)

    def _dense64(self, differentiable=True):
        return self.to_dense(torch.float64)                                            # (ski_dense is autograd-visible)


class SKIInvQuadLogdetFn(torch.autograd.Function):
    """(inv_quad[c], logdet) of scale * W K_UU W^T + noise I + diag(noise_vec) by preconditioned mBCG + SLQ (``bbmm.inv_quad_logdet_forward`` on the
    interpolation product).  Backward: A = W^T left, B = W^T right by the scatter kernel, then ``bilinear``: the gradients of the Toeplitz columns
    (lengthscales, an inner outputscale, shape parameters follow through the base kernel's own expression) and, as the sum itself, of the scale.
    ``x1`` / ``x2``: the graph-attached inputs (None: not wanted); their gradients take A and B through two more grid-side products and ONE
    launch of the derivative-stencil kernel (``input_grads``)."""

    @staticmethod
    def forward(ctx, scale, noise, noise_vec, rhs, op, opts, x1, x2, *columns):
        n = op.shape[-1]
        ks = op.ks
        _no_sharding()
        if opts.get("group") is not None:
            raise NotImplementedError("structured kernel interpolation does not shard its probes (settings.sharding)")
        plan, os_, _, dv, _, _ = op._solver_terms()
        res, _, ctx.t_total = structured_forward(opts, _probe_major(rhs), os_, None, dv, plan, n, op._precond)
        ctx.ks, ctx.n, ctx.res = ks, n, res
        ctx.has_scale = scale.numel() > 0
        ctx.save_for_backward(scale, noise, noise_vec, rhs, *columns)
        return res.inv_quad.to(rhs.dtype), res.logdet.to(rhs.dtype)

    @staticmethod
    def backward(ctx, g_iq, g_ld):
        scale, noise, noise_vec, rhs, *columns = ctx.saved_tensors
        ks, n, res = ctx.ks, ctx.n, ctx.res
        left, right, s_y = backward_vectors(res, g_iq, g_ld, ctx.t_total)
        cloud, _ = ks.clouds()
        at, bt = B.ski_interp_t(cloud, left), B.ski_interp_t(cloud, right)
        val, grads = bilinear(at, bt, columns, ks.spec)
        sc = scale.detach().reshape(()).to(torch.float64) if ctx.has_scale else 1.0
        d_cols = [(gc.to(torch.float64) * sc).to(gc.dtype) if ctx.needs_input_grad[8 + i] else None for i, gc in enumerate(grads)]
        d_scale = val.to(scale.dtype).reshape(scale.shape) if (ctx.has_scale and ctx.needs_input_grad[0]) else None
        d_x1, d_x2 = input_grads(ks, left, right, at, bt, ctx.needs_input_grad[6], ctx.needs_input_grad[7])
        d_noise, d_vec, d_rhs = structured_backward_tail(left, right, s_y, n, g_iq, rhs, ctx.needs_input_grad[3], noise=noise,
                                                         noise_vec=noise_vec if (noise_vec.numel() and ctx.needs_input_grad[2]) else None)
        return (d_scale, d_noise, d_vec, d_rhs, None, None, d_x1, d_x2, *d_cols)


# ---------------------------------------------------------------------------------------------- prediction
def interpolated_prediction_strategy(train_inputs, train_prior_dist, train_labels, likelihood):
    """What ``GridInterpolationKernel.prediction_strategy`` returns: the interpolated strategy where the training covariance is the matrix-free
    operator, the default one otherwise (dense branch)."""
    from .models import DefaultPredictionStrategy

    cov = train_prior_dist.lazy_covariance_matrix
    cov = cov.evaluate_kernel() if hasattr(cov, "evaluate_kernel") else cov
    if isinstance(cov, SKIFusedLinearOperator):
        return InterpolatedPredictionStrategy(train_inputs, train_prior_dist, train_labels, likelihood)
    return DefaultPredictionStrategy(train_inputs, train_prior_dist, train_labels, likelihood)


def _strategy_base():
    from .models import DefaultPredictionStrategy

    return DefaultPredictionStrategy


class InterpolatedPredictionStrategy(_strategy_base()):
    """``exact_prediction_strategies.py:481-828`` restated: the caches live on the GRID, so a prediction costs one gather over the test points.

      * mean cache  = K_UU W^T K_hat^-1 (y - mu), one grid vector; predictive mean = W_test mean_cache + mu_test;
      * under ``fast_pred_var`` the covariance cache is K_UU W^T S with S S^T ~= K_hat^-1 from the Lanczos root, M x rank; predictive covariance
        = K_** - (W_test C)(W_test C)^T;
      * without ``fast_pred_var`` the covariance is ``DefaultPredictionStrategy.exact_predictive_covar``.

    The reference's fantasy update (WISKI) is not provided."""

    def _train_op(self):
        op = self.lik_train_train_covar.evaluate_kernel()
        return op if isinstance(op, SKIFusedAddedDiagLinearOperator) else None

    def _detach(self, t):
        return t.detach() if settings.detach_test_caches.on() else t

    @property
    def grid_mean_cache(self):
        if getattr(self, "_grid_mean_cache", None) is None:
            op = self._train_op()
            sol = self.mean_cache                                                              # K_hat^-1 (y - mu), [n]
            self._grid_mean_cache = self._detach(op.ks.grid_product(_probe_major(sol.reshape(-1, 1))))
        return self._grid_mean_cache

    @property
    def grid_covar_cache(self):
        if getattr(self, "_grid_covar_cache", None) is None:
            op = self._train_op()
            self._grid_covar_cache = self._detach(op.ks.grid_product(_probe_major(self.covar_cache)))    # [rank, M]
        return self._grid_covar_cache

    def _native(self, test_train_covar):
        return (isinstance(test_train_covar, SKIFusedLinearOperator) and self._train_op() is not None and self.train_labels.dim() == 1
                and (settings.observation_nan_policy.value() == "ignore" or not bool(torch.isnan(self.train_labels).any())))

    def exact_prediction(self, test_mean, test_test_covar, test_train_covar):
        if not self._native(test_train_covar):
            return super().exact_prediction(test_mean, test_test_covar, test_train_covar)
        return (self.exact_predictive_mean(test_mean, test_train_covar), self.exact_predictive_covar(test_test_covar, test_train_covar))

    def exact_predictive_mean(self, test_mean, test_train_covar):
        if not self._native(test_train_covar):
            return super().exact_predictive_mean(test_mean, test_train_covar)
        return test_train_covar.interp_left(self.grid_mean_cache).squeeze(-1).to(test_mean.dtype) + test_mean

    def exact_predictive_covar(self, test_test_covar, test_train_covar):
        if not self._native(test_train_covar) or settings.fast_pred_var.off() or settings.skip_posterior_variances.on():
            return super().exact_predictive_covar(test_test_covar, test_train_covar)
        from .operators import MatmulLinearOperator, SumLinearOperator, to_linear_operator

        self._last_test_train_covar = test_train_covar
        root = test_train_covar.interp_left(self.grid_covar_cache).to(test_train_covar.dtype)      # [n_test, rank]
        if torch.is_tensor(test_test_covar):
            return to_linear_operator(torch.add(test_test_covar, root @ root.mT, alpha=-1))
        return SumLinearOperator(test_test_covar, MatmulLinearOperator(DenseLinearOperator(root), DenseLinearOperator(root.mT.mul(-1))))

    def get_fantasy_strategy(self, *args, **kwargs):
        raise NotImplementedError("InterpolatedPredictionStrategy: fantasy updates (WISKI) are not provided")
