"""Float64 restatement of KISS-GP written from the formulas alone, independent of ``gpytorch_amd``: the oracle of the SKI tests.

Per axis i of a regular grid (g0 = grid_i[0], h = grid_i[1] - grid_i[0], m nodes): s = (x - g0) / h, f = floor(s), r = s - f, base b = f - 1, weights
u(r + 1), u(r), u(r - 1), u(r - 2) with Keys' cubic convolution u(a) = (1.5 |a| - 2.5) |a|^2 + 1 for |a| < 1, ((-0.5 |a| + 2.5) |a| - 4) |a| + 2
otherwise.  b < 0: b = 0 and the weights are one-hot at the nearest of the first four nodes; b > m - 4: b = m - 4, one-hot at the nearest of the last
four.  A point's 4^d weights are the products of its per-axis weights, the flat node index is sum_i idx_i prod_{j > i} m_j (axis 0 slowest), and
K_UU = T_0 kron T_1 kron ... with T_i the symmetric Toeplitz matrix of the base kernel's first column on axis i.
"""
from __future__ import annotations

import math

import torch


def u(a: float) -> float:
    a = abs(a)
    if a < 1.0:
        return (1.5 * a - 2.5) * a * a + 1.0
    return ((-0.5 * a + 2.5) * a - 4.0) * a + 2.0


def axis_stencil(x: float, g0: float, h: float, m: int):
    """(base, [w0..w3], boundary?) of one coordinate on one axis."""
    s = (x - g0) / h
    f = math.floor(s)
    r = s - f
    b = f - 1
    if b < 0:
        near = min(range(4), key=lambda k: (abs(k - s), k))
        return 0, [1.0 if k == near else 0.0 for k in range(4)], True
    if b > m - 4:
        near = min(range(4), key=lambda k: (abs(m - 4 + k - s), k))
        return m - 4, [1.0 if k == near else 0.0 for k in range(4)], True
    return b, [u(r + 1.0), u(r), u(r - 1.0), u(r - 2.0)], False


def grid_numbers(grid):
    g = [a.double() for a in grid]
    return [float(a[0]) for a in g], [float(a[1] - a[0]) for a in g], [a.numel() for a in g]


def dense_w(x: torch.Tensor, grid, return_boundary: bool = False):
    """W [n, M] in float64 (x: float32-exact or float64 values), point by point."""
    g0, h, m = grid_numbers(grid)
    d = len(grid)
    xs = x.double().reshape(-1, d).tolist()
    W = torch.zeros(len(xs), math.prod(m), dtype=torch.float64)
    edge = torch.zeros(len(xs), dtype=torch.bool)
    for p, pt in enumerate(xs):
        idx, val = [0], [1.0]
        for i in range(d):
            b, w, e = axis_stencil(pt[i], g0[i], h[i], m[i])
            edge[p] |= e
            idx = [j * m[i] + b + k for j in idx for k in range(4)]
            val = [v * w[k] for v in val for k in range(4)]
        for j, v in zip(idx, val):
            W[p, j] += v
    return (W, edge) if return_boundary else W


def toeplitz(col: torch.Tensor) -> torch.Tensor:
    m = col.numel()
    i = torch.arange(m)
    return col[(i.unsqueeze(0) - i.unsqueeze(1)).abs()]


def columns(kind: str, grid, lengthscale, inner_scale=None, alpha=None):
    """First Toeplitz columns of a stationary base kernel, one per axis (float64, differentiable): lengthscale a tensor with 1 or d entries; an
    inner outputscale multiplies EVERY axis (a ScaleKernel base is evaluated once per axis)."""
    ls = lengthscale.double().reshape(-1)
    out = []
    for i, a in enumerate(grid):
        a = a.double()
        tau2 = ((a - a[0]) / (ls[i] if ls.numel() > 1 else ls[0])).pow(2)
        if kind == "rbf":
            c = torch.exp(-0.5 * tau2)
        elif kind == "rq":
            c = (1.0 + tau2 / (2.0 * alpha.double().reshape(()))).pow(-alpha.double().reshape(()))
        elif kind == "matern52":
            r = (5.0 * tau2 + 1e-30).sqrt()
            c = (1.0 + r + r * r / 3.0) * torch.exp(-r)
        else:
            raise KeyError(kind)
        out.append(c if inner_scale is None else c * inner_scale.double().reshape(()))
    return out


def k_uu(cols) -> torch.Tensor:
    K = toeplitz(cols[0])
    for c in cols[1:]:
        K = torch.kron(K, toeplitz(c))
    return K


def k_ski(x1, x2, grid, cols, scale=None) -> torch.Tensor:
    K = dense_w(x1, grid) @ k_uu(cols) @ dense_w(x2, grid).T
    return K if scale is None else K * scale.double().reshape(())


def mll(x, y, grid, cols, scale, noise, mean=0.0) -> torch.Tensor:
    """The exact marginal log likelihood PER DATUM (the convention of ExactMarginalLogLikelihood) by dense Cholesky."""
    n = x.shape[0]
    K = k_ski(x, x, grid, cols, scale) + noise.double().reshape(()) * torch.eye(n, dtype=torch.float64)
    L = torch.linalg.cholesky(K)
    r = (y.double() - mean).unsqueeze(-1)
    quad = (r * torch.cholesky_solve(r, L)).sum()
    return (-0.5 * (quad + 2.0 * L.diagonal().log().sum() + n * math.log(2.0 * math.pi))) / n


def posterior(x, y, xs, grid, cols, scale, noise, mean=0.0):
    """(mean, covariance of f) at the test points xs by dense Cholesky."""
    n = x.shape[0]
    K = k_ski(x, x, grid, cols, scale) + noise.double().reshape(()) * torch.eye(n, dtype=torch.float64)
    Ks = k_ski(xs, x, grid, cols, scale)
    Kss = k_ski(xs, xs, grid, cols, scale)
    L = torch.linalg.cholesky(K)
    mu = mean + (Ks @ torch.cholesky_solve((y.double() - mean).unsqueeze(-1), L)).squeeze(-1)
    return mu, Kss - Ks @ torch.cholesky_solve(Ks.T, L)


def kuu_matmul(cols, U: torch.Tensor) -> torch.Tensor:
    """K_UU @ U for U [M, t] without forming the Kronecker product (grids too large for ``k_uu``): one contraction per axis, float64."""
    sizes = [c.numel() for c in cols]
    out = U.double().reshape(*sizes, -1)
    for i, c in enumerate(cols):
        out = torch.movedim(torch.tensordot(toeplitz(c.double()), out, dims=([1], [i])), 0, i)
    return out.reshape(-1, U.shape[-1])
