"""Float64 restatement of ADDITIVE KISS-GP written from the formulas alone, on top of ``tests/ski_ref.py``: the oracle of the additive SKI tests.

Input column q is interpolated onto its own one-dimensional axis q (``ski_ref.dense_w`` at d = 1):  W_add = [W_0 | W_1 | .. | W_{d-1}]  [n, sum m_q],
K_UU = blockdiag(T_0 .. T_{d-1}) with T_q the symmetric Toeplitz matrix of the base kernel's first column on axis q, and
K = scale W_add K_UU W_add^T = scale sum_q W_q T_q W_q^T.  ``grid``: the d axes (the reference's model passes d copies of one axis); ``cols``: one
column per axis, or ONE column shared by all axes.
"""
from __future__ import annotations

import math

import torch

from tests import ski_ref as R


def _cols(cols, d):
    return list(cols) * d if len(cols) == 1 else list(cols)


def dense_w_add(x: torch.Tensor, grid, return_boundary: bool = False):
    """W_add [n, sum m_q] in float64; the boundary mask is per point and axis, [n, d]."""
    parts = [R.dense_w(x[:, q], [g], return_boundary=True) for q, g in enumerate(grid)]
    W = torch.cat([p[0] for p in parts], dim=1)
    return (W, torch.stack([p[1] for p in parts], dim=1)) if return_boundary else W


def k_uu_add(cols, d=None) -> torch.Tensor:
    return torch.block_diag(*[R.toeplitz(c) for c in _cols(cols, len(cols) if d is None else d)])


def kuu_add_matmul(cols, sizes, U: torch.Tensor) -> torch.Tensor:
    """blockdiag(T_q) @ U for U [sum m_q, t], block by block."""
    cs = _cols(cols, len(sizes))
    out, o = [], 0
    for c, m in zip(cs, sizes):
        out.append(R.toeplitz(c.double()) @ U[o: o + m].double())
        o += m
    return torch.cat(out)


def k_ski_add(x1, x2, grid, cols, scale=None) -> torch.Tensor:
    K = dense_w_add(x1, grid) @ k_uu_add(cols, len(grid)) @ dense_w_add(x2, grid).T
    return K if scale is None else K * scale.double().reshape(())


def mll(x, y, grid, cols, scale, noise, mean=0.0) -> torch.Tensor:
    """The exact marginal log likelihood PER DATUM by dense Cholesky."""
    n = x.shape[0]
    K = k_ski_add(x, x, grid, cols, scale) + noise.double().reshape(()) * torch.eye(n, dtype=torch.float64)
    L = torch.linalg.cholesky(K)
    r = (y.double() - mean).unsqueeze(-1)
    quad = (r * torch.cholesky_solve(r, L)).sum()
    return (-0.5 * (quad + 2.0 * L.diagonal().log().sum() + n * math.log(2.0 * math.pi))) / n


def posterior(x, y, xs, grid, cols, scale, noise, mean=0.0):
    """(mean, covariance of f) at the test points xs by dense Cholesky."""
    n = x.shape[0]
    K = k_ski_add(x, x, grid, cols, scale) + noise.double().reshape(()) * torch.eye(n, dtype=torch.float64)
    Ks = k_ski_add(xs, x, grid, cols, scale)
    Kss = k_ski_add(xs, xs, grid, cols, scale)
    L = torch.linalg.cholesky(K)
    mu = mean + (Ks @ torch.cholesky_solve((y.double() - mean).unsqueeze(-1), L)).squeeze(-1)
    return mu, Kss - Ks @ torch.cholesky_solve(Ks.T, L)
