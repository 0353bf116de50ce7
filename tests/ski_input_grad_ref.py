"""Float64 restatement of the INPUT gradients of KISS-GP, written from the formulas alone with dense W and dW: the oracle of the input-gradient tests
(the companion of ``tests/ski_ref.py``, whose rule and node order it shares).

K = s W_1 K_UU W_2^T.  For a bilinear form B = sum_c l_c^T K r_c:

    dB/dx1[p, a] = sum_c l_c[p] sum_k (dw_pk / dx_a) G_R[c][node_pk],   G_R = s K_UU W_2^T R
    dB/dx2[q, a] = sum_c r_c[q] sum_k (dw_qk / dx_a) G_L[c][node_qk],   G_L = s K_UU W_1^T L

and their sum where x1 is x2.  dw_pk / dx_a = the u'-weight on axis a times the plain weights on the other axes.  Per axis the stencil arguments are
a = r + 1, r, 1 - r, 2 - r with da/dr = +1, +1, -1, -1 and dr/dx = 1 / h; inner'(a) = (4.5 a - 5) a for the two middle positions, outer'(a) =
(-1.5 a + 5) a - 4 for the two outer ones.  An axis on which the point takes the boundary rule (one-hot weights) contributes zero on that axis only.
"""
from __future__ import annotations

import math

import torch

from tests import ski_ref as R


def axis_weights(x: torch.Tensor, g0: float, h: float, m: int):
    """One axis, coordinates x [n] (float64): (clamped base [n], weights [n, 4], derivative weights d/dx [n, 4], boundary mask [n])."""
    s = (x - g0) / h
    f = torch.floor(s)
    r = s - f
    b = f.to(torch.int64) - 1
    a = torch.stack([r + 1.0, r, 1.0 - r, 2.0 - r], dim=-1)
    inner, outer = ((1.5 * a - 2.5) * a) * a + 1.0, ((-0.5 * a + 2.5) * a - 4.0) * a + 2.0
    dinner, douter = (4.5 * a - 5.0) * a, (-1.5 * a + 5.0) * a - 4.0
    mid = torch.tensor([False, True, True, False])
    sign = torch.tensor([1.0, 1.0, -1.0, -1.0], dtype=torch.float64)
    w = torch.where(mid, inner, outer)
    dw = torch.where(mid, dinner, douter) * sign / h
    left, right = b < 0, b > m - 4
    near_left = (s > 0.5).to(torch.int64)                      # the nearest of the first four nodes: node 0 or node 1
    near_right = 2 + (s > m - 1.5).to(torch.int64)             # the nearest of the last four: stencil position 2 or 3
    edge = left | right
    onehot = torch.nn.functional.one_hot(torch.where(left, near_left, near_right), 4).to(torch.float64)
    w = torch.where(edge.unsqueeze(-1), onehot, w)
    dw = torch.where(edge.unsqueeze(-1), torch.zeros_like(dw), dw)
    return b.clamp(0, m - 4), w, dw, edge


def dense_w_dw(x: torch.Tensor, grid):
    """(W [n, M], dW [n, d, M], boundary [n, d]) in float64 for points x [n, d] (float32-exact or float64 values); node order: axis 0 slowest."""
    g0, h, m = R.grid_numbers(grid)
    d = len(grid)
    x = x.double().reshape(-1, d)
    n = x.shape[0]
    axes = [axis_weights(x[:, i], g0[i], h[i], m[i]) for i in range(d)]
    M = math.prod(m)
    W = torch.zeros(n, M, dtype=torch.float64)
    dW = torch.zeros(n, d, M, dtype=torch.float64)
    rows = torch.arange(n)
    for k in range(4 ** d):
        o = [(k // 4 ** (d - 1 - i)) % 4 for i in range(d)]
        idx = torch.zeros(n, dtype=torch.int64)
        for i in range(d):
            idx = idx * m[i] + axes[i][0] + o[i]
        val = torch.ones(n, dtype=torch.float64)
        for i in range(d):
            val = val * axes[i][1][:, o[i]]
        W[rows, idx] += val
        for a in range(d):
            dv = torch.ones(n, dtype=torch.float64)
            for i in range(d):
                dv = dv * (axes[i][2] if i == a else axes[i][1])[:, o[i]]
            dW[rows, a, idx] += dv
    return W, dW, torch.stack([ax[3] for ax in axes], dim=-1)


def contract(dW: torch.Tensor, G: torch.Tensor, C: torch.Tensor):
    """dX[p, a] = sum_c C[c, p] sum_k dW[p, a, k] G[c, k] and its magnitude A[p, a] = sum_c |C| sum_k |dW| |G|; G [t, M], C [t, n]."""
    G, C = G.double(), C.double()
    val = torch.einsum("cp,pak,ck->pa", C, dW, G)
    mag = torch.einsum("cp,pak,ck->pa", C.abs(), dW.abs(), G.abs())
    return val, mag


def bilinear_input_grads(x1, x2, grid, cols, scale, L, Rm):
    """(dB/dx1 [n, d], dB/dx2 [m, d]) of B = sum_c l_c^T (s W_1 K_UU W_2^T) r_c for L [n, t], R [m, t]; ``x2 is x1``: both are returned separately
    (the gradient of the shared input is their sum)."""
    W1, dW1, _ = dense_w_dw(x1, grid)
    W2, dW2, _ = (W1, dW1, None) if x2 is x1 else dense_w_dw(x2, grid)
    s = 1.0 if scale is None else float(scale)
    cols = [c.detach().double() for c in cols]
    G_R = s * R.kuu_matmul(cols, W2.T @ Rm.double()).T           # [t, M]
    G_L = s * R.kuu_matmul(cols, W1.T @ L.double()).T
    return contract(dW1, G_R, L.double().T)[0], contract(dW2, G_L, Rm.double().T)[0]


def mll_feature_grads(z, y, grid, cols, scale, noise, mean=0.0):
    """(mll per datum, d mll / d z [n, d]) of the exact marginal log likelihood of y under K = s W K_UU W^T + noise I at the features z, by dense
    Cholesky: d mll / d K = (alpha alpha^T - K^-1) / (2 n), a symmetric D, so B = tr(D K) with L = D, R = I and both sides moving the point."""
    n = z.shape[0]
    W, dW, _ = dense_w_dw(z, grid)
    s, cols = float(scale), [c.detach().double() for c in cols]
    KW = s * R.kuu_matmul(cols, W.T)                             # [M, n] = s K_UU W^T
    K = W @ KW + float(noise) * torch.eye(n, dtype=torch.float64)
    Lc = torch.linalg.cholesky(K)
    r = (y.double() - mean).unsqueeze(-1)
    alpha = torch.cholesky_solve(r, Lc)
    val = -0.5 * ((r * alpha).sum() + 2.0 * Lc.diagonal().log().sum() + n * math.log(2.0 * math.pi)) / n
    D = (alpha @ alpha.T - torch.cholesky_inverse(Lc)) / (2.0 * n)
    dz = 2.0 * torch.einsum("pak,kp->pa", dW, KW @ D)            # column p of s K_UU W^T D: the grid vector of the coefficient one-hot at p
    return val, dz
