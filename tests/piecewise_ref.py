"""float64 torch restatement of the piecewise-polynomial covariance (Rasmussen & Williams eq. 4.21 as the reference EXECUTES it,
``gpytorch/kernels/piecewise_polynomial_kernel.py:11-28, 104-121``): the oracle of test_piecewise_cpu.py / test_gpu_piecewise.py.  Written from
the formulas, with plain differences instead of the reference's Gram-trick distance; derivatives come from autograd.

    k = max(1 - r, 0)^(j + q) P_q(r),   r = |(x - x') / lengthscale|,   j = floor(D / 2) + q + 1
    P_0 = 1,  P_1 = 1 + (j + 1) r,  P_2 = 1 + (j + 2) r + (j + 4 j + 3) / 3 r^2  (the executed coefficient, not the docstring's j^2 + 4 j + 3),
    P_3 = 1 + (j + 3) r + (6 j^2 + 36 j + 45) / 15 r^2 + (j^3 + 9 j^2 + 23 j + 15) / 15 r^3
"""
import torch


def pp_j(d: int, q: int) -> int:
    return d // 2 + q + 1


def pp_poly(r, j: int, q: int):
    if q == 0:
        return torch.ones_like(r)
    if q == 1:
        return 1 + (j + 1) * r
    if q == 2:
        return 1 + (j + 2) * r + (j + 4 * j + 3) / 3.0 * r * r
    if q == 3:
        return 1 + (j + 3) * r + (6 * j * j + 36 * j + 45) / 15.0 * r * r + (j ** 3 + 9 * j * j + 23 * j + 15) / 15.0 * r ** 3
    raise ValueError(q)


def pp_dist(x1, x2, ls):
    """Pairwise |x1_i / ls - x2_j / ls| in float64; zero differences get a zero (sub)gradient instead of NaN."""
    z1, z2 = x1.double() / ls.double().reshape(1, -1), x2.double() / ls.double().reshape(1, -1)
    s = (z1.unsqueeze(1) - z2.unsqueeze(0)).pow(2).sum(-1)
    safe = torch.where(s > 0, s, torch.ones_like(s))
    return torch.where(s > 0, safe.sqrt(), torch.zeros_like(s))


def pp_cov(x1, x2, ls, q: int, num_dims=None):
    """K [n, m] float64; ``ls``: 1 or d lengthscales (tensor); ``num_dims``: D of j when it is not the width of x1."""
    x1, x2 = torch.as_tensor(x1), torch.as_tensor(x2)
    ls = torch.as_tensor(ls, dtype=torch.float64)
    j = pp_j(x1.shape[-1] if num_dims is None else num_dims, q)
    r = pp_dist(x1, x2, ls)
    return (1 - r).clamp_min(0).pow(j + q) * pp_poly(r, j, q)
