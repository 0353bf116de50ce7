"""float64 torch restatement of the product of two stationary covariance families over two column groups, the oracle of test_product_cpu.py /
test_gpu_product.py.  Written from the formulas (``gpytorch/kernels/rbf_kernel.py:68-85``, ``matern_kernel.py:85-110``, the elementwise product of
``kernels/kernel.py:634-688``), with plain differences instead of the reference's Gram-trick distance; derivatives come from autograd.

    k(x, x') = k_A(r_A) k_B(r_B),   r_F = |(x_F - x'_F) / lengthscale_F| over the columns of factor F
    RBF: exp(-r^2 / 2);   Matern nu: with u = sqrt(2 nu) r,  e^-u  (1/2),  (1 + u) e^-u  (3/2),  (1 + u + u^2 / 3) e^-u  (5/2)
"""
import torch

FAMILIES = ("rbf", "matern12", "matern32", "matern52")       # by family id 0..3
PAIRS = [(a, b) for a in range(4) for b in range(a, 4) if b > 0]   # the nine canonical pairs (K_A <= K_B, not both RBF)


def scaled_dist(x1, x2, ls):
    """Pairwise |x1_i / ls - x2_j / ls| in float64; zero differences get a zero (sub)gradient instead of NaN."""
    ls = torch.as_tensor(ls, dtype=torch.float64).reshape(1, -1)
    z1, z2 = torch.as_tensor(x1).double() / ls, torch.as_tensor(x2).double() / ls
    s = (z1.unsqueeze(1) - z2.unsqueeze(0)).pow(2).sum(-1)
    safe = torch.where(s > 0, s, torch.ones_like(s))
    return torch.where(s > 0, safe.sqrt(), torch.zeros_like(s))


def factor_cov(kind, x1, x2, ls):
    """One factor: K [n, m] float64 of family ``kind`` (a name or an id 0..3); ``ls``: 1 or d lengthscales."""
    kind = FAMILIES[kind] if isinstance(kind, int) else kind
    r = scaled_dist(x1, x2, ls)
    if kind == "rbf":
        return torch.exp(-0.5 * r * r)
    nu = {"matern12": 0.5, "matern32": 1.5, "matern52": 2.5}[kind]
    u = (2.0 * nu) ** 0.5 * r
    e = torch.exp(-u)
    return e if nu == 0.5 else ((1 + u) * e if nu == 1.5 else (1 + u + u * u / 3.0) * e)


def prod_cov(ka, kb, da, x1, x2, ls):
    """The product on GATHERED clouds [n, D_A + D_B] (columns of A first); ``ls``: D_A + D_B lengthscales, one per gathered column."""
    ls = torch.as_tensor(ls, dtype=torch.float64).reshape(-1)
    x1, x2 = torch.as_tensor(x1), torch.as_tensor(x2)
    return factor_cov(ka, x1[:, :da], x2[:, :da], ls[:da]) * factor_cov(kb, x1[:, da:], x2[:, da:], ls[da:])
