"""float64 torch restatement of the product-structure covariance over a one-dimensional stationary base family, the oracle of
test_product_structure_cpu.py / test_gpu_product_structure.py.  Written from the formulas (``gpytorch/kernels/product_structure_kernel.py:70-76`` over
``rbf_kernel.py:68-85`` / ``matern_kernel.py:85-110``), with plain per-dimension differences instead of the reference's Gram-trick distance;
derivatives come from autograd.

    k(x, x') = prod_{q<d} k'(rho_q),   rho_q = |x_q - x'_q| / lengthscale_q
    RBF: exp(-rho^2 / 2);   Matern nu: with u = sqrt(2 nu) rho,  e^-u  (1/2),  (1 + u) e^-u  (3/2),  (1 + u + u^2 / 3) e^-u  (5/2)

With a Matern base this is the tensor-product (separable) Matern covariance; with the RBF base it is the RBF with per-dimension lengthscales.  An
outputscale s INSIDE the structure kernel scales each of the d factors: s^d in all."""
import torch

FAMILIES = ("rbf", "matern12", "matern32", "matern52")       # by family id 0..3
MATERN = FAMILIES[1:]                                         # the bases of the native family "ps"


def ps_terms(kind, x1, x2, ls, diag=False):
    """The d one-dimensional covariances k'(rho_q), [n, m, d] ([n, d] with ``diag``) in float64; ``ls``: 1 or d lengthscales (autograd-visible)."""
    kind = FAMILIES[kind] if isinstance(kind, int) else kind
    x1, x2 = torch.as_tensor(x1).double(), torch.as_tensor(x2).double()
    ls = torch.as_tensor(ls, dtype=torch.float64).reshape(1, -1)
    rho = ((x1 - x2) / ls).abs() if diag else ((x1.unsqueeze(1) - x2.unsqueeze(0)) / ls).abs()
    if kind == "rbf":
        return torch.exp(-0.5 * rho * rho)
    nu = {"matern12": 0.5, "matern32": 1.5, "matern52": 2.5}[kind]
    u = (2.0 * nu) ** 0.5 * rho
    e = torch.exp(-u)
    return e if nu == 0.5 else ((1 + u) * e if nu == 1.5 else (1 + u + u * u / 3.0) * e)


def ps_cov(kind, x1, x2, ls, diag=False):
    """The product-structure covariance prod_q k'(rho_q): K [n, m] float64 ([n] with ``diag``)."""
    return ps_terms(kind, x1, x2, ls, diag).prod(-1)
