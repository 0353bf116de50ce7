"""float64 closed forms of the Newton-Girard additive covariance (Duvenaud's additive GP), the oracle of test_newton_girard_cpu.py /
test_gpu_newton_girard.py.  Written from the formula, not from any recursion the code under test uses:

    k(x, x') = sum_{n=1..R} sigma_n e_n(z_1 .. z_d),   z_q = k'(|x_q - x'_q| / lengthscale_q)   (tests/additive_ref.py ``add_terms``)

e_n, the n-th elementary symmetric polynomial, is the SUM OVER ALL n-SUBSETS of the product of their members (``itertools.combinations``): positive
terms only, no recursion, at most C(8, 4) = 70 products per order.  The native family evaluates k~ = k / S, S = sum_n sigma_n C(d, n) (``ng_norm``).
Derivatives come from autograd through these forms.
"""
import itertools
import math

import torch

from tests.additive_ref import FAMILIES, add_terms, base_cov, dim_dists  # noqa: F401


def esp(z, r):
    """[e_1 .. e_r] of the values along the last dimension of ``z`` (float64), by enumeration of the subsets."""
    d = z.shape[-1]
    out = []
    for n in range(1, r + 1):
        acc = torch.zeros_like(z[..., 0])
        for idx in itertools.combinations(range(d), n):
            acc = acc + z[..., list(idx)].prod(-1)
        out.append(acc)
    return out


def ng_norm(sigma, d):
    """S = sum_n sigma_n C(d, n) = k(x, x)."""
    sigma = torch.as_tensor(sigma, dtype=torch.float64).reshape(-1)
    return sum(sigma[n - 1] * math.comb(d, n) for n in range(1, sigma.numel() + 1))


def ng_cov(kind, x1, x2, ls, sigma, diag=False):
    """k [n, m] float64 ([n] with ``diag``); ``sigma``: the R outputscales; ``ls``: 1 or d lengthscales."""
    sigma = torch.as_tensor(sigma, dtype=torch.float64).reshape(-1)
    e = esp(add_terms(kind, x1, x2, ls, diag), sigma.numel())
    return sum(sigma[n] * e[n] for n in range(sigma.numel()))


def ng_cov_normalised(kind, x1, x2, ls, sigma, diag=False):
    """What the native family generates: k / S (unit diagonal)."""
    d = torch.as_tensor(x1).shape[-1]
    return ng_cov(kind, x1, x2, ls, sigma, diag) / ng_norm(sigma, d)


def ng_grad_sums(kind, x1, x2, ls, sigma, W, rc):
    """The 1 + d + rc bilinear-derivative sums of the native family's derivative kernel, formed densely in float64 (W [n, m] the weights):
        sums[0] = sum W k~;   sums[1 + q] = sum W (dk~/dz_q) (dk'/ds)(s_q) s_q;   sums[1 + d + n - 1] = sum W e_n,  n = 1..rc
    with k~ = k / S and s_q the squared scaled distance of dimension q.  Autograd delivers both derivatives: dk~/dz_q through the subset enumeration,
    and (dk'/ds) s = (1/2) dk'/du with rho = e^u (exactly zero where rho = 0: k' is flat in s there for RBF / Matern 3/2 / 5/2, and for Matern 1/2
    (dk'/ds) s = -rho e^-rho / 2 -> 0)."""
    x1, x2, W = torch.as_tensor(x1).double(), torch.as_tensor(x2).double(), torch.as_tensor(W).double()
    ls = torch.as_tensor(ls, dtype=torch.float64).reshape(-1)
    sigma = torch.as_tensor(sigma, dtype=torch.float64).reshape(-1)
    d, r = x1.shape[1], sigma.numel()
    S = ng_norm(sigma, d)
    rho = dim_dists(x1, x2, ls)
    u = rho.clamp_min(1e-300).log().requires_grad_(True)
    (dz_du,) = torch.autograd.grad(base_cov(kind, u.exp()).sum(), u)
    dzs = torch.where(rho > 0, 0.5 * dz_du, torch.zeros_like(dz_du))
    zr = base_cov(kind, rho).requires_grad_(True)
    e = esp(zr, rc)
    kt = sum(sigma[n] / S * e[n] for n in range(r))
    (dk_dz,) = torch.autograd.grad(kt.sum(), zr)
    sums = [(W * kt.detach()).sum()] + [(W * dk_dz[..., q] * dzs[..., q]).sum() for q in range(d)] + [(W * e[n].detach()).sum() for n in range(rc)]
    return torch.stack(sums)
