"""float64 torch restatement of the first-order additive covariance over a one-dimensional stationary base family, the oracle of
test_additive_cpu.py / test_gpu_additive.py.  Written from the formulas (``gpytorch/kernels/additive_structure_kernel.py:62-68`` over
``rbf_kernel.py:68-85`` / ``matern_kernel.py:85-110``), with plain per-dimension differences instead of the reference's Gram-trick distance;
derivatives come from autograd.

    k(x, x') = sum_{q<d} k'(rho_q),   rho_q = |x_q - x'_q| / lengthscale_q
    RBF: exp(-rho^2 / 2);   Matern nu: with u = sqrt(2 nu) rho,  e^-u  (1/2),  (1 + u) e^-u  (3/2),  (1 + u + u^2 / 3) e^-u  (5/2)

The library's native family evaluates the MEAN over the d terms (``add_mean``); the caller's scale carries d x outputscale.

Two layers.  ``add_cov`` / ``add_terms`` / ``add_mean`` are the CLOSED FORM in float64: exact to rounding, the oracle of the device tests.
``ref_add_cov`` restates the reference's EXECUTED arithmetic -- inputs divided by the lengthscale of their dimension (Matern: centred first), every
dimension a batch member [d, n, 1], distances through oracle/kernels.py's restatement of ``sq_dist`` / ``dist`` (Gram-trick expansion; ``torch.cdist``
for two different inputs) -- in the dtype of its inputs; it is what tests/test_additive_cpu.py pins to the reference's own outputs at the fixture
bounds.  The two differ by the rounding of the reference's distance: the Gram-trick squared distance is off by delta ~ 4 eps (|z|^2 + |z'|^2), the
distance by delta / (2 rho), which Matern-1/2 (slope -1 at rho = 0) passes on undamped -- 2.5e-12 on an 18 x 26 float64 cloud in three dimensions.
"""
import math

import torch

from oracle import kernels as OK

FAMILIES = ("rbf", "matern12", "matern32", "matern52")       # by family id 0..3


def dim_dists(x1, x2, ls, diag=False):
    """rho [n, m, d] (or [n, d] with ``diag``) in float64: per-dimension |x1_iq - x2_jq| / ls_q; ``ls``: 1 or d lengthscales."""
    x1, x2 = torch.as_tensor(x1).double(), torch.as_tensor(x2).double()
    ls = torch.as_tensor(ls, dtype=torch.float64).reshape(1, -1)
    if diag:
        return ((x1 - x2) / ls).abs()
    return ((x1.unsqueeze(1) - x2.unsqueeze(0)) / ls).abs()


def base_cov(kind, rho):
    """k'(rho) of family ``kind`` (a name or an id 0..3), elementwise."""
    kind = FAMILIES[kind] if isinstance(kind, int) else kind
    if kind == "rbf":
        return torch.exp(-0.5 * rho * rho)
    nu = {"matern12": 0.5, "matern32": 1.5, "matern52": 2.5}[kind]
    u = (2.0 * nu) ** 0.5 * rho
    e = torch.exp(-u)
    return e if nu == 0.5 else ((1 + u) * e if nu == 1.5 else (1 + u + u * u / 3.0) * e)


def add_terms(kind, x1, x2, ls, diag=False):
    """The d one-dimensional covariances, [n, m, d] ([n, d] with ``diag``)."""
    return base_cov(kind, dim_dists(x1, x2, ls, diag))


def add_cov(kind, x1, x2, ls, diag=False):
    """The additive covariance sum_q k'(rho_q): K [n, m] float64 ([n] with ``diag``)."""
    return add_terms(kind, x1, x2, ls, diag).sum(-1)


def add_mean(kind, x1, x2, ls, diag=False):
    """What the native family generates: the mean of the d terms (unit diagonal)."""
    return add_terms(kind, x1, x2, ls, diag).mean(-1)


def ref_add_cov(kind, x1, x2, ls, diag=False):
    """The additive covariance as the reference executes it, in the dtype of ``x1``: K [n, m] ([n] with ``diag``); ``ls`` shaped [1, 1] or [1, d]."""
    kind = FAMILIES[kind] if isinstance(kind, int) else kind
    x1, x2 = torch.as_tensor(x1), torch.as_tensor(x2)
    ls = torch.as_tensor(ls, dtype=x1.dtype).reshape(1, -1)
    if kind != "rbf":
        mean = x1.mean(dim=-2, keepdim=True)
        x1, x2 = x1 - mean, x2 - mean
    t1, t2 = x1.div(ls).transpose(-1, -2).unsqueeze(-1), x2.div(ls).transpose(-1, -2).unsqueeze(-1)     # [d, n, 1]
    same = t1.shape == t2.shape and torch.equal(t1, t2)
    if diag:
        r = torch.zeros(t1.shape[:-1], dtype=t1.dtype) if same else torch.linalg.norm(t1 - t2, dim=-1)
        sq = r if same else r.pow(2)
    elif kind == "rbf":
        sq = OK.sq_dist(t1, t2, same)
    else:
        r = OK.dist(t1, t2, same)
    if kind == "rbf":
        return sq.div(-2.0).exp().sum(-2 if diag else -3)
    nu = {"matern12": 0.5, "matern32": 1.5, "matern52": 2.5}[kind]
    e = torch.exp(-math.sqrt(nu * 2) * r)
    poly = 1 if nu == 0.5 else ((math.sqrt(3) * r).add(1) if nu == 1.5 else (math.sqrt(5) * r).add(1).add(5.0 / 3.0 * r ** 2))
    return (poly * e).sum(-2 if diag else -3)
