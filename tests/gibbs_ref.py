"""Float64 oracle of the Gibbs covariance, written from the formula (not from the library, not from the reference's code):

    k(x, x') = sqrt(2 l l' / (l^2 + l'^2)) exp(-|x - x'|^2 / (l^2 + l'^2)),   l = l(x), l' = l(x')

with squared distances by direct differences.  The exponent of the prefactor is 1/2 for every d, as ``gpytorch/kernels/gibbs_kernel.py`` executes it.
``field`` is the closed-form positive lengthscale field the golden fixture (tests/golden/make_gibbs_golden.py) is generated with."""
import torch


def field(x):
    """A smooth positive lengthscale field l(x) in [0.08, 0.32], [..., n, d] -> [..., n, 1], in the dtype of x."""
    return 0.2 + 0.12 * torch.sin(3.0 * x.sum(-1, keepdim=True) + 0.5)


class MLP(torch.nn.Module):
    """d -> 8 -> 1 Softplus network plus a floor, seeded: a learnable ``lengthscale_fn`` that is positive for any weights."""

    def __init__(self, d=1, seed=0, dtype=torch.float32, floor=0.05, w2_scale=0.3, b2=-1.0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.w1 = torch.nn.Parameter(torch.randn(d, 8, generator=g, dtype=dtype))
        self.b1 = torch.nn.Parameter(torch.randn(8, generator=g, dtype=dtype))
        self.w2 = torch.nn.Parameter(w2_scale * torch.randn(8, 1, generator=g, dtype=dtype))
        self.b2 = torch.nn.Parameter(torch.full((1,), b2, dtype=dtype))
        self.floor = floor

    def forward(self, x):
        h = torch.nn.functional.softplus(x @ self.w1 + self.b1)
        return torch.nn.functional.softplus(h @ self.w2 + self.b2) + self.floor


def _f64(*ts):
    return [t.detach().to(device="cpu", dtype=torch.float64) for t in ts]


def gibbs_k(x1, l1, x2, l2):
    """K [n, m] in float64 from points [n, d], [m, d] and lengthscales [n] or [n, 1], [m] or [m, 1] (autograd-visible in every argument)."""
    l1, l2 = l1.reshape(-1, 1), l2.reshape(1, -1)
    s = (x1.unsqueeze(1) - x2.unsqueeze(0)).square().sum(-1)
    S = l1 * l1 + l2 * l2
    return torch.sqrt(2.0 * l1 * l2 / S) * torch.exp(-s / S)


def gibbs_K(x1, l1, x2=None, l2=None):
    """K in float64 on the CPU, whatever the arguments' dtype and device; one cloud when x2 is None."""
    x1, l1 = _f64(x1, l1)
    x2, l2 = (x1, l1) if x2 is None else _f64(x2, l2)
    return gibbs_k(x1, l1, x2, l2)


def gibbs_diag(x1, l1, x2, l2):
    """k(x1[i], x2[i]) in float64 on the CPU."""
    x1, l1, x2, l2 = _f64(x1, l1, x2, l2)
    l1, l2 = l1.reshape(-1), l2.reshape(-1)
    S = l1 * l1 + l2 * l2
    return torch.sqrt(2.0 * l1 * l2 / S) * torch.exp(-(x1 - x2).square().sum(-1) / S)


def prefactor(l1, l2):
    """sqrt(2 l l' / (l^2 + l'^2)) [n, m] in float64."""
    l1, l2 = _f64(l1, l2)
    l1, l2 = l1.reshape(-1, 1), l2.reshape(1, -1)
    return torch.sqrt(2.0 * l1 * l2 / (l1 * l1 + l2 * l2))


def gibbs_grad_sums(x1, l1, x2, l2, W):
    """(G0, g1 [n], g2 [m]) by float64 autograd: G0 = sum W o K, g1[i] = d G0 / d l1[i], g2[j] = d G0 / d l2[j], the two clouds' lengthscales taken as
    INDEPENDENT variables (for one cloud against itself the total derivative is g1 + g2)."""
    x1, l1, x2, l2, W = _f64(x1, l1, x2, l2, W)
    l1 = l1.reshape(-1).clone().requires_grad_(True)
    l2 = l2.reshape(-1).clone().requires_grad_(True)
    g0 = (W * gibbs_k(x1, l1, x2, l2)).sum()
    g1, g2 = torch.autograd.grad(g0, (l1, l2))
    return g0.detach(), g1, g2
