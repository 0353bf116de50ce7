"""Float64 restatement of the symmetrized-KL covariance over Gaussian inputs x = [mu (d) | log sigma^2 (d)], written from the formulas:
    a = 1e-8 + exp(log sigma^2),  b = 1 / a
    SKL(x, x') = 1/2 sum_q [ a_q / a'_q + a'_q / a_q - 2 + (mu_q - mu'_q)^2 (b_q + b'_q) ],      k = exp(-SKL / l)
and, for F = sum_ij W_ij k_ij, its closed-form derivatives.  A reference only: pinned to the reference's own outputs by tests/test_skl_cpu.py."""
import torch

EPS = 1e-8


def skl_S(X1, X2):
    """SKL [n, m] of float64 clouds."""
    d = X1.shape[-1] // 2
    m1, a1 = X1[:, None, :d], EPS + X1[:, None, d:].exp()
    m2, a2 = X2[None, :, :d], EPS + X2[None, :, d:].exp()
    return 0.5 * (a1 / a2 + a2 / a1 - 2.0 + (m1 - m2) ** 2 * (1.0 / a1 + 1.0 / a2)).sum(-1)


def skl_K(X1, X2, ls):
    return torch.exp(-skl_S(X1, X2) / ls)


def skl_grad_sums(X1, X2, ls, W):
    """(G0 = sum W k, G1 = sum W k (2 SKL), g_mu [n, d] = dF/dmu of X1's points, g_a [n, d] = dF/da of X1's points) for F = sum W k."""
    d = X1.shape[-1] // 2
    m1, a1 = X1[:, None, :d], EPS + X1[:, None, d:].exp()
    m2, a2 = X2[None, :, :d], EPS + X2[None, :, d:].exp()
    WK = (W * skl_K(X1, X2, ls))[..., None]
    dm = m1 - m2
    g_mu = -(WK * dm * (1.0 / a1 + 1.0 / a2)).sum(1) / ls
    g_a = -(WK * (1.0 / a2 - (a2 + dm ** 2) / a1 ** 2)).sum(1) / (2.0 * ls)
    return WK.sum(), (WK[..., 0] * 2.0 * skl_S(X1, X2)).sum(), g_mu, g_a


def central_difference(f, x, h=1e-6):
    """df/dx of a scalar function of a float64 tensor, entry by entry."""
    g = torch.zeros_like(x)
    for i in range(x.numel()):
        e = torch.zeros_like(x)
        e.view(-1)[i] = h
        g.view(-1)[i] = (f(x + e) - f(x - e)) / (2.0 * h)
    return g
