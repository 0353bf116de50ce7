"""Float64 restatement of the spectral-mixture covariance and of its bilinear-derivative sums, written from the formulas (the oracle of
tests/test_sm_cpu.py and tests/test_gpu_sm.py; no project code).

    k(x, x') = prod_{j<d} f_j,   f_j = sum_{q<Q} w_q e_qj g_qj,   e_qj = exp(-2 pi^2 sigma_qj^2 tau_j^2),  g_qj = cos(2 pi mu_qj tau_j),  tau = x - x'

(the sum over the mixtures BEFORE the product over the dimensions: what the reference executes).  x: [n, d]; w: [Q]; mu, sigma: [Q, d]."""
import math

import torch

TWO_PI = 2.0 * math.pi


def _terms(x1, x2, mu, sigma):
    tau = (x1.double().unsqueeze(1) - x2.double().unsqueeze(0)).unsqueeze(0)        # [1, n, m, d]
    mu, sigma = mu.double().reshape(mu.shape[0], 1, 1, -1), sigma.double().reshape(sigma.shape[0], 1, 1, -1)
    e = torch.exp(-2.0 * math.pi ** 2 * sigma ** 2 * tau ** 2)
    return tau, e, torch.cos(TWO_PI * mu * tau), torch.sin(TWO_PI * mu * tau)     # [Q, n, m, d] each (tau: [1, n, m, d])


def sm_cov(x1, x2, w, mu, sigma):
    """K [n, m] in float64."""
    _, e, g, _ = _terms(x1, x2, mu, sigma)
    return (w.double().reshape(-1, 1, 1, 1) * e * g).sum(0).prod(-1)


def sm_sums(x1, x2, w, mu, sigma, W):
    """(sum W k, A, B, C, absA, absB, absC) for a weight matrix W [n, m]; A, B, C: [Q, d],
        A_qj = sum W rest_j e g,   B_qj = sum W rest_j w_q e tau_j^2 g,   C_qj = sum W rest_j w_q e tau_j sn,   rest_j = prod_{j' != j} f_j'
    and abs*: the same sums over |summand| (what a relative bound on a cancelling sum has to be read against)."""
    tau, e, g, sn = _terms(x1, x2, mu, sigma)
    wq = w.double().reshape(-1, 1, 1, 1)
    f = (wq * e * g).sum(0)                                                        # [n, m, d]
    d = f.shape[-1]
    rest = torch.stack([torch.cat([f[..., :j], f[..., j + 1:]], -1).prod(-1) for j in range(d)], -1)   # [n, m, d]
    Wd = W.double().unsqueeze(-1)
    ta, tb, tc = Wd * rest * e * g, Wd * rest * wq * e * tau ** 2 * g, Wd * rest * wq * e * tau * sn
    s = lambda v: v.sum((1, 2))  # noqa: E731
    return float((W.double() * f.prod(-1)).sum()), s(ta), s(tb), s(tc), s(ta.abs()), s(tb.abs()), s(tc.abs())


def sm_param_grads(A, B, C, sigma):
    """d/dw [Q], d/dmu [Q, d], d/dsigma [Q, d] of sum W k from the sums."""
    return A.sum(-1), -TWO_PI * C, -4.0 * math.pi ** 2 * sigma.double() * B
