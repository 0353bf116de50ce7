"""Float64 dense reference of the linear model of coregionalisation, written from the textbook formulas (not from the library, not from the
reference's code):  K = sum_q theta_q kron(k_q(x1, x2), B_q), interleaved rows i*T + tau, with k_q = exp(-s/2) (RBF) or the Matern polynomial in
r = sqrt(2 nu s) times exp(-r), s = sum_k ((x_k - x'_k) / l_k)^2.  Autograd-visible, so the model tests differentiate through it."""
import torch


def radial(nu, s):
    """nu = None: RBF; 0.5, 1.5, 2.5: Matern."""
    if nu is None:
        return torch.exp(-0.5 * s)
    r = torch.sqrt(2.0 * nu * s + 1e-30)
    poly = {0.5: 1.0, 1.5: 1.0 + r, 2.5: 1.0 + r + r * r / 3.0}[nu]
    return poly * torch.exp(-r)


def member_k(nu, ls, x1, x2):
    """k_q(x1, x2) [n, m] in float64; ``ls``: a number or d values."""
    z1, z2 = x1.double() / torch.as_tensor(ls, dtype=torch.float64), x2.double() / torch.as_tensor(ls, dtype=torch.float64)
    return radial(nu, (z1.unsqueeze(1) - z2.unsqueeze(0)).pow(2).sum(-1))


def lcm_matrix(x1, x2, members):
    """members: (nu, lengthscale, theta, B_q [T, T]) per latent process -> [n T, m T]."""
    return sum(torch.kron(torch.as_tensor(th, dtype=torch.float64) * member_k(nu, ls, x1, x2), torch.as_tensor(bq, dtype=torch.float64))
               for nu, ls, th, bq in members)


def task_covar(factor, var):
    """B = F F^T + diag(v) (the index kernel's task covariance)."""
    return factor.double() @ factor.double().t() + torch.diag(var.double())
