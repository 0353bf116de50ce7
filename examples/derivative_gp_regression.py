#!/usr/bin/env python3
"""GP regression with derivative observations in two dimensions on one MI355X through the gpytorch-shaped API: the setting of the reference's
examples/08_Advanced_Usage/Simple_GP_Regression_Derivative_Information_2d.ipynb (Franke's function on the unit square, observed together with both
partial derivatives; ``RBFKernelGrad`` -- or, with ``--kernel matern52``, ``Matern52KernelGrad`` -- + ``ConstantMeanGrad`` + a three-task Gaussian likelihood, Adam on the marginal log likelihood), written for
this package.  The covariance over values and gradients is 3 n x 3 n; here it is one matrix-free operator, so ``--n`` may be large.  With
``--kernel rbf-gradgrad`` the two non-mixed second derivatives are observed as well (``RBFKernelGradGrad`` + ``ConstantMeanGradGrad`` + a five-task
likelihood: a 5 n x 5 n operator, still never formed).

    python examples/derivative_gp_regression.py                    # a 10 x 10 grid
    python examples/derivative_gp_regression.py --n 20000 --iters 10
    python examples/derivative_gp_regression.py --kernel matern52   # a prior that is twice, not infinitely, differentiable
    python examples/derivative_gp_regression.py --kernel rbf-gradgrad   # curvature data: d2f/dx2 and d2f/dy2 are observed too
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpytorch_amd as gpytorch  # noqa: E402


def franke(x, second=False):
    """Franke's function on [0, 1]^2 with its gradient by autograd: [n, 3] = (f, df/dx, df/dy); ``second``: [n, 5], d2f/dx2 and d2f/dy2 appended."""
    x = x.clone().requires_grad_(True)
    u, v = x[:, 0], x[:, 1]
    f = (0.75 * torch.exp(-((9 * u - 2) ** 2 + (9 * v - 2) ** 2) / 4) + 0.75 * torch.exp(-((9 * u + 1) ** 2) / 49 - (9 * v + 1) / 10)
         + 0.5 * torch.exp(-((9 * u - 7) ** 2 + (9 * v - 3) ** 2) / 4) - 0.2 * torch.exp(-((9 * u - 4) ** 2) - (9 * v - 7) ** 2))
    (grad,) = torch.autograd.grad(f.sum(), x, create_graph=second)
    cols = [f.detach().unsqueeze(-1), grad.detach()]
    if second:   # f is a sum over the points, so the gradient of the a-th gradient column holds d2f/dx_a^2 of every point in its a-th column
        cols += [torch.autograd.grad(grad[:, a].sum(), x, retain_graph=True)[0][:, a : a + 1] for a in range(2)]
    return torch.cat(cols, -1)


class GPModelWithDerivatives(gpytorch.models.ExactGP):
    def __init__(self, train_x, train_y, likelihood, kernel="rbf"):
        super().__init__(train_x, train_y, likelihood)
        self.mean_module = gpytorch.means.ConstantMeanGradGrad() if kernel == "rbf-gradgrad" else gpytorch.means.ConstantMeanGrad()
        self.base_kernel = KERNELS[kernel](ard_num_dims=2)
        self.covar_module = gpytorch.kernels.ScaleKernel(self.base_kernel)

    def forward(self, x):
        return gpytorch.distributions.MultitaskMultivariateNormal(self.mean_module(x), self.covar_module(x))


KERNELS = {"rbf": gpytorch.kernels.RBFKernelGrad, "matern52": gpytorch.kernels.Matern52KernelGrad, "rbf-gradgrad": gpytorch.kernels.RBFKernelGradGrad}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100, help="training points (100: a 10 x 10 grid; otherwise uniform in the unit square)")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--kernel", choices=sorted(KERNELS), default="rbf", help="the covariance over values and gradients (rbf-gradgrad: and second derivatives)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this example runs the fused HIP path: it needs a ROCm device"
    dev = torch.device("cuda:0")
    torch.manual_seed(args.seed)
    if args.n == 100:
        g1 = torch.linspace(0, 1, 10)
        train_x = torch.stack(torch.meshgrid(g1, g1, indexing="ij"), -1).reshape(-1, 2)
    else:
        train_x = torch.rand(args.n, 2)
    second = args.kernel == "rbf-gradgrad"
    tasks = 5 if second else 3
    train_y = franke(train_x, second)
    train_y = train_y + 0.05 * torch.randn(train_x.shape[0], tasks) * (train_y.std(0) if second else 1.0)   # (second derivatives of Franke's function reach 100)
    g2 = torch.linspace(0, 1, 25)
    test_x = torch.stack(torch.meshgrid(g2, g2, indexing="ij"), -1).reshape(-1, 2)
    test_y = franke(test_x, second)
    train_x, train_y, test_x = train_x.to(dev), train_y.to(dev), test_x.to(dev)

    likelihood = gpytorch.likelihoods.MultitaskGaussianLikelihood(num_tasks=tasks).to(dev)  # the value, two partial derivatives (and two second derivatives)
    model = GPModelWithDerivatives(train_x, train_y, likelihood, args.kernel).to(dev)
    print("covariance operator:", type(model.covar_module(train_x)).__name__, tuple(model.covar_module(train_x).shape))

    model.train()
    likelihood.train()
    optimizer = torch.optim.Adam(model.parameters(), lr=0.05)
    mll = gpytorch.mlls.ExactMarginalLogLikelihood(likelihood, model)
    t0 = time.perf_counter()
    for i in range(args.iters):
        optimizer.zero_grad()
        loss = -mll(model(train_x), train_y)
        loss.backward()
        ls = model.base_kernel.lengthscale.reshape(-1).tolist()
        print("Iter %d/%d - Loss: %.3f   lengthscales: %.3f, %.3f   noise: %.3f" % (i + 1, args.iters, loss.item(), ls[0], ls[1], likelihood.noise.item()))
        optimizer.step()
    torch.cuda.synchronize()
    print(f"training: {time.perf_counter() - t0:.2f} s")

    model.eval()
    likelihood.eval()
    with torch.no_grad(), gpytorch.settings.fast_pred_var():
        mean = likelihood(model(test_x)).mean.cpu()
    for k, name in enumerate(("f", "df/dx", "df/dy", "d2f/dx2", "d2f/dy2")[:tasks]):
        print(f"{name:6s} mean absolute error on the 25 x 25 grid: {(mean[:, k] - test_y[:, k]).abs().mean():.4f}")


if __name__ == "__main__":
    main()
