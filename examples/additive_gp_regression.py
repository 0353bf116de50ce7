#!/usr/bin/env python3
"""First-order additive GP regression on one MI355X through the gpytorch-shaped API: f(x) = sum_q f_q(x_q) in d = 6 dimensions with
``AdditiveStructureKernel`` over an ARD Matern-5/2 base -- the model of the reference's "Kernels with Additive or Product Structure" material.  The
reference sums a d x n x n tensor; here the kernel is one matrix-free operator (d one-dimensional covariances per pair of points, summed in
registers, one contraction), so a few thousand points train through mBCG + SLQ and predict with LOVE variances like any other exact GP.

    python examples/additive_gp_regression.py                      # n = 4000, d = 6
    python examples/additive_gp_regression.py --n 50000 --iters 10
"""
import argparse
import math
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpytorch_amd as gpytorch  # noqa: E402


class AdditiveGPModel(gpytorch.models.ExactGP):
    def __init__(self, train_x, train_y, likelihood):
        super().__init__(train_x, train_y, likelihood)
        d = train_x.shape[-1]
        self.mean_module = gpytorch.means.ConstantMean()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)   # (the reference deprecates the class name, not the model)
            self.covar_module = gpytorch.kernels.ScaleKernel(
                gpytorch.kernels.AdditiveStructureKernel(gpytorch.kernels.MaternKernel(nu=2.5, ard_num_dims=d), num_dims=d))

    def forward(self, x):
        return gpytorch.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))


def target(x):
    """A sum of one-dimensional effects of different smoothness, one per input dimension."""
    parts = [torch.sin(2 * math.pi * x[:, 0]), (x[:, 1] - 0.5).abs() * 2, x[:, 2] ** 2, torch.cos(3 * math.pi * x[:, 3]) * 0.5,
             torch.tanh(6 * (x[:, 4] - 0.5)), 0.2 * x[:, 5]]
    return sum(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4000)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this example runs the fused HIP path: it needs a ROCm device"
    dev = torch.device("cuda:0")
    torch.manual_seed(args.seed)
    d = 6
    train_x = torch.rand(args.n, d)
    train_y = target(train_x) + 0.1 * torch.randn(args.n)
    test_x = torch.rand(500, d)
    test_y = target(test_x)
    train_x, train_y, test_x, test_y = train_x.to(dev), train_y.to(dev), test_x.to(dev), test_y.to(dev)

    likelihood = gpytorch.likelihoods.GaussianLikelihood().to(dev)
    model = AdditiveGPModel(train_x, train_y, likelihood).to(dev)
    op = model.covar_module(train_x)
    print("covariance operator:", type(op).__name__, "of family", op.spec.kind)

    model.train()
    likelihood.train()
    optimizer = torch.optim.Adam(model.parameters(), lr=0.1)
    mll = gpytorch.mlls.ExactMarginalLogLikelihood(likelihood, model)
    t0 = time.perf_counter()
    for i in range(args.iters):
        optimizer.zero_grad()
        loss = -mll(model(train_x), train_y)
        loss.backward()
        print("Iter %d/%d - Loss: %.3f" % (i + 1, args.iters, loss.item()))
        optimizer.step()
    torch.cuda.synchronize()
    print(f"training: {time.perf_counter() - t0:.2f} s")
    print("lengthscales:", [round(v, 3) for v in model.covar_module.base_kernel.base_kernel.lengthscale.detach().reshape(-1).tolist()])

    model.eval()
    likelihood.eval()
    with torch.no_grad(), gpytorch.settings.fast_pred_var():
        pred = likelihood(model(test_x))
        lower, upper = pred.confidence_region()
    rmse = float((pred.mean - test_y).pow(2).mean().sqrt())
    inside = float(((test_y >= lower) & (test_y <= upper)).float().mean())
    print(f"test RMSE {rmse:.4f} (noise 0.1), {100 * inside:.1f} % of the noise-free targets inside the 95 % region")


if __name__ == "__main__":
    main()
