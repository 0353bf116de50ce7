#!/usr/bin/env python3
"""KISS-GP regression in two dimensions on one MI355X through the gpytorch-shaped API (the reference's
examples/02_Scalable_Exact_GPs/KISSGP_Regression.ipynb, its 2-D part): ``GridInterpolationKernel`` over an RBF kernel on a grid from
``choose_grid_size``, Adam on the marginal log likelihood, predictions with LOVE variances -- and the same data under an exact ``RBFKernel`` model
beside it, so that the test errors of the approximation and of the kernel it approximates can be compared.

    python examples/kissgp_regression.py
    python examples/kissgp_regression.py --n 100000 --iters 20
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpytorch_amd as gpytorch  # noqa: E402


class GPRegressionModel(gpytorch.models.ExactGP):
    def __init__(self, train_x, train_y, likelihood, kiss: bool):
        super().__init__(train_x, train_y, likelihood)
        self.mean_module = gpytorch.means.ConstantMean()
        base = gpytorch.kernels.RBFKernel()
        if kiss:
            grid_size = gpytorch.utils.grid.choose_grid_size(train_x)
            base = gpytorch.kernels.GridInterpolationKernel(base, grid_size=grid_size, num_dims=2)
        self.covar_module = gpytorch.kernels.ScaleKernel(base)

    def forward(self, x):
        return gpytorch.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))


def fit_and_test(name, kiss, train_x, train_y, test_x, test_y, iters):
    dev = train_x.device
    likelihood = gpytorch.likelihoods.GaussianLikelihood().to(dev)
    model = GPRegressionModel(train_x, train_y, likelihood, kiss).to(dev)
    model.train()
    likelihood.train()
    optimizer = torch.optim.Adam(model.parameters(), lr=0.1)
    mll = gpytorch.mlls.ExactMarginalLogLikelihood(likelihood, model)
    t0 = time.perf_counter()
    for i in range(iters):
        optimizer.zero_grad()
        loss = -mll(model(train_x), train_y)
        loss.backward()
        optimizer.step()
        if i % 10 == 0 or i == iters - 1:
            print(f"  {name} iter {i + 1}/{iters} - loss {loss.item():.3f}")
    torch.cuda.synchronize()
    train_s = time.perf_counter() - t0
    model.eval()
    likelihood.eval()
    with torch.no_grad(), gpytorch.settings.fast_pred_var():
        pred = likelihood(model(test_x))
        mae = (pred.mean - test_y).abs().mean().item()
    print(f"{name}: covariance operator {type(model.covar_module(train_x)).__name__}, training {train_s:.2f} s, test MAE {mae:.4f}")
    return mae


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4000)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this example runs the HIP path: it needs a ROCm device"
    dev = torch.device("cuda:0")
    torch.manual_seed(args.seed)

    def f(x):
        return torch.sin(2 * math.pi * x[:, 0]) * torch.cos(1.5 * math.pi * x[:, 1])

    train_x = torch.rand(args.n, 2)
    train_y = f(train_x) + 0.1 * torch.randn(args.n)
    test_x = torch.rand(1000, 2) * 0.9 + 0.05
    test_y = f(test_x)
    train_x, train_y, test_x, test_y = (t.to(dev) for t in (train_x, train_y, test_x, test_y))
    mae_kiss = fit_and_test("KISS-GP", True, train_x, train_y, test_x, test_y, args.iters)
    mae_exact = fit_and_test("exact RBF", False, train_x, train_y, test_x, test_y, args.iters)
    print(f"test MAE: KISS-GP {mae_kiss:.4f}   exact RBFKernel {mae_exact:.4f}")


if __name__ == "__main__":
    main()
