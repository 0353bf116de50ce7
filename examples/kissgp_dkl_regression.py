#!/usr/bin/env python3
"""Deep kernel learning over KISS-GP on one MI355X through the gpytorch-shaped API (the structure of the reference's
examples/06_PyTorch_NN_Integration_DKL/KISSGP_Deep_Kernel_Regression_CUDA.ipynb on synthetic data): a multilayer perceptron maps the inputs to two
features, ``ScaleToBounds(-1, 1)`` scales them onto the grid, and ``ScaleKernel(GridInterpolationKernel(RBFKernel(ard_num_dims=2), grid_size=100))``
covers the features.  The features require grad, so the covariance stays ONE matrix-free operator and the marginal log likelihood hands the network
its gradient through the derivative-stencil kernel: network and GP hyper-parameters are trained jointly by Adam.

    python examples/kissgp_dkl_regression.py
    python examples/kissgp_dkl_regression.py --n 100000 --iters 30
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpytorch_amd as gpytorch  # noqa: E402

GRID_SIZE = 100
GRID_BOUNDS = [(-1.0, 1.0), (-1.0, 1.0)]


class LargeFeatureExtractor(torch.nn.Sequential):
    def __init__(self, data_dim):
        super().__init__()
        self.add_module("linear1", torch.nn.Linear(data_dim, 1000))
        self.add_module("relu1", torch.nn.ReLU())
        self.add_module("linear2", torch.nn.Linear(1000, 500))
        self.add_module("relu2", torch.nn.ReLU())
        self.add_module("linear3", torch.nn.Linear(500, 50))
        self.add_module("relu3", torch.nn.ReLU())
        self.add_module("linear4", torch.nn.Linear(50, 2))


class GPRegressionModel(gpytorch.models.ExactGP):
    def __init__(self, train_x, train_y, likelihood):
        super().__init__(train_x, train_y, likelihood)
        self.mean_module = gpytorch.means.ConstantMean()
        self.covar_module = gpytorch.kernels.ScaleKernel(gpytorch.kernels.GridInterpolationKernel(
            gpytorch.kernels.RBFKernel(ard_num_dims=2), grid_size=GRID_SIZE, num_dims=2, grid_bounds=GRID_BOUNDS))
        self.feature_extractor = LargeFeatureExtractor(train_x.size(-1))
        self.scale_to_bounds = gpytorch.utils.grid.ScaleToBounds(-1.0, 1.0)

    def forward(self, x):
        projected_x = self.scale_to_bounds(self.feature_extractor(x))      # the features: inside 0.95 x the grid's bounds
        return gpytorch.distributions.MultivariateNormal(self.mean_module(projected_x), self.covar_module(projected_x))


def make_data(n, data_dim=8, seed=0):
    """A smooth function of two hidden directions of the inputs, plus noise: (x [n, data_dim], y [n]) on the CPU."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(n, data_dim, generator=gen) * 2.0 - 1.0
    a = torch.randn(data_dim, 2, generator=torch.Generator().manual_seed(1234)) / math.sqrt(data_dim)
    u = torch.tanh(x @ a)
    y = torch.sin(3.0 * u[:, 0]) * torch.cos(2.0 * u[:, 1]) + 0.5 * u[:, 0] * u[:, 1] + 0.05 * torch.randn(n, generator=gen)
    return x, y


def build(train_x, train_y):
    dev = train_x.device
    likelihood = gpytorch.likelihoods.GaussianLikelihood().to(dev)
    model = GPRegressionModel(train_x, train_y, likelihood).to(dev)
    return model, likelihood


def make_optimizer(model, likelihood, lr=0.01):
    return torch.optim.Adam([
        {"params": model.feature_extractor.parameters()},
        {"params": model.covar_module.parameters()},
        {"params": model.mean_module.parameters()},
        {"params": likelihood.parameters()},
    ], lr=lr)


def train_step(model, likelihood, mll, optimizer, train_x, train_y):
    optimizer.zero_grad()
    loss = -mll(model(train_x), train_y)
    loss.backward()
    optimizer.step()
    return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this example runs the HIP path: it needs a ROCm device"
    dev = torch.device("cuda:0")
    torch.manual_seed(args.seed)
    x, y = make_data(args.n + 2000, seed=args.seed)
    train_x, train_y, test_x, test_y = (t.to(dev) for t in (x[: args.n], y[: args.n], x[args.n:], y[args.n:]))
    model, likelihood = build(train_x, train_y)
    model.train()
    likelihood.train()
    optimizer = make_optimizer(model, likelihood)
    mll = gpytorch.mlls.ExactMarginalLogLikelihood(likelihood, model)
    t0 = time.perf_counter()
    for i in range(args.iters):
        loss = train_step(model, likelihood, mll, optimizer, train_x, train_y)
        if i % 10 == 0 or i == args.iters - 1:
            print(f"  iter {i + 1}/{args.iters} - loss {loss.item():.3f}")
    torch.cuda.synchronize()
    train_s = time.perf_counter() - t0
    op = model.covar_module(model.scale_to_bounds(model.feature_extractor(train_x)))
    model.eval()
    likelihood.eval()
    with torch.no_grad(), gpytorch.settings.fast_pred_var():
        pred = likelihood(model(test_x))
        mae = (pred.mean - test_y).abs().mean().item()
    print(f"deep kernel KISS-GP: covariance operator {type(op).__name__}, training {train_s:.2f} s, test MAE {mae:.4f} "
          f"(predicting the mean of the training targets: {(test_y - train_y.mean()).abs().mean().item():.4f})")


if __name__ == "__main__":
    main()
