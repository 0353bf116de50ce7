#!/usr/bin/env python3
"""Additive KISS-GP regression on one MI355X through the gpytorch-shaped API: the model of the reference's
test/examples/test_kissgp_additive_regression.py, written as the test writes it -- ``AdditiveStructureKernel`` over a ``GridInterpolationKernel``
with ``num_dims=1`` (ONE one-dimensional grid of 100 nodes, every input column interpolated onto it) over ``ScaleKernel(RBFKernel(ard_num_dims=d))``
-- trained with Adam under the test's settings and evaluated on a held-out lattice.  The default is the test's own problem (a 20 x 20 lattice on
[0, 1]^2, y = sin(x0) + cos(x1) + noise / 20, mean absolute error below 0.2); ``--n`` and ``--d`` run the same model on a random cloud of n points
in d dimensions with the additive target sum_q sin(2 x_q + q), which is what the O(n d) product is for.

    python examples/kissgp_additive_regression.py
    python examples/kissgp_additive_regression.py --n 200000 --d 8 --iters 30
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpytorch_amd as gpytorch  # noqa: E402
from gpytorch_amd.kernels import AdditiveStructureKernel, GridInterpolationKernel, RBFKernel, ScaleKernel  # noqa: E402


class GPRegressionModel(gpytorch.models.ExactGP):
    def __init__(self, train_x, train_y, likelihood):
        super().__init__(train_x, train_y, likelihood)
        d = train_x.shape[-1]
        self.mean_module = gpytorch.means.ZeroMean()
        self.base_covar_module = ScaleKernel(RBFKernel(ard_num_dims=d))
        self.covar_module = AdditiveStructureKernel(GridInterpolationKernel(self.base_covar_module, grid_size=100, num_dims=1), num_dims=d)

    def forward(self, x):
        return gpytorch.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))


def lattice(n):
    t = torch.arange(n, dtype=torch.float32) / (n - 1)
    return torch.stack([t.repeat_interleave(n), t.repeat(n)], dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=0, help="0: the reference test's 20 x 20 lattice; otherwise a random cloud of n points")
    ap.add_argument("--d", type=int, default=2)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this example runs the HIP path: it needs a ROCm device"
    dev = torch.device("cuda:0")
    torch.manual_seed(args.seed)
    if args.n == 0:
        train_x, test_x = lattice(20), lattice(10)
        train_y = torch.sin(train_x[:, 0]) + torch.cos(train_x[:, 1])
        train_y = train_y + torch.randn_like(train_y).div_(20.0)
        test_y = torch.sin(test_x[:, 0]) + torch.cos(test_x[:, 1])
    else:
        def f(x):
            return torch.sin(2.0 * x + torch.arange(x.shape[-1])).sum(-1)

        train_x = torch.rand(args.n, args.d)
        train_y = f(train_x) + 0.1 * torch.randn(args.n)
        test_x = torch.rand(1000, args.d) * 0.9 + 0.05
        test_y = f(test_x)
    train_x, train_y, test_x, test_y = (t.to(dev) for t in (train_x, train_y, test_x, test_y))

    likelihood = gpytorch.likelihoods.GaussianLikelihood().to(dev)
    model = GPRegressionModel(train_x, train_y, likelihood).to(dev)
    mll = gpytorch.mlls.ExactMarginalLogLikelihood(likelihood, model)
    with gpytorch.settings.max_preconditioner_size(10), gpytorch.settings.max_cg_iterations(50), gpytorch.settings.fast_pred_var():
        model.train()
        likelihood.train()
        optimizer = torch.optim.Adam(model.parameters(), lr=args.lr)
        t0 = time.perf_counter()
        for i in range(args.iters):
            optimizer.zero_grad()
            loss = -mll(model(train_x), train_y)
            loss.backward()
            optimizer.step()
            print(f"  iter {i + 1}/{args.iters} - loss {loss.item():.3f}")
        torch.cuda.synchronize()
        train_s = time.perf_counter() - t0
        operator = type(model.covar_module(train_x)).__name__
        model.eval()
        likelihood.eval()
        with torch.no_grad():
            test_preds = likelihood(model(test_x)).mean
    mae = torch.mean(torch.abs(test_y - test_preds)).item()
    print(f"covariance operator {operator}, lengthscales {model.base_covar_module.base_kernel.lengthscale.reshape(-1).tolist()}")
    print(f"training {train_s:.2f} s for {args.iters} steps at n = {train_x.shape[0]}, d = {train_x.shape[1]}; test mean absolute error {mae:.4f}")
    if args.n == 0:
        assert mae < 0.2, "the reference test's bar"


if __name__ == "__main__":
    main()
