#!/usr/bin/env python3
"""Tensor-product (separable) Matern-5/2 GP regression on one MI355X through the gpytorch-shaped API: k(x, x') = prod_q k'(x_q, x'_q) in d = 6
dimensions with ``ProductStructureKernel`` over an ARD Matern-5/2 base -- the default covariance of computer-experiment emulators (kriging).  The
reference multiplies a d x n x n tensor down; here the kernel is one matrix-free operator (one exponential per pair of points whatever d, the d
polynomials multiplied in registers, one contraction), so a few thousand points train through mBCG + SLQ and predict with LOVE variances like any
other exact GP.

    python examples/product_structure_gp_regression.py                      # n = 4000, d = 6
    python examples/product_structure_gp_regression.py --n 50000 --iters 10
    python examples/product_structure_gp_regression.py --dense              # the comparison: the same model formed densely (``kernels.ps_dense``)
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


class ProductStructureGPModel(gpytorch.models.ExactGP):
    def __init__(self, train_x, train_y, likelihood):
        super().__init__(train_x, train_y, likelihood)
        d = train_x.shape[-1]
        self.mean_module = gpytorch.means.ConstantMean()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)   # (the reference deprecates the class name, not the model)
            self.covar_module = gpytorch.kernels.ScaleKernel(
                gpytorch.kernels.ProductStructureKernel(gpytorch.kernels.MaternKernel(nu=2.5, ard_num_dims=d), num_dims=d))

    def forward(self, x):
        return gpytorch.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))


def target(x):
    """A simulator-like response: a product of one-dimensional effects plus a weak additive trend."""
    prod = torch.sin(math.pi * x[:, 0]) * (0.5 + x[:, 1]) * torch.cos(1.5 * x[:, 2]) * (1.0 + 0.5 * torch.tanh(4 * (x[:, 3] - 0.5)))
    return 2.0 * prod + 0.3 * x[:, 4] - 0.2 * x[:, 5] ** 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4000)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dense", action="store_true", help="form the covariance densely (kernels.ps_dense) instead of the native family")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this example runs the fused HIP path: it needs a ROCm device"
    dev = torch.device("cuda:0")
    torch.manual_seed(args.seed)
    if args.dense:   # the rule that selects the native family says no: every call takes the dense branch
        gpytorch.kernels.ps_native = lambda *a, **k: False
    d = 6
    train_x = torch.rand(args.n, d)
    train_y = target(train_x) + 0.05 * torch.randn(args.n)
    test_x = torch.rand(500, d)
    test_y = target(test_x)
    train_x, train_y, test_x, test_y = train_x.to(dev), train_y.to(dev), test_x.to(dev), test_y.to(dev)

    likelihood = gpytorch.likelihoods.GaussianLikelihood().to(dev)
    model = ProductStructureGPModel(train_x, train_y, likelihood).to(dev)
    model.covar_module.base_kernel.base_kernel.lengthscale = 0.7
    op = model.covar_module(train_x)
    print("covariance operator:", type(op).__name__, "of family", getattr(getattr(op, "spec", None), "kind", "(dense)"))

    model.train()
    likelihood.train()
    optimizer = torch.optim.Adam(model.parameters(), lr=0.1)
    mll = gpytorch.mlls.ExactMarginalLogLikelihood(likelihood, model)
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for i in range(args.iters):
        optimizer.zero_grad()
        loss = -mll(model(train_x), train_y)
        loss.backward()
        print("Iter %d/%d - Loss: %.3f" % (i + 1, args.iters, loss.item()))
        optimizer.step()
    torch.cuda.synchronize()
    print(f"training: {time.perf_counter() - t0:.2f} s, peak device memory {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB")
    print("lengthscales:", [round(v, 3) for v in model.covar_module.base_kernel.base_kernel.lengthscale.detach().reshape(-1).tolist()])

    model.eval()
    likelihood.eval()
    with torch.no_grad(), gpytorch.settings.fast_pred_var():
        pred = likelihood(model(test_x))
        lower, upper = pred.confidence_region()
    rmse = float((pred.mean - test_y).pow(2).mean().sqrt())
    inside = float(((test_y >= lower) & (test_y <= upper)).float().mean())
    print(f"test RMSE {rmse:.4f} (noise 0.05), {100 * inside:.1f} % of the noise-free targets inside the 95 % region")


if __name__ == "__main__":
    main()
