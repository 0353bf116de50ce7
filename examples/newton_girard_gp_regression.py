#!/usr/bin/env python3
"""Additive GP regression WITH interactions on one MI355X through the gpytorch-shaped API: Duvenaud's additive GP,
k = sum_{n<=R} sigma_n e_n(z_1 .. z_d), with ``NewtonGirardAdditiveKernel`` over an ARD Matern-5/2 base in d = 6 dimensions, interactions up to order
R = 3.  The target is a sum of one-dimensional effects plus ONE pairwise interaction; the learned sigma_n say how much of the function each
interaction order carries.  The reference forms a d x n x n tensor, R power sums of it and R + 1 polynomials; here the kernel is one matrix-free
operator (d one-dimensional covariances per pair of points, the polynomials by a one-pass recursion in registers, one contraction), so a few
thousand points train through mBCG + SLQ and predict with LOVE variances like any other exact GP.

    python examples/newton_girard_gp_regression.py                      # n = 4000, d = 6, R = 3
    python examples/newton_girard_gp_regression.py --n 40000 --iters 10 --max-degree 2
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


class InteractionGPModel(gpytorch.models.ExactGP):
    def __init__(self, train_x, train_y, likelihood, max_degree):
        super().__init__(train_x, train_y, likelihood)
        d = train_x.shape[-1]
        self.mean_module = gpytorch.means.ConstantMean()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)   # (the reference deprecates the class name, not the model)
            # no ScaleKernel: one outputscale per interaction order is the kernel's own parameter
            self.covar_module = gpytorch.kernels.NewtonGirardAdditiveKernel(gpytorch.kernels.MaternKernel(nu=2.5, ard_num_dims=d), num_dims=d,
                                                                            max_degree=max_degree)

    def forward(self, x):
        return gpytorch.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))


def target(x):
    """One-dimensional effects in four of the six dimensions and one pairwise interaction between dimensions 4 and 5."""
    return (torch.sin(2 * math.pi * x[:, 0]) + (x[:, 1] - 0.5).abs() * 2 + x[:, 2] ** 2 + 0.5 * torch.cos(3 * math.pi * x[:, 3])
            + 1.5 * torch.sin(2 * math.pi * x[:, 4]) * (x[:, 5] - 0.5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4000)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--max-degree", type=int, default=3)
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
    model = InteractionGPModel(train_x, train_y, likelihood, args.max_degree).to(dev)
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
    print("lengthscales:", [round(v, 3) for v in model.covar_module.base_kernel.lengthscale.detach().reshape(-1).tolist()])
    sigma = model.covar_module.outputscale.detach().reshape(-1).tolist()
    share = [s * math.comb(d, k + 1) for k, s in enumerate(sigma)]     # sigma_n C(d, n): the prior variance the n-th order carries
    print("sigma_n (one per interaction order):", [round(s, 4) for s in sigma])
    print("share of the prior variance per order:", [round(v / sum(share), 3) for v in share])

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
