#!/usr/bin/env python3
"""Spectral-mixture GP regression on one MI355X through the gpytorch-shaped API: the cells of the reference's
examples/01_Exact_GPs/Spectral_Mixture_GP_Regression.ipynb (fifteen points of one sine period, four mixtures, ``initialize_from_data``, Adam on the
marginal log likelihood, extrapolation to five periods with LOVE variances), and with ``--n`` the same model on a long quasi-periodic series, where the
kernel runs matrix-free (the reference forms a Q x n x n x d tensor).

    python examples/spectral_mixture_regression.py                 # the notebook
    python examples/spectral_mixture_regression.py --n 100000 --iters 10
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpytorch_amd as gpytorch  # noqa: E402


class SpectralMixtureGPModel(gpytorch.models.ExactGP):
    def __init__(self, train_x, train_y, likelihood):
        super().__init__(train_x, train_y, likelihood)
        self.mean_module = gpytorch.means.ConstantMean()
        self.covar_module = gpytorch.kernels.SpectralMixtureKernel(num_mixtures=4)
        self.covar_module.initialize_from_data(train_x, train_y)

    def forward(self, x):
        return gpytorch.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=15, help="training points (15: the notebook's data)")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this example runs the fused HIP path: it needs a ROCm device"
    dev = torch.device("cuda:0")
    torch.manual_seed(args.seed)
    if args.n == 15:
        train_x = torch.linspace(0, 1, 15)
        train_y = torch.sin(train_x * (2 * math.pi))
        test_x = torch.linspace(0, 5, 51)
    else:   # a long quasi-periodic series: two tones and noise on [0, 1]
        train_x = torch.rand(args.n).sort().values
        train_y = torch.sin(2 * math.pi * 1.9 * train_x) + 0.5 * torch.cos(2 * math.pi * 5.2 * train_x) + 0.1 * torch.randn(args.n)
        test_x = torch.linspace(0, 1.5, 151)
    train_x, train_y, test_x = train_x.to(dev), train_y.to(dev), test_x.to(dev)

    likelihood = gpytorch.likelihoods.GaussianLikelihood().to(dev)
    model = SpectralMixtureGPModel(train_x, train_y, likelihood).to(dev)
    print("covariance operator:", type(model.covar_module(train_x.unsqueeze(-1))).__name__)

    model.train()
    likelihood.train()
    optimizer = torch.optim.Adam(model.parameters(), lr=0.1)
    mll = gpytorch.mlls.ExactMarginalLogLikelihood(likelihood, model)
    t0 = time.perf_counter()
    for i in range(args.iters):
        optimizer.zero_grad()
        output = model(train_x)
        loss = -mll(output, train_y)
        loss.backward()
        print("Iter %d/%d - Loss: %.3f" % (i + 1, args.iters, loss.item()))
        optimizer.step()
    torch.cuda.synchronize()
    print(f"training: {time.perf_counter() - t0:.2f} s")

    model.eval()
    likelihood.eval()
    with torch.no_grad(), gpytorch.settings.fast_pred_var():
        observed_pred = likelihood(model(test_x))
        lower, upper = observed_pred.confidence_region()
    for x, mu, lo, hi in list(zip(test_x.tolist(), observed_pred.mean.tolist(), lower.tolist(), upper.tolist()))[::10]:
        print(f"x = {x:5.2f}   mean {mu:+.3f}   95 % [{lo:+.3f}, {hi:+.3f}]")


if __name__ == "__main__":
    main()
