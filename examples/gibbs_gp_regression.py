#!/usr/bin/env python3
"""Non-stationary GP regression on one MI355X through the gpytorch-shaped API: a one-dimensional CHIRP, whose wiggles get faster along the axis, with
``GibbsKernel`` -- the covariance with an input-dependent lengthscale l(x) -- and a small Softplus MLP as ``lengthscale_fn``.  A stationary kernel has
to pick one lengthscale for the whole record; here l(x) is learned and shrinks where the signal speeds up.  The reference forms about six n x n
tensors per evaluation (and their autograd copies); here the kernel is one matrix-free operator whose prepared rows carry the per-point lengthscale,
and the derivative pass hands the gradient with respect to every l(x_i) to autograd, which carries it into the MLP.

    python examples/gibbs_gp_regression.py                      # n = 20 000
    python examples/gibbs_gp_regression.py --n 4000 --iters 200 --lr 0.02
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpytorch_amd as gpytorch  # noqa: E402


class LengthscaleMLP(torch.nn.Module):
    """x -> l(x) > 0: 1 -> 16 -> 1 with Softplus, plus a floor that keeps l away from zero."""

    def __init__(self, hidden=16, floor=0.005, init=0.05):
        super().__init__()
        self.net = torch.nn.Sequential(torch.nn.Linear(1, hidden), torch.nn.Softplus(), torch.nn.Linear(hidden, 1), torch.nn.Softplus())
        self.floor = floor
        with torch.no_grad():   # start near l(x) = floor + init, with hidden units that switch on at different places of [0, 1]
            self.net[0].weight.fill_(8.0)
            self.net[0].bias.copy_(-8.0 * torch.linspace(0.0, 1.0, hidden))
            self.net[2].weight.mul_(0.1)
            self.net[2].bias.fill_(math.log(math.expm1(init)))

    def forward(self, x):
        return self.net(x) + self.floor


class GibbsGPModel(gpytorch.models.ExactGP):
    def __init__(self, train_x, train_y, likelihood):
        super().__init__(train_x, train_y, likelihood)
        self.mean_module = gpytorch.means.ConstantMean()
        self.covar_module = gpytorch.kernels.ScaleKernel(gpytorch.kernels.GibbsKernel(LengthscaleMLP()))

    def forward(self, x):
        return gpytorch.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))


def chirp(x):
    """sin(2 pi (2 x + 10 x^3)): the local frequency grows from 2 to 32 across [0, 1]."""
    return torch.sin(2 * math.pi * (2 * x + 10 * x ** 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20_000)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this example runs the fused HIP path: it needs a ROCm device"
    dev = torch.device("cuda:0")
    torch.manual_seed(args.seed)
    n = args.n
    train_x = torch.rand(n, 1)
    train_y = chirp(train_x[:, 0]) + 0.2 * torch.randn(n)
    test_x = torch.linspace(0.01, 0.99, 500).unsqueeze(-1)
    test_y = chirp(test_x[:, 0])
    train_x, train_y, test_x, test_y = train_x.to(dev), train_y.to(dev), test_x.to(dev), test_y.to(dev)

    likelihood = gpytorch.likelihoods.GaussianLikelihood().to(dev)
    model = GibbsGPModel(train_x, train_y, likelihood).to(dev)
    likelihood.noise = 0.1
    op = model.covar_module(train_x)
    print("covariance operator:", type(op).__name__, "of family", op.spec.kind)

    model.train()
    likelihood.train()
    optimizer = torch.optim.Adam(model.parameters(), lr=args.lr)
    mll = gpytorch.mlls.ExactMarginalLogLikelihood(likelihood, model)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for i in range(args.iters):
        optimizer.zero_grad()
        loss = -mll(model(train_x), train_y)
        loss.backward()
        print("Iter %d/%d - Loss: %.3f" % (i + 1, args.iters, loss.item()))
        optimizer.step()
    torch.cuda.synchronize()
    print(f"training: {time.perf_counter() - t0:.2f} s")

    model.eval()
    likelihood.eval()
    with torch.no_grad(), gpytorch.settings.fast_pred_var():
        pred = likelihood(model(test_x))
        lower, upper = pred.confidence_region()
        l_test = model.covar_module.base_kernel.lengthscale_fn(test_x).reshape(-1)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    rmse = float((pred.mean - test_y).pow(2).mean().sqrt())
    inside = float(((test_y >= lower) & (test_y <= upper)).float().mean())
    print("learned l(x) at x = 0.05, 0.5, 0.95:", [round(float(l_test[i]), 4) for i in (20, 250, 479)])
    print(f"test RMSE {rmse:.4f} (noise 0.2), {100 * inside:.1f} % of the noise-free targets inside the 95 % region")
    print(f"peak device memory {peak / 2 ** 20:.0f} MiB; the dense form's six n x n float32 tensors would need {6 * n * n * 4 / 2 ** 30:.1f} GiB")


if __name__ == "__main__":
    main()
