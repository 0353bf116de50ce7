#!/usr/bin/env python3
"""GP regression on UNCERTAIN inputs on one MI355X through the gpytorch-shaped API: every input is a Gaussian, x = [mu | log sigma^2], and the covariance
is ``GaussianSymmetrizedKLKernel``, k = exp(-SKL(x, x') / l) with the symmetrized Kullback-Leibler divergence of the two Gaussians (the reference's
example notebook for this kernel has the same set-up).  The reference broadcasts about eight n x n x d tensors per evaluation; here the kernel is one
matrix-free operator whose prepared rows carry every point's variance, and the derivative pass hands the gradient with respect to every point's mean
and variance to autograd.

Run 1 fits and predicts with the input variances as given.  Run 2 does not know them: it starts every training point at one common log sigma^2 and
LEARNS the per-point tensor with the hyper-parameters -- the gradient of the marginal log likelihood with respect to those n values comes from the fused
path.  The kernel is not positive definite in general; the likelihood's noise keeps the solves well posed.

    python examples/distributional_gp_regression.py                      # n = 4000
    python examples/distributional_gp_regression.py --n 20000 --iters 50
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpytorch_amd as gpytorch  # noqa: E402


class DistributionalGP(gpytorch.models.ExactGP):
    """``learn_logvar``: the training points' log sigma^2 is a parameter that replaces the variance column of the inputs while training."""

    def __init__(self, train_x, train_y, likelihood, learn_logvar=False):
        super().__init__(train_x, train_y, likelihood)
        self.mean_module = gpytorch.means.ConstantMean()
        self.covar_module = gpytorch.kernels.ScaleKernel(gpytorch.kernels.GaussianSymmetrizedKLKernel())
        d = train_x.shape[-1] // 2
        self.d = d
        self.logvar = torch.nn.Parameter(train_x[:, d:].clone()) if learn_logvar else None

    def forward(self, x):
        if self.logvar is not None and self.training:
            x = torch.cat([x[:, : self.d], self.logvar], -1)
        return gpytorch.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))


def run(name, train_x, train_y, test_x, test_y, iters, lr, learn_logvar):
    dev = train_x.device
    likelihood = gpytorch.likelihoods.GaussianLikelihood().to(dev)
    model = DistributionalGP(train_x, train_y, likelihood, learn_logvar).to(dev)
    likelihood.noise = 0.5
    model.train()
    likelihood.train()
    op = model.covar_module(train_x)
    print(f"[{name}] covariance operator:", type(op).__name__, "of family", op.spec.kind)
    optimizer = torch.optim.Adam(model.parameters(), lr=lr)
    mll = gpytorch.mlls.ExactMarginalLogLikelihood(likelihood, model)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        optimizer.zero_grad()
        loss = -mll(model(train_x), train_y)
        loss.backward()
        if i % 10 == 0 or i == iters - 1:
            print(f"[{name}] Iter {i + 1}/{iters} - Loss: {loss.item():.3f}")
        optimizer.step()
    torch.cuda.synchronize()
    print(f"[{name}] training: {time.perf_counter() - t0:.2f} s")
    if learn_logvar:   # predict with what was learned
        model.set_train_data(torch.cat([train_x[:, : model.d], model.logvar.detach()], -1), train_y, strict=False)
    model.eval()
    likelihood.eval()
    with torch.no_grad(), gpytorch.settings.fast_pred_var():
        pred = likelihood(model(test_x))
    rmse = float((pred.mean - test_y).pow(2).mean().sqrt())
    print(f"[{name}] test RMSE {rmse:.4f}; lengthscale {model.covar_module.base_kernel.lengthscale.item():.3f}, noise {likelihood.noise.item():.3f}")
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this example runs the fused HIP path: it needs a ROCm device"
    dev = torch.device("cuda:0")
    torch.manual_seed(args.seed)

    def data(n):
        # true positions on [0, 1]; what is observed is a noisy position mu with a KNOWN, point-dependent standard deviation
        pos = torch.rand(n)
        sd = 0.01 + 0.05 * torch.rand(n)
        mu = pos + sd * torch.randn(n)
        y = torch.sin(2 * math.pi * pos) + 0.1 * torch.randn(n)
        return torch.stack([mu, (sd * sd).log()], -1).to(dev), y.to(dev), sd

    train_x, train_y, sd = data(args.n)
    test_x, test_y, _ = data(500)
    run("given variances", train_x, train_y, test_x, test_y, args.iters, args.lr, learn_logvar=False)
    blind = train_x.clone()
    blind[:, 1] = math.log(0.03 ** 2)   # the variances are NOT known: one common start, then learned per point
    model = run("learned variances", blind, train_y, test_x, test_y, args.iters, args.lr, learn_logvar=True)
    learned_sd = (0.5 * model.logvar.detach()[:, 0]).exp().cpu()
    moved = float((learned_sd - 0.03).abs().mean())
    print(f"learned per-point standard deviations: mean |sd - start| = {moved:.4f}, range [{float(learned_sd.min()):.3f}, {float(learned_sd.max()):.3f}]"
          f" (the data were generated with sd in [0.01, 0.06])")


if __name__ == "__main__":
    main()
