#!/usr/bin/env python3
"""Sequence fitness regression on one MI355X through the gpytorch-shaped API: synthetic protein-like sequences (T positions over V letters, one-hot
encoded and flattened to T V columns) whose fitness depends on a few positions, with ``HammingIMQKernel`` -- the inverse-multiquadric Hamming kernel
k = ((1 + alpha) / (alpha + d_Hamming))^beta.  The reference's distance broadcasts an n x n x T x V tensor (n = 2000, T = 100, V = 20: 32 GB); here
the kernel is one matrix-free operator on sequences stored as one byte per position, and alpha, beta, the outputscale and the noise are trained by
the marginal log likelihood.

    python examples/hamming_sequence_gp_regression.py                      # n = 20 000, T = 100, V = 20
    python examples/hamming_sequence_gp_regression.py --n 4000 --iters 50
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpytorch_amd as gpytorch  # noqa: E402


class SequenceGPModel(gpytorch.models.ExactGP):
    def __init__(self, train_x, train_y, likelihood, vocab_size):
        super().__init__(train_x, train_y, likelihood)
        self.mean_module = gpytorch.means.ConstantMean()
        self.covar_module = gpytorch.kernels.ScaleKernel(gpytorch.kernels.HammingIMQKernel(vocab_size=vocab_size))

    def forward(self, x):
        return gpytorch.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))


def sequences(n, t, v, gen, parents):
    """Mutants of a few wild types: every sequence copies one parent and redraws each position with its own probability in 0..0.3."""
    par = parents[torch.randint(0, parents.shape[0], (n,), generator=gen)]
    redraw = torch.rand(n, t, generator=gen) < 0.3 * torch.rand(n, 1, generator=gen)
    return torch.where(redraw, torch.randint(0, v, (n, t), generator=gen), par)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20_000)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--vocab", type=int, default=20)
    ap.add_argument("--sites", type=int, default=6, help="positions the fitness depends on")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this example runs the fused HIP path: it needs a ROCm device"
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(args.seed)
    n, t, v = args.n, args.length, args.vocab
    parents = torch.randint(0, v, (4, t), generator=gen)
    tok = sequences(n + 500, t, v, gen, parents)
    sites = torch.randperm(t, generator=gen)[: args.sites]
    effect = torch.randn(args.sites, v, generator=gen)
    fitness = sum(effect[i][tok[:, s]] for i, s in enumerate(sites)) / args.sites ** 0.5
    y = fitness + 0.1 * torch.randn(n + 500, generator=gen)
    x = torch.nn.functional.one_hot(tok, v).reshape(n + 500, t * v).float()
    train_x, train_y, test_x, test_y = x[:n].to(dev), y[:n].to(dev), x[n:].to(dev), fitness[n:].to(dev)

    likelihood = gpytorch.likelihoods.GaussianLikelihood().to(dev)
    model = SequenceGPModel(train_x, train_y, likelihood, v).to(dev)
    likelihood.noise = 0.1
    op = model.covar_module(train_x)
    print("covariance operator:", type(op).__name__, "of family", op.spec.kind, "-- prepared cloud:", op.prepared()[0].xp.numel() * 4, "bytes")

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
        hk = model.covar_module.base_kernel
        print("Iter %d/%d - Loss: %.3f   alpha: %.3f   beta: %.3f   noise: %.4f" % (i + 1, args.iters, loss.item(), hk.alpha.item(), hk.beta.item(),
                                                                                  likelihood.noise.item()))
        optimizer.step()
    torch.cuda.synchronize()
    print(f"training: {time.perf_counter() - t0:.2f} s")

    model.eval()
    likelihood.eval()
    with torch.no_grad(), gpytorch.settings.fast_pred_var():
        pred = likelihood(model(test_x))
        lower, upper = pred.confidence_region()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    rmse = float((pred.mean - test_y).pow(2).mean().sqrt())
    inside = float(((test_y >= lower) & (test_y <= upper)).float().mean())
    print(f"test RMSE {rmse:.4f} (fitness std {float(test_y.std()):.3f}, noise 0.1), {100 * inside:.1f} % of the noise-free targets inside the 95 % region")
    print(f"peak device memory {peak / 2 ** 20:.0f} MiB; the reference's n x n x T x V float32 tensor would need {n * n * t * v * 4 / 2 ** 30:.0f} GiB")


if __name__ == "__main__":
    main()
