"""Two outputs, two latent processes: the linear model of coregionalisation K = K_rbf (x) B_1 + K_matern32 (x) B_2 -- a smooth shared trend plus a
rougher component, each with its own lengthscale and its own 2 x 2 task covariance.  Training and prediction run on the fused multi-member product
(``kernels.LCMKernel`` -> ``lcm.LCMFusedLinearOperator``); ``max_cholesky_size(0)`` keeps even this small problem on the iterative path.
    python examples/lcm_multitask_regression.py"""
import math
import sys

import torch

sys.path.insert(0, ".")
import gpytorch_amd as gpytorch  # noqa: E402

dev = torch.device("cuda:0")
torch.manual_seed(0)
n, T = 2000, 2
x = torch.rand(n, 1)
smooth, rough = torch.sin(2 * math.pi * x[:, 0]), 0.3 * torch.sin(14 * math.pi * x[:, 0])
y = torch.stack([smooth + rough, 0.7 * smooth - rough], -1) + 0.05 * torch.randn(n, T)


class LCMGP(gpytorch.models.ExactGP):
    def __init__(self, x, y, lik):
        super().__init__(x, y, lik)
        self.mean_module = gpytorch.means.MultitaskMean(gpytorch.means.ConstantMean(), num_tasks=T)
        self.covar_module = gpytorch.kernels.LCMKernel([gpytorch.kernels.RBFKernel(), gpytorch.kernels.MaternKernel(nu=1.5)], num_tasks=T, rank=1)

    def forward(self, x):
        return gpytorch.distributions.MultitaskMultivariateNormal(self.mean_module(x), self.covar_module(x))


lik = gpytorch.likelihoods.MultitaskGaussianLikelihood(num_tasks=T).to(dev)
model = LCMGP(x.to(dev), y.to(dev), lik).to(dev)
model.covar_module.covar_module_list[0].data_covar_module.lengthscale = 0.3
model.covar_module.covar_module_list[1].data_covar_module.lengthscale = 0.05
mll = gpytorch.ExactMarginalLogLikelihood(lik, model)
opt = torch.optim.Adam(model.parameters(), lr=0.05)
model.train()
lik.train()
with gpytorch.settings.max_cholesky_size(0):
    for it in range(30):
        opt.zero_grad()
        loss = -mll(model(x.to(dev)), y.to(dev))
        loss.backward()
        opt.step()
        if it % 10 == 0 or it == 29:
            print(f"iter {it:2d}  -mll {loss.item():.4f}")
    model.eval()
    lik.eval()
    xs = torch.linspace(0, 1, 200).unsqueeze(-1)
    truth = torch.stack([torch.sin(2 * math.pi * xs[:, 0]) + 0.3 * torch.sin(14 * math.pi * xs[:, 0]),
                         0.7 * torch.sin(2 * math.pi * xs[:, 0]) - 0.3 * torch.sin(14 * math.pi * xs[:, 0])], -1)
    with torch.no_grad():
        pred = lik(model(xs.to(dev)))
    rmse = float((pred.mean.cpu() - truth).pow(2).mean().sqrt())
print(f"test rmse {rmse:.4f}  mean predictive sd {float(pred.variance.sqrt().mean()):.4f}")
assert rmse < 0.1
