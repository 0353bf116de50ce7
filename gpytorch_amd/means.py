"""Mean functions used by the ExactGP hot path (``gpytorch/means/constant_mean.py:111-113``,
``zero_mean.py``).  Pure PyTorch glue."""
from __future__ import annotations

import torch

from .module import Module


class Mean(Module):
    def __call__(self, x):
        if x.dim() == 1:
            x = x.unsqueeze(1)
        return self.forward(x)


class ZeroMean(Mean):
    def forward(self, x):
        return torch.zeros(x.shape[:-1], dtype=x.dtype, device=x.device)


class ConstantMean(Mean):
    def __init__(self, constant_prior=None, constant_constraint=None, batch_shape=torch.Size()):
        super().__init__()
        self.batch_shape = torch.Size(batch_shape)
        self.register_parameter("raw_constant", torch.nn.Parameter(torch.zeros(self.batch_shape)))
        if constant_constraint is not None:
            self.register_constraint("raw_constant", constant_constraint)
        if constant_prior is not None:
            self.register_prior("mean_prior", constant_prior, self._constant_param, self._constant_closure)

    @staticmethod
    def _constant_param(m):        # constant_mean.py:99-101
        return m.constant

    @staticmethod
    def _constant_closure(m, value):
        m._set_transformed("raw_constant", value)

    @property
    def constant(self):
        return self._get_transformed("raw_constant")

    @constant.setter
    def constant(self, value):
        self._set_transformed("raw_constant", value)

    def forward(self, x):
        c = self.constant.unsqueeze(-1)  # constant_mean.py:111-113
        return c.expand(*torch.broadcast_shapes(c.shape[:-1], x.shape[:-2]), x.shape[-2])


class ConstantMeanGrad(Mean):
    """``gpytorch/means/constant_mean_grad.py:10-22``: the mean of a GP over values and gradients -- a learned constant for the value, zero for the
    d partial derivatives; [..., n, d + 1]."""

    derivatives_per_dim = 1

    def __init__(self, prior=None, batch_shape=torch.Size(), **kwargs):
        super().__init__()
        self.batch_shape = torch.Size(batch_shape)
        self.register_parameter("constant", torch.nn.Parameter(torch.zeros(*self.batch_shape, 1)))
        if prior is not None:
            self.register_prior("mean_prior", prior, "constant")

    def forward(self, x):
        batch = torch.broadcast_shapes(self.batch_shape, x.shape[:-2])
        n, d = x.shape[-2:]
        c = self.constant.unsqueeze(-1).expand(*batch, n, 1)
        return torch.cat([c, torch.zeros(*batch, n, self.derivatives_per_dim * d, dtype=c.dtype, device=c.device)], -1)


class ConstantMeanGradGrad(ConstantMeanGrad):
    """``gpytorch/means/constant_mean_gradgrad.py:10-22``: the mean of a GP over values, gradients and non-mixed second derivatives -- a learned
    constant for the value, zero for the 2 d derivative components; [..., n, 2 d + 1]."""

    derivatives_per_dim = 2
