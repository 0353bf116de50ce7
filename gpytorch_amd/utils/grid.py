"""Grid helpers of KISS-GP (``gpytorch/utils/grid.py``): ``choose_grid_size``, ``create_grid``, ``create_data_from_grid``, ``ScaleToBounds``."""
from __future__ import annotations

import math

import torch


class ScaleToBounds(torch.nn.Module):
    """Scale the inputs into 0.95 x [lower_bound, upper_bound] (``grid.py:11-54``): in training mode by the minimum and maximum of the batch at
    hand, which it remembers; in evaluation mode by the remembered ones, clamping what falls outside."""

    def __init__(self, lower_bound, upper_bound):
        super().__init__()
        self.lower_bound = float(lower_bound)
        self.upper_bound = float(upper_bound)
        self.register_buffer("min_val", torch.tensor(lower_bound))
        self.register_buffer("max_val", torch.tensor(upper_bound))

    def forward(self, x):
        if self.training:
            min_val, max_val = x.min(), x.max()
            self.min_val.data = min_val
            self.max_val.data = max_val
        else:
            min_val, max_val = self.min_val, self.max_val
            x = x.clamp(min_val, max_val)
        diff = max_val - min_val
        return (x - min_val) * (0.95 * (self.upper_bound - self.lower_bound) / diff) + 0.95 * self.lower_bound


def choose_grid_size(train_inputs, ratio=1.0, kronecker_structure=True):
    """A grid size for KISS-GP from the training inputs [..., n, d] (``grid.py:80-100``): ``ratio`` grid points per data point in total -- with the
    Kronecker structure int(ratio n^(1/d)) per dimension."""
    num_data = train_inputs.numel() if train_inputs.dim() == 1 else train_inputs.size(-2)
    num_dim = 1 if train_inputs.dim() == 1 else train_inputs.size(-1)
    if kronecker_structure:
        return int(ratio * math.pow(num_data, 1.0 / num_dim))
    return ratio * num_data


def convert_legacy_grid(grid: torch.Tensor):
    return [grid[:, i] for i in range(grid.size(-1))]


def create_data_from_grid(grid) -> torch.Tensor:
    """All points of the grid, [prod m_i, d], the FIRST dimension running fastest (``grid.py:107-127``: the reference's legacy order)."""
    if torch.is_tensor(grid):
        grid = convert_legacy_grid(grid)
    ndims = len(grid)
    assert all(axis.dim() == 1 for axis in grid)
    mesh = torch.stack(torch.meshgrid(*grid, indexing="ij"), dim=-1)
    return mesh.permute(*reversed(range(ndims + 1))).reshape(ndims, -1).transpose(0, 1)


def create_grid(grid_sizes, grid_bounds, extend=True, device="cpu", dtype=torch.float):
    """One 1-D tensor of ``grid_sizes[i]`` equally spaced points per dimension (``grid.py:130-175``).  With ``extend`` the spacing is
    (hi - lo) / (m - 2) and the grid reaches one spacing past each bound, which cubic interpolation needs near the boundary."""
    grid = []
    for i in range(len(grid_bounds)):
        lo, hi = grid_bounds[i]
        diff = float(hi - lo) / (grid_sizes[i] - 2)
        if extend:
            grid.append(torch.linspace(lo - diff, hi + diff, grid_sizes[i], device=device, dtype=dtype))
        else:
            grid.append(torch.linspace(lo, hi, grid_sizes[i], device=device, dtype=dtype))
    return grid
