#!/usr/bin/env python3
"""Golden fixture of KISS-GP's cubic interpolation, made by EXECUTING the reference's own code in the build container
(``python tests/golden/make_ski_golden.py``; see make_golden.py for the approach and for what may be committed: outputs only).

What is executed from the reference (nothing is copied into the repo):

  * ``gpytorch/utils/interpolation.py`` -> the methods ``Interpolation.interpolate`` and ``Interpolation._cubic_interpolation_kernel``, extracted
    with ``ast`` because the module cannot be imported (``linear_operator`` is not installed);
  * ``gpytorch/utils/grid.py`` -> ``create_grid``, ``create_data_from_grid`` and ``choose_grid_size``, loaded as a module (it imports torch only).

``ski_values.npz`` holds numeric arrays only: per case the grid axes, x, ``interp_indices`` and ``interp_values``; and per grid shape the output of
``create_data_from_grid``.
"""
from __future__ import annotations

import os
import sys
from functools import reduce
from operator import mul

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, _extract_method, _load  # noqa: E402

# name, grid sizes, bounds per axis, dtype
CASES = [
    ("a", (9,), [(0.0, 1.0)], torch.float64),
    ("b", (9,), [(-2.0, 3.0)], torch.float32),
    ("c", (9, 6), [(0.0, 1.0), (-1.0, 1.0)], torch.float64),
    ("d", (9, 6), [(0.0, 1.0), (-1.0, 1.0)], torch.float32),
    ("e", (7, 6, 5), [(0.0, 1.0), (0.0, 2.0), (-1.0, 0.5)], torch.float64),
    ("f", (7, 6, 5), [(0.0, 1.0), (0.0, 2.0), (-1.0, 0.5)], torch.float32),
    ("g", (4, 4, 4), [(0.0, 1.0)] * 3, torch.float64),
    ("h", (4, 4, 4), [(0.0, 1.0)] * 3, torch.float32),
    ("i", (12,), [(999.0, 1000.0)], torch.float64),
]


def points(grid, g, dt):
    """<= 40 points: interior draws, points exactly on nodes, points in the first and the last cell of each axis, grid.min and grid.max."""
    d = len(grid)
    lo = torch.stack([a.min() for a in grid])
    hi = torch.stack([a.max() for a in grid])
    h = torch.stack([a[1] - a[0] for a in grid])
    u = torch.rand(14, d, generator=g, dtype=dt)
    interior = lo + h + u * (hi - lo - 2 * h)
    nodes = torch.stack([torch.stack([a[int(torch.randint(0, a.numel(), (1,), generator=g))] for a in grid]) for _ in range(8)])
    first = lo + 0.98 * h * torch.rand(6, d, generator=g, dtype=dt) + 0.01 * h
    last = hi - 0.98 * h * torch.rand(6, d, generator=g, dtype=dt) - 0.01 * h
    mixed = torch.where(torch.rand(4, d, generator=g) < 0.5, first[:4], interior[:4])
    return torch.cat([interior, nodes, first, last, mixed, lo.unsqueeze(0), hi.unsqueeze(0)]).to(dt)


def main():
    if not os.path.isdir(REF):
        sys.exit("reference not mounted; fixtures are generated in the build container only")
    grid_mod = _load(f"{REF}/utils/grid.py", "ref_grid")
    ns = {"torch": torch, "convert_legacy_grid": grid_mod.convert_legacy_grid, "reduce": reduce, "mul": mul}
    path = f"{REF}/utils/interpolation.py"
    Ref = type("RefInterpolation", (), {"interpolate": _extract_method(path, "Interpolation", "interpolate", ns),
                                        "_cubic_interpolation_kernel": _extract_method(path, "Interpolation", "_cubic_interpolation_kernel", ns)})
    out = {}
    for name, sizes, bounds, dt in CASES:
        g = torch.Generator().manual_seed(5000 + ord(name))
        grid = grid_mod.create_grid(list(sizes), bounds, dtype=dt)
        x = points(grid, g, dt)
        assert x.shape[0] <= 40
        idx, val = Ref().interpolate(grid, x)
        for i, a in enumerate(grid):
            out[f"{name}_grid{i}"] = a.numpy()
        out.update({f"{name}_x": x.numpy(), f"{name}_bounds": np.array(bounds), f"{name}_idx": idx.numpy(), f"{name}_val": val.numpy()})
        out[f"{name}_data"] = grid_mod.create_data_from_grid(grid).numpy()
        print(name, sizes, dt, tuple(val.shape))
    sizes = [(n, d, ratio, int(grid_mod.choose_grid_size(torch.zeros(n, d), ratio))) for n, d, ratio in
             [(100, 1, 1.0), (1000, 2, 1.0), (500000, 3, 1.0), (4096, 3, 0.5), (77, 2, 2.0)]]
    out["choose_grid_size"] = np.array(sizes, dtype=np.float64)
    np.savez_compressed(os.path.join(OUT, "ski_values.npz"), **out)
    print("wrote ski_values.npz with", len(out), "arrays")


if __name__ == "__main__":
    main()
