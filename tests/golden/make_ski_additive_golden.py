#!/usr/bin/env python3
"""Golden fixture of ADDITIVE KISS-GP (AdditiveStructureKernel over GridInterpolationKernel(num_dims=1)), made by EXECUTING the reference's own code
in the build container (``python tests/golden/make_ski_additive_golden.py``; see make_golden.py for the approach and for what may be committed:
outputs only).

What is executed from the reference (nothing is copied into the repo):

  * ``gpytorch/utils/interpolation.py`` -> ``Interpolation.interpolate`` (extracted with ``ast``, as make_ski_golden.py does) on
    ``x.transpose(-1, -2).unsqueeze(-1).reshape(-1, 1)`` against ONE shared grid axis: exactly what
    ``GridInterpolationKernel._compute_grid(last_dim_is_batch=True)`` does (``grid_interpolation_kernel.py:132-143``); the indices and values are
    stored in its [d, n, 4] layout;
  * ``gpytorch/kernels/rbf_kernel.py`` / ``matern_kernel.py`` / ``rq_kernel.py`` -> the ``forward`` METHODS, through the reference's own
    ``Kernel.covar_dist``, called as ``grid_kernel.py:142-146`` calls the base kernel: first grid point against the one-column grid under
    ``last_dim_is_batch=True``, with a lengthscale [1, k].  The outputs [k, m] are the first Toeplitz columns of the k batch members.

``ski_additive_values.npz`` holds numeric arrays only.
"""
from __future__ import annotations

import math
import os
import sys
from functools import reduce
from operator import mul

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, _extract_functions, _extract_method, _load  # noqa: E402

# name, d, grid size, bounds of the one axis, dtype
CASES = [
    ("a", 2, 9, (0.0, 1.0), torch.float64),
    ("b", 2, 9, (-2.0, 3.0), torch.float32),
    ("c", 5, 12, (0.0, 1.0), torch.float64),
    ("d", 5, 12, (-1.0, 0.5), torch.float32),
]


def points(axis, d, g, dt):
    """<= 40 points of d columns, all on the ONE axis: interior draws, coordinates exactly on nodes, in the first and in the last cell, mixed rows,
    grid.min and grid.max."""
    lo, hi, h = axis.min(), axis.max(), axis[1] - axis[0]
    interior = lo + h + torch.rand(14, d, generator=g, dtype=dt) * (hi - lo - 2 * h)
    nodes = axis[torch.randint(0, axis.numel(), (8, d), generator=g)]
    first = lo + 0.98 * h * torch.rand(6, d, generator=g, dtype=dt) + 0.01 * h
    last = hi - 0.98 * h * torch.rand(6, d, generator=g, dtype=dt) - 0.01 * h
    mixed = torch.where(torch.rand(4, d, generator=g) < 0.5, first[:4], torch.where(torch.rand(4, d, generator=g) < 0.5, last[:4], interior[:4]))
    return torch.cat([interior, nodes, first, last, mixed, lo.expand(1, d), hi.expand(1, d)]).to(dt)


def main():
    if not os.path.isdir(REF):
        sys.exit("reference not mounted; fixtures are generated in the build container only")
    grid_mod = _load(f"{REF}/utils/grid.py", "ref_grid")
    ns = {"torch": torch, "convert_legacy_grid": grid_mod.convert_legacy_grid, "reduce": reduce, "mul": mul}
    path = f"{REF}/utils/interpolation.py"
    Ref = type("RefInterpolation", (), {"interpolate": _extract_method(path, "Interpolation", "interpolate", ns),
                                        "_cubic_interpolation_kernel": _extract_method(path, "Interpolation", "_cubic_interpolation_kernel", ns)})
    out = {}
    for name, d, size, bounds, dt in CASES:
        g = torch.Generator().manual_seed(7000 + ord(name))
        grid = grid_mod.create_grid([size], [bounds], dtype=dt)
        x = points(grid[0], d, g, dt)
        n = x.shape[0]
        assert n <= 40
        inputs = x.transpose(-1, -2).unsqueeze(-1)                        # grid_interpolation_kernel.py:134-142
        batch_shape = inputs.shape[:-2]
        idx, val = Ref().interpolate(grid, inputs.reshape(-1, 1))
        idx, val = idx.view(*batch_shape, n, -1), val.view(*batch_shape, n, -1)
        assert idx.shape == (d, n, 4)
        out.update({f"{name}_grid": grid[0].numpy(), f"{name}_x": x.numpy(), f"{name}_idx": idx.numpy(), f"{name}_val": val.numpy()})
        print(name, d, size, dt, tuple(val.shape))

    # the base kernel on the one-column grid under last_dim_is_batch, lengthscale [1, k]
    sq_dist, dist = _extract_functions(f"{REF}/kernels/kernel.py", ["sq_dist", "dist"])
    postprocess_rbf, = _extract_functions(f"{REF}/kernels/rbf_kernel.py", ["postprocess_rbf"])
    off = type("Off", (), {"on": staticmethod(lambda: False)})
    kns = {"torch": torch, "math": math, "sq_dist": sq_dist, "dist": dist, "postprocess_rbf": postprocess_rbf, "trace_mode": off}
    covar_dist = _extract_method(f"{REF}/kernels/kernel.py", "Kernel", "covar_dist", dict(kns))
    fwd = {kind: _extract_method(f"{REF}/kernels/{kind}_kernel.py", cls, "forward", dict(kns))
           for kind, cls in (("rbf", "RBFKernel"), ("matern", "MaternKernel"), ("rq", "RQKernel"))}
    axis = grid_mod.create_grid([16], [(-0.3, 1.4)], dtype=torch.float64)[0]
    first, full = axis[:1].unsqueeze(-1), axis.unsqueeze(-1)            # grid_kernel.py:142-143 for a one-axis grid
    out["col_axis"] = axis.numpy()
    for k, ls in ((1, [0.4]), (3, [0.25, 0.5, 0.9])):
        for kind in ("rbf", "matern", "rq"):
            stub = type("Ref" + kind, (), {"covar_dist": covar_dist, "forward": fwd[kind]})()
            stub.lengthscale = torch.tensor([ls], dtype=torch.float64)
            stub.ard_num_dims = k if k > 1 else None
            stub.nu, stub.alpha = 2.5, torch.tensor([1.6], dtype=torch.float64)
            cov = stub.forward(first, full, last_dim_is_batch=True)
            assert cov.shape == (k, 1, axis.numel()), cov.shape
            out[f"col_{kind}_k{k}"] = cov.squeeze(-2).numpy()
        out[f"col_ls_k{k}"] = np.array(ls)
    out["col_alpha"] = np.array(1.6)
    np.savez_compressed(os.path.join(OUT, "ski_additive_values.npz"), **out)
    print("wrote ski_additive_values.npz with", len(out), "arrays")


if __name__ == "__main__":
    main()
