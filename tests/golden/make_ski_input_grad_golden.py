#!/usr/bin/env python3
"""Golden fixture of the INPUT derivative of KISS-GP's cubic interpolation, made by EXECUTING the reference's own code in the build container
(``python tests/golden/make_ski_input_grad_golden.py``; see make_golden.py for the approach and for what may be committed: outputs only).

What is executed from the reference (nothing is copied into the repo): ``Interpolation.interpolate`` and ``_cubic_interpolation_kernel`` of
``gpytorch/utils/interpolation.py`` and ``create_grid`` of ``gpytorch/utils/grid.py``, through the loader of make_ski_golden.py, under
``torch.autograd.functional.jacobian``.  The reference detaches only the stencil base, so its ``interp_values`` carry d/dx through the cubic weights
and none through a one-hot boundary row.

``ski_input_grad_values.npz`` holds numeric arrays only: for every float64 case of make_ski_golden.py (the same grids, seeds and ``points()``) the
grid axes, x [n, d], ``interp_indices`` [n, 4^d], ``interp_values`` [n, 4^d] and the per-point Jacobian d values[p, :] / d x[p, :]  [n, 4^d, d].
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
from make_ski_golden import CASES, points  # noqa: E402


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
        if dt != torch.float64:
            continue
        g = torch.Generator().manual_seed(5000 + ord(name))
        grid = grid_mod.create_grid(list(sizes), bounds, dtype=dt)
        x = points(grid, g, dt)
        idx, val = Ref().interpolate(grid, x)
        full = torch.autograd.functional.jacobian(lambda z: Ref().interpolate(grid, z)[1], x)           # [n, 4^d, n, d]
        ar = torch.arange(x.shape[0])
        jac = full[ar, :, ar, :]                                                                       # [n, 4^d, d]: point p moves its own row only
        off = full.clone()
        off[ar, :, ar, :] = 0.0
        assert not off.any()
        for i, a in enumerate(grid):
            out[f"{name}_grid{i}"] = a.numpy()
        out.update({f"{name}_x": x.numpy(), f"{name}_idx": idx.numpy(), f"{name}_val": val.detach().numpy(), f"{name}_jac": jac.numpy()})
        print(name, sizes, tuple(jac.shape), float(jac.abs().max()))
    np.savez_compressed(os.path.join(OUT, "ski_input_grad_values.npz"), **out)
    print("wrote ski_input_grad_values.npz with", len(out), "arrays")


if __name__ == "__main__":
    main()
