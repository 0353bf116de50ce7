#!/usr/bin/env python3
"""Golden fixture of the piecewise-polynomial family, made by EXECUTING the reference's own code in the build container
(``python tests/golden/make_piecewise_golden.py``; see make_golden.py for the approach and for what may be committed: outputs only).

What is executed from the reference (nothing is copied into the repo):
  * ``gpytorch/kernels/piecewise_polynomial_kernel.py`` -> the module-level functions ``_fmax`` and ``_get_cov`` and the method
    ``PiecewisePolynomialKernel.forward`` (which computes j = floor(D / 2) + q + 1 itself), extracted with ``ast`` because the package cannot
    be imported (``linear_operator`` is not installed);
  * ``gpytorch/kernels/kernel.py`` -> ``sq_dist``, ``dist`` and the method ``Kernel.covar_dist`` the forward goes through.
The forward is bound to a stub that carries ``q`` and the lengthscale in the shape the real module holds it ([1, 1] or [1, d]).

``piecewise_values.npz`` holds numeric arrays only: per case x1, x2, ls, and K for q = 0..3.  The clouds are scaled so that a good share of the
pairs lies on each side of r = 1.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, _extract_functions, _extract_method  # noqa: E402

CASES = [  # name, n, m, d, ard, same, dtype
    ("a", 24, 24, 1, False, True, torch.float64),
    ("b", 18, 26, 2, False, False, torch.float64),
    ("c", 22, 22, 3, True, True, torch.float64),
    ("d", 17, 23, 5, True, False, torch.float64),
    ("e", 20, 20, 10, False, True, torch.float64),
    ("f", 21, 27, 3, False, False, torch.float32),
    ("g", 24, 24, 2, True, True, torch.float32),
    ("h", 19, 25, 10, True, False, torch.float32),
]


def main():
    if not os.path.isdir(REF):
        sys.exit("reference not mounted; fixtures are generated in the build container only")
    sq_dist, dist = _extract_functions(f"{REF}/kernels/kernel.py", ["sq_dist", "dist"])
    path = f"{REF}/kernels/piecewise_polynomial_kernel.py"
    fmax, get_cov = _extract_functions(path, ["_fmax", "_get_cov"])
    ns = {"torch": torch, "math": math, "sq_dist": sq_dist, "dist": dist, "_fmax": fmax, "_get_cov": get_cov}
    covar_dist = _extract_method(f"{REF}/kernels/kernel.py", "Kernel", "covar_dist", dict(ns))
    forward = _extract_method(path, "PiecewisePolynomialKernel", "forward", dict(ns))
    Ref = type("RefPiecewisePolynomial", (), {"covar_dist": covar_dist, "forward": forward})
    out = {}
    for name, n, m, d, ard, same, dt in CASES:
        g = torch.Generator().manual_seed(2000 + ord(name))
        x1 = torch.rand(n, d, generator=g, dtype=dt)
        x2 = x1.clone() if same else torch.rand(m, d, generator=g, dtype=dt)
        # typical distance of uniform points in the unit cube ~ sqrt(d / 6): lengthscales around it put pairs on both sides of r = 1
        ls = math.sqrt(d / 6.0) * (0.7 + 0.6 * torch.rand(1, d if ard else 1, generator=g, dtype=dt))
        out.update({f"{name}_x1": x1.numpy(), f"{name}_x2": x2.numpy(), f"{name}_ls": ls.numpy(), f"{name}_same": np.array(same)})
        for q in range(4):
            k = Ref()
            k.q, k.lengthscale = q, ls
            K = k.forward(x1, x1 if same else x2)
            out[f"{name}_K{q}"] = K.numpy()
        r = (x1.unsqueeze(1) / ls - x2.unsqueeze(0) / ls).norm(dim=-1)
        print(name, "share of pairs with r < 1:", round(float((r < 1).double().mean()), 3))
    np.savez_compressed(os.path.join(OUT, "piecewise_values.npz"), **out)
    print("wrote piecewise_values.npz with", len(out), "arrays")


if __name__ == "__main__":
    main()
