#!/usr/bin/env python3
"""Golden fixture of the product-structure kernel, made by EXECUTING the reference's own code in the build container
(``python tests/golden/make_product_structure_golden.py``; see make_golden.py for the approach and for what may be committed: outputs only).

What is executed from the reference (nothing is copied into the repo), exactly as make_additive_golden.py does it:
  * ``gpytorch/kernels/product_structure_kernel.py`` -> the method ``ProductStructureKernel.forward`` (lines 70-76: the base kernel under
    ``last_dim_is_batch=True``, then ``.prod(-3)`` / ``.prod(-2)``), extracted with ``ast`` because the package cannot be imported
    (``linear_operator`` is not installed), bound to a stub that carries ``base_kernel``;
  * the stand-in base kernel evaluates the reference's own RBF / Matern arithmetic under ``last_dim_is_batch=True``: the methods
    ``RBFKernel.forward`` and ``MaternKernel.forward`` and the function ``postprocess_rbf`` through the reference's ``Kernel.covar_dist`` /
    ``sq_dist`` / ``dist`` (``kernel.py``), all extracted with ``ast``.  ``ScaleKernel`` is restated as the multiplication it is
    (``scale_kernel.py:110-121``: under ``last_dim_is_batch`` the outputscale gains a trailing dimension, so it scales every one of the d members).

``product_structure_values.npz`` holds numeric arrays only: per case x1, x2, ls (shaped [1, 1] or [1, d]), the inner outputscale, and per base
family K = forward(x1, x2) without and with the inner ScaleKernel (``K_`` / ``Ks_``) and the diagonals forward(x1, x1, diag=True),
forward(x1[:k], x2[:k], diag=True) with it.
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
    ("a", 24, 24, 2, False, True, torch.float64),
    ("b", 18, 26, 3, True, False, torch.float64),
    ("c", 22, 22, 6, True, True, torch.float64),
    ("d", 17, 23, 8, False, False, torch.float64),
    ("e", 20, 31, 9, True, False, torch.float64),
    ("f", 21, 23, 3, True, False, torch.float32),
    ("g", 24, 24, 8, False, True, torch.float32),
]
BASES = [("rbf", None), ("matern12", 0.5), ("matern32", 1.5), ("matern52", 2.5)]


class _Off:
    @staticmethod
    def on():
        return False


class RefScale:
    """ScaleKernel.forward under ``last_dim_is_batch`` as the multiplication it is: the outputscale (no batch shape) gains a trailing dimension and
    multiplies the dimension batch [d, n, m] ([d, n] with ``diag``)."""

    def __init__(self, base, outputscale):
        self.base_kernel, self.outputscale = base, outputscale

    def __call__(self, x1, x2, diag=False, last_dim_is_batch=False, **params):
        orig = self.base_kernel(x1, x2, diag=diag, last_dim_is_batch=last_dim_is_batch, **params)
        os_ = self.outputscale.unsqueeze(-1) if last_dim_is_batch else self.outputscale
        return orig * (os_.unsqueeze(-1) if diag else os_.reshape(*os_.shape, 1, 1))


def main():
    if not os.path.isdir(REF):
        sys.exit("reference not mounted; fixtures are generated in the build container only")
    sq_dist, dist = _extract_functions(f"{REF}/kernels/kernel.py", ["sq_dist", "dist"])
    (postprocess_rbf,) = _extract_functions(f"{REF}/kernels/rbf_kernel.py", ["postprocess_rbf"])
    ns = {"torch": torch, "math": math, "sq_dist": sq_dist, "dist": dist, "postprocess_rbf": postprocess_rbf, "trace_mode": _Off}
    covar_dist = _extract_method(f"{REF}/kernels/kernel.py", "Kernel", "covar_dist", dict(ns))
    rbf_fwd = _extract_method(f"{REF}/kernels/rbf_kernel.py", "RBFKernel", "forward", dict(ns))
    mat_fwd = _extract_method(f"{REF}/kernels/matern_kernel.py", "MaternKernel", "forward", dict(ns))
    ps_fwd = _extract_method(f"{REF}/kernels/product_structure_kernel.py", "ProductStructureKernel", "forward", dict(ns))

    def call(self, x1, x2, diag=False, last_dim_is_batch=False, **params):
        return self.forward(x1, x2, diag=diag, last_dim_is_batch=last_dim_is_batch, **params)

    RefRBF = type("RefRBF", (), {"covar_dist": covar_dist, "forward": rbf_fwd, "__call__": call})
    RefMatern = type("RefMatern", (), {"covar_dist": covar_dist, "forward": mat_fwd, "__call__": call})
    RefPS = type("RefProductStructure", (), {"forward": ps_fwd})
    out = {}
    for name, n, m, d, ard, same, dt in CASES:
        g = torch.Generator().manual_seed(4100 + ord(name))
        x1 = torch.rand(n, d, generator=g, dtype=dt)
        x2 = x1.clone() if same else torch.rand(m, d, generator=g, dtype=dt)
        ls = 0.5 + 0.4 * torch.rand(1, d if ard else 1, generator=g, dtype=dt)
        os_ = 0.7 + 0.6 * torch.rand((), generator=g, dtype=dt)
        k = min(n, x2.shape[0])
        out.update({f"{name}_x1": x1.numpy(), f"{name}_x2": x2.numpy(), f"{name}_ls": ls.numpy(), f"{name}_os": os_.numpy(),
                    f"{name}_same": np.array(same)})
        for kind, nu in BASES:
            base = RefRBF() if nu is None else RefMatern()
            base.lengthscale, base.ard_num_dims, base.nu = ls, (d if ard else None), nu
            ps, pss = RefPS(), RefPS()
            ps.base_kernel, pss.base_kernel = base, RefScale(base, os_)
            out[f"{name}_K_{kind}"] = ps.forward(x1, x1 if same else x2).numpy()
            out[f"{name}_Ks_{kind}"] = pss.forward(x1, x1 if same else x2).numpy()
            out[f"{name}_diag_same_{kind}"] = pss.forward(x1, x1, diag=True).numpy()
            out[f"{name}_diag_pair_{kind}"] = pss.forward(x1[:k], x2[:k], diag=True).numpy()
        print(name, "K shape", out[f"{name}_K_rbf"].shape, "mean", round(float(out[f"{name}_K_matern52"].mean()), 4))
    np.savez_compressed(os.path.join(OUT, "product_structure_values.npz"), **out)
    print("wrote product_structure_values.npz with", len(out), "arrays")


if __name__ == "__main__":
    main()
