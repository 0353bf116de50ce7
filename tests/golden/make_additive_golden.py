#!/usr/bin/env python3
"""Golden fixture of the additive-structure kernel, made by EXECUTING the reference's own code in the build container
(``python tests/golden/make_additive_golden.py``; see make_golden.py for the approach and for what may be committed: outputs only).

What is executed from the reference (nothing is copied into the repo):
  * ``gpytorch/kernels/additive_structure_kernel.py`` -> the method ``AdditiveStructureKernel.forward``, extracted with ``ast`` because the
    package cannot be imported (``linear_operator`` is not installed), bound to a stub that carries ``base_kernel``;
  * the stand-in base kernel evaluates the reference's own RBF / Matern arithmetic under ``last_dim_is_batch=True``: the methods
    ``RBFKernel.forward`` and ``MaternKernel.forward`` and the function ``postprocess_rbf`` (``rbf_kernel.py``, ``matern_kernel.py``) through the
    reference's ``Kernel.covar_dist`` / ``sq_dist`` / ``dist`` (``kernel.py``), all extracted with ``ast``.  Its ``__call__`` hands
    ``last_dim_is_batch`` on to ``forward`` as ``Kernel.__call__`` does; the lazy wrapper the reference puts around the result is not needed
    to sum it.  ``ScaleKernel`` is restated as the multiplication it is (``scale_kernel.py:110-121``: under ``last_dim_is_batch`` the
    outputscale gains a trailing dimension).

``additive_values.npz`` holds numeric arrays only: per case x1, x2, ls (shaped [1, 1] or [1, d]), the outputscale, and per base family
K = forward(x1, x2) and the diagonals forward(x1, x1, diag=True), forward(x1[:k], x2[:k], diag=True).
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
    ("f", 21, 27, 4, True, False, torch.float32),
    ("g", 24, 24, 8, False, True, torch.float32),
]
BASES = [("rbf", None), ("matern12", 0.5), ("matern32", 1.5), ("matern52", 2.5)]


class _Off:
    @staticmethod
    def on():
        return False


def main():
    if not os.path.isdir(REF):
        sys.exit("reference not mounted; fixtures are generated in the build container only")
    sq_dist, dist = _extract_functions(f"{REF}/kernels/kernel.py", ["sq_dist", "dist"])
    (postprocess_rbf,) = _extract_functions(f"{REF}/kernels/rbf_kernel.py", ["postprocess_rbf"])
    ns = {"torch": torch, "math": math, "sq_dist": sq_dist, "dist": dist, "postprocess_rbf": postprocess_rbf, "trace_mode": _Off}
    covar_dist = _extract_method(f"{REF}/kernels/kernel.py", "Kernel", "covar_dist", dict(ns))
    rbf_fwd = _extract_method(f"{REF}/kernels/rbf_kernel.py", "RBFKernel", "forward", dict(ns))
    mat_fwd = _extract_method(f"{REF}/kernels/matern_kernel.py", "MaternKernel", "forward", dict(ns))
    add_fwd = _extract_method(f"{REF}/kernels/additive_structure_kernel.py", "AdditiveStructureKernel", "forward", dict(ns))

    def call(self, x1, x2, diag=False, last_dim_is_batch=False, **params):
        return self.forward(x1, x2, diag=diag, last_dim_is_batch=last_dim_is_batch, **params)

    RefRBF = type("RefRBF", (), {"covar_dist": covar_dist, "forward": rbf_fwd, "__call__": call})
    RefMatern = type("RefMatern", (), {"covar_dist": covar_dist, "forward": mat_fwd, "__call__": call})
    RefAdd = type("RefAdditiveStructure", (), {"forward": add_fwd})
    out = {}
    for name, n, m, d, ard, same, dt in CASES:
        g = torch.Generator().manual_seed(3000 + ord(name))
        x1 = torch.rand(n, d, generator=g, dtype=dt)
        x2 = x1.clone() if same else torch.rand(m, d, generator=g, dtype=dt)
        ls = 0.2 + 0.4 * torch.rand(1, d if ard else 1, generator=g, dtype=dt)
        os_ = 0.5 + torch.rand((), generator=g, dtype=dt)
        k = min(n, x2.shape[0])
        out.update({f"{name}_x1": x1.numpy(), f"{name}_x2": x2.numpy(), f"{name}_ls": ls.numpy(), f"{name}_os": os_.numpy(),
                    f"{name}_same": np.array(same)})
        for kind, nu in BASES:
            base = RefRBF() if nu is None else RefMatern()
            base.lengthscale, base.ard_num_dims, base.nu = ls, (d if ard else None), nu
            add = RefAdd()
            add.base_kernel = base
            out[f"{name}_K_{kind}"] = add.forward(x1, x1 if same else x2).numpy()
            out[f"{name}_diag_same_{kind}"] = add.forward(x1, x1, diag=True).numpy()
            out[f"{name}_diag_pair_{kind}"] = add.forward(x1[:k], x2[:k], diag=True).numpy()
        print(name, "K shape", out[f"{name}_K_rbf"].shape, "mean", round(float(out[f"{name}_K_rbf"].mean()), 3))
    np.savez_compressed(os.path.join(OUT, "additive_values.npz"), **out)
    print("wrote additive_values.npz with", len(out), "arrays")


if __name__ == "__main__":
    main()
