#!/usr/bin/env python3
"""Golden fixture of the Newton-Girard additive kernel, made by EXECUTING the reference's own code in the build container
(``python tests/golden/make_newton_girard_golden.py``; see make_golden.py for the approach and for what may be committed: outputs only).

What is executed from the reference (nothing is copied into the repo):
  * ``gpytorch/kernels/newton_girard_additive_kernel.py`` -> the method ``NewtonGirardAdditiveKernel.forward``, extracted with ``ast`` because the
    package cannot be imported (``linear_operator`` is not installed), bound to a stub that carries ``base_kernel``, ``max_degree`` and
    ``outputscale``; ``to_dense`` is the identity (the stand-in base kernel returns tensors);
  * the stand-in base kernel evaluates the reference's own RBF / Matern arithmetic under ``last_dim_is_batch=True``, exactly as
    make_additive_golden.py sets it up: ``RBFKernel.forward``, ``MaternKernel.forward``, ``postprocess_rbf`` through ``Kernel.covar_dist`` /
    ``sq_dist`` / ``dist``, all extracted with ``ast``.

``newton_girard_values.npz`` holds numeric arrays only: per case x1, x2, ls (shaped [1, 1] or [1, d]), sigma [max_degree], and per base family
K = forward(x1, x2) and the diagonals forward(x1, x1, diag=True), forward(x1[:k], x2[:k], diag=True).  Case names are
``d<d>r<R><s|a><e|t><64|32>``: dimensions, max_degree, single / ARD lengthscale, x1 = x2 (e) or two clouds (t), dtype.

The reference allocates its polynomials with ``torch.empty`` and no dtype, so its float64 outputs carry float32 rounding; the fixture records what it
returns.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, _extract_functions, _extract_method  # noqa: E402

DIMS = (2, 3, 5, 8)
BASES = [("rbf", None), ("matern12", 0.5), ("matern32", 1.5), ("matern52", 2.5)]


def cases():
    """(name, n, m, d, R, ard, same, dtype): every d with every max_degree of {1, 2, 3, d} it admits, in both dtypes; lengthscale shape and
    one / two clouds alternate so that every (dtype, ard, same) combination occurs."""
    out, i = [], 0
    for d in DIMS:
        for r in sorted({1, 2, 3, d}):
            if r > d:
                continue
            for t, dt in enumerate((torch.float64, torch.float32)):
                j = i // 2 + 3 * t      # one step per (d, R) pair: both bits cycle within each dtype
                ard, same = bool(j & 1), bool((j >> 1) & 1)
                n = 12 + (i % 5)
                m = n if same else 11 + (i % 7)
                name = f"d{d}r{r}{'a' if ard else 's'}{'e' if same else 't'}{'64' if dt == torch.float64 else '32'}"
                out.append((name, n, m, d, r, ard, same, dt))
                i += 1
    return out


class _Off:
    @staticmethod
    def on():
        return False


def main():
    if not os.path.isdir(REF):
        sys.exit("reference not mounted; fixtures are generated in the build container only")
    import warnings

    sq_dist, dist = _extract_functions(f"{REF}/kernels/kernel.py", ["sq_dist", "dist"])
    (postprocess_rbf,) = _extract_functions(f"{REF}/kernels/rbf_kernel.py", ["postprocess_rbf"])
    ns = {"torch": torch, "math": math, "sq_dist": sq_dist, "dist": dist, "postprocess_rbf": postprocess_rbf, "trace_mode": _Off,
          "to_dense": lambda t: t, "warnings": warnings}
    covar_dist = _extract_method(f"{REF}/kernels/kernel.py", "Kernel", "covar_dist", dict(ns))
    rbf_fwd = _extract_method(f"{REF}/kernels/rbf_kernel.py", "RBFKernel", "forward", dict(ns))
    mat_fwd = _extract_method(f"{REF}/kernels/matern_kernel.py", "MaternKernel", "forward", dict(ns))
    ng_fwd = _extract_method(f"{REF}/kernels/newton_girard_additive_kernel.py", "NewtonGirardAdditiveKernel", "forward", dict(ns))

    def call(self, x1, x2, diag=False, last_dim_is_batch=False, **params):
        return self.forward(x1, x2, diag=diag, last_dim_is_batch=last_dim_is_batch, **params)

    RefRBF = type("RefRBF", (), {"covar_dist": covar_dist, "forward": rbf_fwd, "__call__": call})
    RefMatern = type("RefMatern", (), {"covar_dist": covar_dist, "forward": mat_fwd, "__call__": call})
    RefNG = type("RefNewtonGirard", (), {"forward": ng_fwd})
    out = {}
    for idx, (name, n, m, d, r, ard, same, dt) in enumerate(cases()):
        g = torch.Generator().manual_seed(4100 + idx)
        x1 = torch.rand(n, d, generator=g, dtype=dt)
        x2 = x1.clone() if same else torch.rand(m, d, generator=g, dtype=dt)
        ls = 0.2 + 0.4 * torch.rand(1, d if ard else 1, generator=g, dtype=dt)
        sigma = 0.2 + torch.rand(r, generator=g, dtype=dt)
        k = min(n, x2.shape[0])
        out.update({f"{name}_x1": x1.numpy(), f"{name}_x2": x2.numpy(), f"{name}_ls": ls.numpy(), f"{name}_sigma": sigma.numpy()})
        for kind, nu in BASES:
            base = RefRBF() if nu is None else RefMatern()
            base.lengthscale, base.ard_num_dims, base.nu = ls, (d if ard else None), nu
            ng = RefNG()
            ng.base_kernel, ng.max_degree, ng.outputscale = base, r, sigma
            out[f"{name}_K_{kind}"] = ng.forward(x1, x1 if same else x2).numpy()
            out[f"{name}_diag_same_{kind}"] = ng.forward(x1, x1, diag=True).numpy()
            out[f"{name}_diag_pair_{kind}"] = ng.forward(x1[:k], x2[:k], diag=True).numpy()
        print(name, "K", out[f"{name}_K_rbf"].shape, out[f"{name}_K_rbf"].dtype, "mean", round(float(out[f"{name}_K_rbf"].mean()), 3))
    np.savez_compressed(os.path.join(OUT, "newton_girard_values.npz"), **out)
    print("wrote newton_girard_values.npz with", len(out), "arrays")


if __name__ == "__main__":
    main()
