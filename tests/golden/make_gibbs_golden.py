#!/usr/bin/env python3
"""Golden fixture of the Gibbs kernel, made by EXECUTING the reference's own code in the build container
(``python tests/golden/make_gibbs_golden.py``; see make_golden.py for the approach and for what may be committed: outputs only).

What is executed from the reference (nothing is copied into the repo):
  * ``gpytorch/kernels/gibbs_kernel.py`` -> the method ``GibbsKernel.forward``, extracted with ``ast`` because the package cannot be imported
    (``linear_operator`` is not installed), bound to a stub that carries ``lengthscale_fn`` and ``covar_dist``;
  * ``gpytorch/kernels/kernel.py`` -> ``Kernel.covar_dist`` and the functions ``sq_dist`` / ``dist`` it calls, extracted the same way.
The stub's ``lengthscale_fn`` is the closed-form positive field ``tests/gibbs_ref.field``, so a test can restate it without any stored parameters.

``gibbs_values.npz`` holds numeric arrays only: per case x1, x2, K = forward(x1, x2) and the diagonals forward(x1, x1, diag=True),
forward(x1[:k], x2[:k], diag=True).  Case names are ``d<d><e|t><64|32>``: dimensions, x1 = x2 (e) or two clouds (t), dtype.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import OUT, REF, _extract_functions, _extract_method  # noqa: E402
from gibbs_ref import field  # noqa: E402

DIMS = (1, 2, 3, 6)


def cases():
    """(name, n, m, d, same, dtype): every d, one and two clouds, both dtypes; n in 12..17."""
    out, i = [], 0
    for d in DIMS:
        for same in (True, False):
            for dt in (torch.float64, torch.float32):
                n = 12 + (i % 6)
                m = n if same else 11 + ((i * 5) % 7)
                out.append((f"d{d}{'e' if same else 't'}{'64' if dt == torch.float64 else '32'}", n, m, d, same, dt))
                i += 1
    return out


def main():
    if not os.path.isdir(REF):
        sys.exit("reference not mounted; fixtures are generated in the build container only")
    sq_dist, dist = _extract_functions(f"{REF}/kernels/kernel.py", ["sq_dist", "dist"])
    ns = {"torch": torch, "sq_dist": sq_dist, "dist": dist}
    covar_dist = _extract_method(f"{REF}/kernels/kernel.py", "Kernel", "covar_dist", dict(ns))
    gibbs_fwd = _extract_method(f"{REF}/kernels/gibbs_kernel.py", "GibbsKernel", "forward", dict(ns))
    RefGibbs = type("RefGibbs", (), {"covar_dist": covar_dist, "forward": gibbs_fwd, "lengthscale_fn": staticmethod(field)})
    out = {}
    for idx, (name, n, m, d, same, dt) in enumerate(cases()):
        g = torch.Generator().manual_seed(5200 + idx)
        x1 = torch.rand(n, d, generator=g, dtype=dt)
        x2 = x1.clone() if same else torch.rand(m, d, generator=g, dtype=dt)
        k = min(n, x2.shape[0])
        ker = RefGibbs()
        out.update({f"{name}_x1": x1.numpy(), f"{name}_x2": x2.numpy()})
        out[f"{name}_K"] = ker.forward(x1, x2).numpy()
        out[f"{name}_diag_same"] = ker.forward(x1, x1, diag=True).numpy()
        out[f"{name}_diag_pair"] = ker.forward(x1[:k], x2[:k], diag=True).numpy()
        print(name, "K", out[f"{name}_K"].shape, out[f"{name}_K"].dtype, "mean", round(float(out[f"{name}_K"].mean()), 3))
    np.savez_compressed(os.path.join(OUT, "gibbs_values.npz"), **out)
    print("wrote gibbs_values.npz with", len(out), "arrays")


if __name__ == "__main__":
    main()
