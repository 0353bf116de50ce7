#!/usr/bin/env python3
"""Golden fixture of the Matern-5/2 kernel with derivative observations, made by EXECUTING the reference's own code in the build container
(``python tests/golden/make_matern52grad_golden.py``; see make_golden.py for the approach and for what may be committed: outputs only).

What is executed from the reference (nothing is copied into the repo): ``gpytorch/kernels/matern52_kernel_grad.py`` -> the method
``Matern52KernelGrad.forward``, extracted with ``ast`` because the package cannot be imported (``linear_operator`` is not installed), bound to a
stub that holds ``lengthscale`` [*batch, 1, 1 or d].  This script supplies its own small stand-ins for what that method calls: ``covar_dist`` (the
plain Euclidean distance of the already scaled inputs), ``KroneckerProductLinearOperator.to_dense`` (torch.kron per batch member), the module
constants ``sqrt5`` and ``five_thirds`` and the parent's ``forward(diag=True)`` (ones).

``matern52grad_values.npz`` holds numeric arrays only: per case x1, x2, ls, K and the diag flag.  The case table is make_rbfgrad_golden.py's.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, _extract_method  # noqa: E402
from make_rbfgrad_golden import CASES, _Kron, _Parent  # noqa: E402


def main():
    if not os.path.isdir(REF):
        sys.exit("reference not mounted; fixtures are generated in the build container only")
    ns = {"torch": torch, "KroneckerProductLinearOperator": _Kron, "sqrt5": math.sqrt(5), "five_thirds": 5.0 / 3.0, "super": lambda: _Parent}
    fwd = _extract_method(f"{REF}/kernels/matern52_kernel_grad.py", "Matern52KernelGrad", "forward", ns)

    def covar_dist(self, x1, x2, diag=False, **params):
        assert not diag
        return (x1.unsqueeze(-2) - x2.unsqueeze(-3)).pow(2).sum(-1).sqrt()

    Ref = type("RefMatern52KernelGrad", (), {"forward": fwd, "covar_dist": covar_dist})
    out = {}
    for name, n, m, d, same, ard, dt, diag, batch in CASES:
        g = torch.Generator().manual_seed(5200 + ord(name))
        x1 = 2.0 * torch.rand(*batch, n, d, generator=g, dtype=dt)
        x2 = x1.clone() if same else 2.0 * torch.rand(*batch, m, d, generator=g, dtype=dt)
        k = Ref()
        k.lengthscale = 0.4 + 0.8 * torch.rand(*batch, 1, d if ard else 1, generator=g, dtype=dt)
        K = k.forward(x1, x2, diag=diag)
        out.update({f"{name}_x1": x1.numpy(), f"{name}_x2": x2.numpy(), f"{name}_ls": k.lengthscale.numpy(), f"{name}_K": K.numpy(),
                    f"{name}_diag": np.array(diag)})
        print(name, tuple(K.shape), K.dtype)
    np.savez_compressed(os.path.join(OUT, "matern52grad_values.npz"), **out)
    print("wrote matern52grad_values.npz with", len(out), "arrays")


if __name__ == "__main__":
    main()
