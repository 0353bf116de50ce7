#!/usr/bin/env python3
"""Golden fixture of the RBF kernel with first- and second-derivative observations, made by EXECUTING the reference's own code in the build container
(``python tests/golden/make_rbfgradgrad_golden.py``; see make_golden.py for the approach and for what may be committed: outputs only).

What is executed from the reference (nothing is copied into the repo): ``gpytorch/kernels/rbf_kernel_gradgrad.py`` -> the method
``RBFKernelGradGrad.forward``, extracted with ``ast`` and bound to a stub that holds ``lengthscale`` [*batch, 1, 1 or d], with the stand-ins of
make_rbfgrad_golden.py for what the method calls (``covar_dist``, ``postprocess_rbf``, ``KroneckerProductLinearOperator.to_dense``, the parent's
``forward(diag=True)``).

The case table is make_rbfgrad_golden.py's with every n1 != n2 case replaced by n1 == n2 with x1 != x2: the reference's ``forward`` raises a shape
mismatch for n1 != n2 (at the line forming ``K_31``), so two different clouds of the same size are the only two-input form it can evaluate.

``rbfgradgrad_values.npz`` holds numeric arrays only: per case x1, x2, ls, K and the diag flag.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, _extract_method  # noqa: E402
from make_rbfgrad_golden import CASES as GRAD_CASES, _Kron, _Parent  # noqa: E402

# name, n, m (= n), d, same, ard, dtype, diag, batch
CASES = [(name, n, n, d, same, ard, dt, diag, batch) for name, n, _, d, same, ard, dt, diag, batch in GRAD_CASES]


def main():
    if not os.path.isdir(REF):
        sys.exit("reference not mounted; fixtures are generated in the build container only")
    ns = {"torch": torch, "KroneckerProductLinearOperator": _Kron, "postprocess_rbf": lambda s: s.div(-2).exp(), "super": lambda: _Parent}
    fwd = _extract_method(f"{REF}/kernels/rbf_kernel_gradgrad.py", "RBFKernelGradGrad", "forward", ns)

    def covar_dist(self, x1, x2, square_dist=False, **params):
        assert square_dist
        return (x1.unsqueeze(-2) - x2.unsqueeze(-3)).pow(2).sum(-1)

    Ref = type("RefRBFKernelGradGrad", (), {"forward": fwd, "covar_dist": covar_dist})
    out = {}
    for name, n, m, d, same, ard, dt, diag, batch in CASES:
        g = torch.Generator().manual_seed(5000 + ord(name))
        x1 = 2.0 * torch.rand(*batch, n, d, generator=g, dtype=dt)
        x2 = x1.clone() if same else 2.0 * torch.rand(*batch, m, d, generator=g, dtype=dt)
        k = Ref()
        k.lengthscale = 0.4 + 0.8 * torch.rand(*batch, 1, d if ard else 1, generator=g, dtype=dt)
        K = k.forward(x1, x2, diag=diag)
        out.update({f"{name}_x1": x1.numpy(), f"{name}_x2": x2.numpy(), f"{name}_ls": k.lengthscale.numpy(), f"{name}_K": K.numpy(),
                    f"{name}_diag": np.array(diag)})
        print(name, tuple(K.shape), K.dtype)
    np.savez_compressed(os.path.join(OUT, "rbfgradgrad_values.npz"), **out)
    print("wrote rbfgradgrad_values.npz with", len(out), "arrays")


if __name__ == "__main__":
    main()
