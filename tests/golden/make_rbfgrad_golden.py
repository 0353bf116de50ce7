#!/usr/bin/env python3
"""Golden fixture of the RBF kernel with derivative observations, made by EXECUTING the reference's own code in the build container
(``python tests/golden/make_rbfgrad_golden.py``; see make_golden.py for the approach and for what may be committed: outputs only).

What is executed from the reference (nothing is copied into the repo): ``gpytorch/kernels/rbf_kernel_grad.py`` -> the method
``RBFKernelGrad.forward``, extracted with ``ast`` because the package cannot be imported (``linear_operator`` is not installed), bound to a stub
that holds ``lengthscale`` [*batch, 1, 1 or d].  This script supplies its own small stand-ins for what that method calls: ``covar_dist`` (squared
distances of the already scaled inputs), ``postprocess_rbf`` (exp(-s / 2)), ``KroneckerProductLinearOperator.to_dense`` (torch.kron per batch
member) and the parent's ``forward(diag=True)`` (ones).

``rbfgrad_values.npz`` holds numeric arrays only: per case x1, x2, ls, K and the diag flag.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, _extract_method  # noqa: E402

CASES = [  # name, n, m, d, same, ard, dtype, diag, batch
    ("a", 9, 9, 1, True, False, torch.float64, False, ()),
    ("b", 7, 12, 1, False, True, torch.float64, False, ()),
    ("c", 10, 10, 2, True, True, torch.float64, False, ()),
    ("d", 11, 6, 2, False, False, torch.float32, False, ()),
    ("e", 8, 8, 3, True, True, torch.float32, False, ()),
    ("f", 5, 12, 3, False, True, torch.float64, False, ()),
    ("g", 12, 12, 4, True, False, torch.float64, False, ()),
    ("h", 6, 9, 4, False, True, torch.float64, False, ()),
    ("i", 7, 7, 5, True, True, torch.float64, False, ()),
    ("j", 4, 10, 5, False, False, torch.float32, False, ()),
    ("k", 9, 9, 3, True, True, torch.float64, True, ()),
    ("l", 8, 8, 2, True, False, torch.float32, True, ()),
    ("m", 6, 7, 2, False, True, torch.float64, False, (3,)),
]


class _Kron:
    def __init__(self, a, b):
        self.a, self.b = a, b

    def to_dense(self):
        if self.a.dim() == 2:
            return torch.kron(self.a, self.b)
        return torch.stack([torch.kron(a, b) for a, b in zip(self.a.reshape(-1, *self.a.shape[-2:]), self.b.reshape(-1, *self.b.shape[-2:]))]).reshape(
            *self.a.shape[:-2], self.a.shape[-2] * self.b.shape[-2], self.a.shape[-1] * self.b.shape[-1])


class _Parent:
    @staticmethod
    def forward(x1, x2, diag=False):
        assert diag
        return torch.ones(*x1.shape[:-1], dtype=x1.dtype)


def main():
    if not os.path.isdir(REF):
        sys.exit("reference not mounted; fixtures are generated in the build container only")
    ns = {"torch": torch, "KroneckerProductLinearOperator": _Kron, "postprocess_rbf": lambda s: s.div(-2).exp(), "super": lambda: _Parent}
    fwd = _extract_method(f"{REF}/kernels/rbf_kernel_grad.py", "RBFKernelGrad", "forward", ns)

    def covar_dist(self, x1, x2, square_dist=False, **params):
        assert square_dist
        return (x1.unsqueeze(-2) - x2.unsqueeze(-3)).pow(2).sum(-1)

    Ref = type("RefRBFKernelGrad", (), {"forward": fwd, "covar_dist": covar_dist})
    out = {}
    for name, n, m, d, same, ard, dt, diag, batch in CASES:
        g = torch.Generator().manual_seed(4000 + ord(name))
        x1 = 2.0 * torch.rand(*batch, n, d, generator=g, dtype=dt)
        x2 = x1.clone() if same else 2.0 * torch.rand(*batch, m, d, generator=g, dtype=dt)
        k = Ref()
        k.lengthscale = 0.4 + 0.8 * torch.rand(*batch, 1, d if ard else 1, generator=g, dtype=dt)
        K = k.forward(x1, x2, diag=diag)
        out.update({f"{name}_x1": x1.numpy(), f"{name}_x2": x2.numpy(), f"{name}_ls": k.lengthscale.numpy(), f"{name}_K": K.numpy(),
                    f"{name}_diag": np.array(diag)})
        print(name, tuple(K.shape), K.dtype)
    np.savez_compressed(os.path.join(OUT, "rbfgrad_values.npz"), **out)
    print("wrote rbfgrad_values.npz with", len(out), "arrays")


if __name__ == "__main__":
    main()
