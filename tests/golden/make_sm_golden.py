#!/usr/bin/env python3
"""Golden fixture of the spectral-mixture family, made by EXECUTING the reference's own code in the build container
(``python tests/golden/make_sm_golden.py``; see make_golden.py for the approach and for what may be committed: outputs only).

What is executed from the reference (nothing is copied into the repo): ``gpytorch/kernels/spectral_mixture_kernel.py`` -> the methods
``SpectralMixtureKernel.forward`` and ``SpectralMixtureKernel._create_input_grid``, extracted with ``ast`` because the package cannot be imported
(``linear_operator`` is not installed), bound to a stub that holds ``mixture_weights`` [Q], ``mixture_means`` / ``mixture_scales`` [Q, 1, d],
``ard_num_dims`` and ``num_mixtures``.

``sm_values.npz`` holds numeric arrays only: per case x1, x2, w, mu, sigma, K and the two flags (diag, last_dim_is_batch).
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, _extract_method  # noqa: E402

CASES = [  # name, n, m, d, Q, same, dtype, diag, last_dim_is_batch
    ("a", 24, 24, 1, 1, True, torch.float64, False, False),
    ("b", 18, 26, 1, 4, False, torch.float64, False, False),
    ("c", 22, 22, 1, 8, True, torch.float32, False, False),
    ("d", 17, 23, 2, 3, False, torch.float64, False, False),
    ("e", 20, 20, 3, 4, True, torch.float64, False, False),
    ("f", 21, 27, 3, 4, False, torch.float32, False, False),
    ("g", 19, 19, 2, 3, False, torch.float64, True, False),
    ("h", 16, 21, 2, 3, False, torch.float64, False, True),
]


def main():
    if not os.path.isdir(REF):
        sys.exit("reference not mounted; fixtures are generated in the build container only")
    path = f"{REF}/kernels/spectral_mixture_kernel.py"
    ns = {"torch": torch, "math": math}
    Ref = type("RefSpectralMixture", (), {"forward": _extract_method(path, "SpectralMixtureKernel", "forward", dict(ns)),
                                          "_create_input_grid": _extract_method(path, "SpectralMixtureKernel", "_create_input_grid", dict(ns))})
    out = {}
    for name, n, m, d, q, same, dt, diag, ldb in CASES:
        g = torch.Generator().manual_seed(3000 + ord(name))
        x1 = torch.rand(n, d, generator=g, dtype=dt)
        x2 = x1.clone() if same else torch.rand(m, d, generator=g, dtype=dt)
        k = Ref()
        k.num_mixtures, k.ard_num_dims = q, d
        k.mixture_weights = 0.3 + torch.rand(q, generator=g, dtype=dt)
        k.mixture_means = 0.5 + 2.5 * torch.rand(q, 1, d, generator=g, dtype=dt)
        k.mixture_scales = 0.9 + 0.5 * torch.rand(q, 1, d, generator=g, dtype=dt)
        K = k.forward(x1, x2, diag=diag, last_dim_is_batch=ldb)
        out.update({f"{name}_x1": x1.numpy(), f"{name}_x2": x2.numpy(), f"{name}_w": k.mixture_weights.numpy(), f"{name}_mu": k.mixture_means.numpy(),
                    f"{name}_sigma": k.mixture_scales.numpy(), f"{name}_K": K.numpy(), f"{name}_diag": np.array(diag), f"{name}_ldb": np.array(ldb)})
        print(name, tuple(K.shape), K.dtype)
    np.savez_compressed(os.path.join(OUT, "sm_values.npz"), **out)
    print("wrote sm_values.npz with", len(out), "arrays")


if __name__ == "__main__":
    main()
