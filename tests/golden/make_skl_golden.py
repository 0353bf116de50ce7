#!/usr/bin/env python3
"""Golden fixture of the symmetrized-KL kernel over Gaussian inputs, made by EXECUTING the reference's own code in the build container
(``python tests/golden/make_skl_golden.py``; see make_golden.py for the approach and for what may be committed: outputs only).

What is executed from the reference (nothing is copied into the repo):
  * ``gpytorch/kernels/gaussian_symmetrized_kl_kernel.py`` -> the function ``_symmetrized_kl``, extracted with ``ast`` because the package cannot
    be imported (``linear_operator`` is not installed);
  * ``gpytorch/kernels/distributional_input_kernel.py`` -> the method ``DistributionalInputKernel.forward``, extracted the same way and bound to a
    stub that carries ``distance_function`` and ``lengthscale``.

``skl_values.npz`` holds numeric arrays only: per case x1, x2 (two clouds only), S = _symmetrized_kl(x1, x2), K = forward(x1, x2) at lengthscale d and
the diagonal forward(x1[:k], x2[:k], diag=True).  Case names are ``d<d><e|t><64|32>``: dimensions, x1 = x2 (e) or two clouds (t), dtype.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import OUT, REF, _extract_functions, _extract_method  # noqa: E402

DIMS = (1, 2, 3, 6)


def main():
    if not os.path.isdir(REF):
        sys.exit("reference not mounted; fixtures are generated in the build container only")
    (skl,) = _extract_functions(f"{REF}/kernels/gaussian_symmetrized_kl_kernel.py", ["_symmetrized_kl"])
    fwd = _extract_method(f"{REF}/kernels/distributional_input_kernel.py", "DistributionalInputKernel", "forward", {"torch": torch})
    out, idx = {}, 0
    for d in DIMS:
        for same in (True, False):
            for dt in (torch.float64, torch.float32):
                name = f"d{d}{'e' if same else 't'}{'64' if dt == torch.float64 else '32'}"
                g = torch.Generator().manual_seed(6100 + idx)
                n, m = 8 + idx % 4, 7 + (idx * 5) % 4

                def cloud(rows):   # mu uniform in [0, 1]^d, log sigma^2 uniform in [-3, -1]
                    return torch.cat([torch.rand(rows, d, generator=g, dtype=dt), -3.0 + 2.0 * torch.rand(rows, d, generator=g, dtype=dt)], -1)

                x1 = cloud(n)
                x2 = x1.clone() if same else cloud(m)
                k = min(n, x2.shape[0])
                ker = type("RefKernel", (), {"forward": fwd, "distance_function": staticmethod(skl), "lengthscale": torch.tensor([[float(d)]], dtype=dt)})()
                out[f"{name}_x1"] = x1.numpy()
                if not same:
                    out[f"{name}_x2"] = x2.numpy()
                out[f"{name}_S"] = skl(x1, x2).numpy()
                out[f"{name}_K"] = ker.forward(x1, x2).numpy()
                out[f"{name}_diag_pair"] = ker.forward(x1[:k], x2[:k], diag=True).numpy()
                print(name, "K", out[f"{name}_K"].shape, out[f"{name}_K"].dtype, "mean", round(float(out[f"{name}_K"].mean()), 3))
                idx += 1
    np.savez_compressed(os.path.join(OUT, "skl_values.npz"), **out)
    print("wrote skl_values.npz with", len(out), "arrays")


if __name__ == "__main__":
    main()
