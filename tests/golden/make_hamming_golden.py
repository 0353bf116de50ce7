#!/usr/bin/env python3
"""Golden fixture of the inverse-multiquadric Hamming kernel, made by EXECUTING the reference's own code in the build container
(``python tests/golden/make_hamming_golden.py``; see make_golden.py for the approach and for what may be committed: outputs only).

What is executed from the reference (nothing is copied into the repo), all from ``gpytorch/kernels/hamming_kernel.py``, extracted with ``ast``
because the package cannot be imported (``linear_operator`` is not installed):
  * the methods ``HammingIMQKernel.forward`` and ``HammingIMQKernel._imq``, bound to a stub that carries ``vocab_size``, ``alpha``, ``beta`` ([1]
    tensors, as the kernel's properties return them without a batch shape) and an empty ``batch_shape``;
  * the module-level function ``hamming_dist`` that ``forward`` calls.

``hamming_values.npz`` holds numeric arrays only: per case x1, x2 (one-hot, flattened), alpha, beta, K = forward(x1, x2) and the diagonals
forward(x1, x1, diag=True), forward(x1[:k], x2[:k], diag=True).  Case names are ``t<T>v<V><e|t><64|32>``: positions, vocabulary, x1 = x2 (e) or
two clouds (t), dtype.
"""
from __future__ import annotations

import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import OUT, REF, _extract_method  # noqa: E402
from hamming_ref import one_hot, random_tokens  # noqa: E402

SHAPES = ((1, 2), (3, 4), (5, 20))   # (T, V)


def cases():
    """(name, n, m, T, V, same, dtype): every shape, one and two clouds, both dtypes; n in 12..17."""
    out, i = [], 0
    for t, v in SHAPES:
        for same in (True, False):
            for dt in (torch.float64, torch.float32):
                n = 12 + (i % 6)
                m = n if same else 11 + ((i * 5) % 7)
                out.append((f"t{t}v{v}{'e' if same else 't'}{'64' if dt == torch.float64 else '32'}", n, m, t, v, same, dt))
                i += 1
    return out


def _extract_function(path, name, ns):
    """The module-level FunctionDef ``name`` of ``path`` compiled in ``ns``, annotations dropped (they name typing aliases)."""
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.FunctionDef) and node.name == name:
            node.returns = None
            for a in node.args.args + node.args.kwonlyargs:
                a.annotation = None
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
            return ns[name]
    raise KeyError(name)


def main():
    if not os.path.isdir(REF):
        sys.exit("reference not mounted; fixtures are generated in the build container only")
    path = f"{REF}/kernels/hamming_kernel.py"
    ns = {"torch": torch}
    _extract_function(path, "hamming_dist", ns)
    fwd = _extract_method(path, "HammingIMQKernel", "forward", ns)
    imq = _extract_method(path, "HammingIMQKernel", "_imq", ns)
    RefHamming = type("RefHamming", (), {"forward": fwd, "_imq": imq, "batch_shape": torch.Size([])})
    out = {}
    for idx, (name, n, m, t, v, same, dt) in enumerate(cases()):
        tok1 = random_tokens(n, t, v, 7300 + idx)
        x1 = one_hot(tok1, v, dt)
        x2 = x1.clone() if same else one_hot(random_tokens(m, t, v, 7400 + idx, close_to=tok1), v, dt)
        k = min(n, x2.shape[0])
        ker = RefHamming()
        ker.vocab_size = v
        ker.alpha = torch.tensor([0.3 + 0.45 * (idx % 7)], dtype=dt)
        ker.beta = torch.tensor([0.5 + 0.5 * (idx % 6)], dtype=dt)
        out.update({f"{name}_x1": x1.numpy(), f"{name}_x2": x2.numpy(), f"{name}_alpha": ker.alpha.numpy(), f"{name}_beta": ker.beta.numpy()})
        out[f"{name}_K"] = ker.forward(x1, x2).numpy()
        out[f"{name}_diag_same"] = ker.forward(x1, x1, diag=True).numpy()
        out[f"{name}_diag_pair"] = ker.forward(x1[:k], x2[:k], diag=True).numpy()
        print(name, "K", out[f"{name}_K"].shape, out[f"{name}_K"].dtype, "mean", round(float(out[f"{name}_K"].mean()), 3))
    np.savez_compressed(os.path.join(OUT, "hamming_values.npz"), **out)
    print("wrote hamming_values.npz with", len(out), "arrays")


if __name__ == "__main__":
    main()
